"""Relighting in the photograph on the CPU ("Relighting in the photograph"; no GPU): the header against the
binding, every refusal of the three entries through raw ctypes before anything is launched, the quotient composite's CPU twin against
an fp64 restatement and at its exact cases, the default floor, the fp64 reference's own property (two replays, one walk), and the
refusals of `render_real` and `render_rolling_envmap` before any device is touched."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import path_relight_fp64 as pr  # noqa: E402
import path_testlib as tl  # noqa: E402

INVALID_ARG = -1
RENDER, COMPOSITE, COMPOSITE_HOST = "matpbr_path_render_relight", "matpbr_path_composite_relight", "matpbr_path_composite_relight_host"
FEATURE = "relighting in the photograph"
_report = tl.reporter("path relight host", "test_path_relight_host")
_u32 = lambda x: np.ascontiguousarray(x).view(np.uint32)


@pytest.fixture(scope="module")
def path_lib():
    return tl.load()


def test_the_header_declares_what_the_binding_binds(path_lib):
    with open(os.path.join(ROOT, "include", "matpbr_path.h")) as f:
        raw = f.read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(matpbr_path_\w+)\s*\(", text))
    assert path_lib.RELIGHT_SYMBOLS == (RENDER, COMPOSITE, COMPOSITE_HOST) and set(path_lib.RELIGHT_SYMBOLS) <= declared
    assert not set(path_lib.RELIGHT_SYMBOLS) & set(path_lib.LATE_SYMBOLS)          # a group beside LATE_SYMBOLS, as the last five are
    assert list(path_lib.FEATURE_SYMBOLS)[-1] == FEATURE and len(path_lib.FEATURE_SYMBOLS) == 16
    assert path_lib.FEATURE_SYMBOLS[FEATURE] == path_lib.RELIGHT_SYMBOLS
    assert re.search(r"#define MATPBR_PATH_VERSION 3\b", raw)
    lib = path_lib.load()
    assert lib.matpbr_path_version() == path_lib.VERSION == 3
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    render = path_lib.SIGNATURES["matpbr_path_render"][1]
    want = {RENDER: render[:18] + render[19:] + [P] * 4 + [I, I] + [P] * 3,        # the render's arguments without `out`, then the nine of its own
            COMPOSITE: [P] * 3 + [I, I, F, F, P, P], COMPOSITE_HOST: [P] * 3 + [I, I, F, F, P]}
    for name in path_lib.RELIGHT_SYMBOLS:
        assert hasattr(lib, name), name                                            # the built library exports it
        fn = path_lib.symbol(name, lib)
        res, args = path_lib.SIGNATURES[name]
        assert fn.argtypes == args == want[name] and fn.restype == res == I, name
    for name in ("pathtrace", "path_filters"):
        mod = __import__("materialist_amd." + name, fromlist=[name])
        assert callable(mod.composite_relight) and callable(mod.composite_relight_host) and mod.RELIGHT_FLOOR == 0.01
    assert callable(path_lib.PathTracer.render_relight)

    class Old:
        pass

    for name in path_lib.RELIGHT_SYMBOLS:
        with pytest.raises(path_lib.PathError, match=name + ".*" + FEATURE):
            path_lib.symbol(name, Old())


_RAW = np.zeros(18, np.float64)
PTR = _RAW[(-_RAW.ctypes.data % 16) // 8:][:16].ctypes.data   # what every pointer of a refused call points at: it is never read
FRAME = ("nodes", "tris", "a", "r", "m", "H", "W", "fov", "env", "row_cdf", "col_cdf", "env_pdf", "He", "We", "spp", "max_depth", "seed", "spp_per_launch")
GOOD = dict(zip(FRAME, [PTR] * 5 + [4, 6, 35.0] + [PTR] * 4 + [2, 4, 3, 4, 0, 2]))
GOOD.update(rays=None, stream=None, env_b=PTR, row_cdf_b=PTR, col_cdf_b=PTR, env_pdf_b=PTR, He_b=2, We_b=4, nrm=None, base=PTR, relit=PTR)
# every term of the validity condition, broken one at a time: matpbr_path_render's, then the entry's own
BROKEN = [(k, None) for k in ("nodes", "tris", "a", "r", "m", "env", "row_cdf", "col_cdf", "env_pdf")] + \
         [(k, v) for k in ("H", "W", "He", "We", "spp", "spp_per_launch") for v in (0, -1)] + \
         [("max_depth", 0), ("max_depth", 17), ("fov", 0.0), ("fov", 180.0), ("fov", float("nan"))] + \
         [(k, None) for k in ("env_b", "row_cdf_b", "col_cdf_b", "env_pdf_b", "base", "relit")] + \
         [(k, v) for k in ("He_b", "We_b") for v in (0, -3)]


@pytest.mark.parametrize("nrm", [None, PTR], ids=["face", "map"])
def test_render_relight_refuses_without_a_device(path_lib, nrm):
    """Every pointer a non-null dummy that a refusing call never reads; each case is invalid in exactly one respect and returns
    MATPBR_PATH_ERR_INVALID_ARG before any launch (the call these start from is accepted on the GPU: test_gpu_path_relight.py)."""
    fn = path_lib.symbol(RENDER)
    assert len(GOOD) == len(path_lib.SIGNATURES[RENDER][1])
    for key, bad in BROKEN:
        args = {**GOOD, "nrm": nrm, "rays": nrm, key: bad}                        # rays and nrm are the nullable ones: both ways
        assert fn(*args.values()) == INVALID_ARG, (key, bad)


def test_the_composites_refuse(path_lib):
    H, W = 3, 5
    img = np.ones((H, W, 3), np.float32)
    out = np.empty_like(img)
    good = dict(base=img.ctypes.data, relit=img.ctypes.data, photo=img.ctypes.data, H=H, W=W, scale=1.0, floor=0.5, out=out.ctypes.data)
    host, dev = path_lib.symbol(COMPOSITE_HOST), path_lib.symbol(COMPOSITE)
    assert host(*good.values()) == 0 and np.array_equal(out, img)
    broken = [(k, None) for k in ("base", "relit", "photo", "out")] + [(k, v) for k in ("H", "W") for v in (0, -2)] + \
             [(k, v) for k in ("scale", "floor") for v in (0.0, -1.0, float("inf"), float("nan"))]
    for key, bad in broken:
        args = {**good, key: bad}
        assert host(*args.values()) == INVALID_ARG, (key, bad)
        assert dev(*args.values(), None) == INVALID_ARG, (key, bad)               # validation precedes the launch: no device is needed
    for fn in (path_lib.composite_relight_host, path_lib.composite_relight):       # the same words on both sides, before a device is touched
        with pytest.raises(ValueError, match=r"photo must be \[H,W,3\]"):
            fn(img, img, img[..., 0])
        with pytest.raises(ValueError, match=r"relit must be \[3, 5, 3\], got \[2, 5, 3\]"):
            fn(img, img[1:], img)
        with pytest.raises(ValueError, match=r"base must be \[3, 5, 3\]"):
            fn(img[:, 1:], img, img)
        with pytest.raises(ValueError, match="scale must be finite and positive"):
            fn(img, img, img, 0.0)
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="floor must be finite and positive"):
                fn(img, img, img, 1.0, bad)


def _images(H=20, W=24, seed=5):
    rng = np.random.default_rng(seed)
    base = rng.gamma(2.0, 0.5, (H, W, 3)).astype(np.float32)
    relit = rng.gamma(2.0, 0.5, (H, W, 3)).astype(np.float32)
    photo = rng.gamma(2.0, 0.5, (H, W, 3)).astype(np.float32)
    base[2, 3] = 0.0                                       # a channel triple the model sees no light in,
    relit[4, 5] = 0.0                                      # one the new light leaves dark
    base[6, 7] = relit[6, 7] = 0.0                         # and both
    return base, relit, photo


def test_the_host_composite_against_fp64(path_lib):
    """`composite_relight_host` against max(0, photo (relit scale + floor) / (base scale + floor)) in fp64, within 2 ulp, the ulp taken as
    float32's machine epsilon relative to the value, 2^-23 |x|.  The scales are powers of two, so the two products by `scale` are exact;
    the two sums, the division and the last product are correctly rounded, a relative error of at most 2^-24 each, and relative errors
    add along a quotient and a product: at most 4 x 2^-24 = 2 ulp, whatever the inputs.  (Counted in the spacing of float32 at the
    result, which is 2^-23 |x| at the bottom of a binade and half that at its top, the same four roundings may reach just under 4: these
    images give 2.01 at one value.  That figure is printed beside the other; it is not the bound.)"""
    base, relit, photo = _images()
    worst, worst_spacing = 0.0, 0.0
    for scale, floor in ((1.0, 0.02), (0.25, 1e-3), (1.0, 3.0)):
        got = path_lib.composite_relight_host(base, relit, photo, scale, floor).astype(np.float64)
        want = pr.composite(base, relit, photo, scale, np.float32(floor))
        ulps = np.abs(got - want) / (2.0 ** -23 * np.maximum(np.abs(want), np.finfo(np.float32).tiny))
        worst = max(worst, float(ulps.max()))
        worst_spacing = max(worst_spacing, float((np.abs(got - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)).max()))
        assert ulps.max() <= 2.0, (scale, floor, ulps.max())
        g_max = (relit.astype(np.float64) * scale + floor) / floor
        assert (got <= photo * g_max * (1 + 2.0 ** -22)).all()                     # the floor bounds the quotient
    _report("composite_relight_host against fp64: largest error in ulp = 2^-23 |x| (bound 2); the same in the spacing at the result",
            f"{worst:.3f}; {worst_spacing:.3f}")


def test_the_exact_cases_of_the_composite(path_lib):
    base, relit, photo = _images()
    for scale, floor in ((1.0, 0.02), (0.125, 1e-3)):
        same = path_lib.composite_relight_host(base, base.copy(), photo, scale, floor)
        assert np.array_equal(_u32(same), _u32(photo))                             # g is exactly 1: the photograph's bits, dark texels included
        dark = path_lib.composite_relight_host(base, np.zeros_like(base), photo, scale, floor)
        fl, sc = np.float32(floor), np.float32(scale)
        want = np.maximum(np.float32(0), photo * (fl / (base * sc + fl)))          # photo floor / (B0 + floor), each operation in float32
        assert np.array_equal(_u32(dark), _u32(want))
        assert (dark <= photo).all() and np.array_equal(_u32(dark[2, 3]), _u32(photo[2, 3]))   # where the model is dark too the ratio is 1
    neg = path_lib.composite_relight_host(base, relit, -photo, 1.0, 0.02)
    assert not neg.any()                                                           # max(0, .)


def test_the_default_floor(path_lib):
    """floor=None is 0.01 x mean(base scale) over all pixels and channels, formed in fp64 and rounded once."""
    base, relit, photo = _images()
    for scale in (1.0, 0.5):
        floor = np.float32(0.01 * scale * base.mean(dtype=np.float64))
        got = path_lib.composite_relight_host(base, relit, photo, scale)
        assert np.array_equal(_u32(got), _u32(path_lib.composite_relight_host(base, relit, photo, scale, float(floor))))
        assert not np.array_equal(got, path_lib.composite_relight_host(base, relit, photo, scale, 2 * float(floor)))
    with pytest.raises(ValueError, match="base has no light"):
        path_lib.composite_relight_host(np.zeros_like(base), relit, photo)


def test_two_replays_record_one_walk(path_lib, oracle64):
    """The property the kernel rests on, in fp64 on the tests' groove: under A, under A rolled, under the 4 x 8 envmap and under the
    all-zero envmap (no tables: no emitter samples at all) the replays record the same vertices.  `reference` asserts it."""
    s = pr.relight_scene(path_lib)
    assert s["tab_zero"]["row_cdf"][-1] == 0 and s["tab_b"]["row_cdf"][-1] > 0 and s["env_small"].shape == (4, 8, 3)
    for b in ("env_b", "env_small", "env_zero"):
        for normal in (False, True):
            ref = pr.reference(oracle64, s, 4, 0, normal=normal, b=b)
            n_vert = sum(v["pix"].size for v in ref["rec"][0]["vertices"])
            assert n_vert > s["H"] * s["W"] and np.isfinite(ref["relit"]).all()
    ref = pr.reference(oracle64, s, 4, 0)
    differ = float((ref["base"] != ref["relit"]).any(-1).mean())
    _report("max_depth 4 seed 0: share of pixels whose radiance differs between A and A rolled by 8 columns", f"{differ:.4f}")
    assert differ > 0.9 and not pr.reference(oracle64, s, 4, 0, b="env_zero")["relit"].any()
    same = pr.reference(oracle64, s, 4, 0, b="env")
    assert np.array_equal(same["base"], same["relit"])


KW = dict(save_path=None, device="nowhere")


def test_render_real_and_rolling_refuse_before_any_work(path_lib, tmp_path):
    """`relight_composite=True` raises ValueError for what it does not do, and for a missing photograph, before the scene is read or a
    device touched (there is neither here)."""
    from materialist_amd import relight

    kw = dict(input_path=str(tmp_path), save_path=str(tmp_path), device="nowhere")
    ok = dict(integrator="path", relight_composite=True)
    edit = {"albedo": None, "roughness": 0.2, "metallic": None}
    none = {"albedo": None, "roughness": None, "metallic": None}
    real = lambda **k: relight.render_real("nothing", "new.hdr", **{**ok, **k}, **kw)
    rolling = lambda **k: relight.render_rolling_envmap("nothing", None, 2, 90.0, **{**ok, **k}, **kw)
    for call in (real, rolling):
        with pytest.raises(ValueError, match="relight_composite needs integrator='path'"):
            call(integrator="sh")
        for e in (edit, {"albedo": [0.1, 0, 0]}, {"metallic": 1.0}):
            with pytest.raises(ValueError, match="relight_composite knows no material edit"):
                call(edit=e)
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="relight_floor must be finite and > 0"):
                call(relight_floor=bad)
        with pytest.raises(ValueError, match="composite needs the photograph: .*gt_image.exr does not exist"):
            call(edit=none)
        with pytest.raises(ValueError, match="composite needs the photograph: .*no_such.exr does not exist"):
            call(relight_photo=os.path.join(str(tmp_path), "no_such.exr"))
        for alone in ({"relight_photo": "p.exr"}, {"relight_floor": 0.1}):
            with pytest.raises(ValueError, match="relight_photo and relight_floor need relight_composite=True"):
                call(relight_composite=False, **alone)
    with pytest.raises(ValueError, match="relight_composite knows no edit composite"):
        real(composite=True, edit=edit)
    with pytest.raises(ValueError, match="relight_composite needs a new light"):
        relight.render_real("nothing", None, **ok, **kw)
    with pytest.raises(ValueError, match="composite needs the photograph"):          # a scale alone is a new light
        relight.render_real("nothing", None, env_scale=2.0, **ok, **kw)
    with pytest.raises(ValueError, match="No envmap found"):                        # without it they go on to look for the scene
        relight.render_rolling_envmap("nothing", None, 2, 90.0, integrator="path", **kw)


def test_the_command_line(path_lib, tmp_path):
    import render_final

    base = ["--save_name", "case", "--integrator", "path"]
    a = render_final.parse_args(base + ["--mode", "real", "--env_path", "x.hdr", "--relight_composite"])
    assert a.relight_composite and a.relight_photo is None and a.relight_floor is None
    a = render_final.parse_args(base + ["--mode", "rolling", "--relight_composite", "--relight_photo", "p.exr", "--relight_floor", "0.05",
                                        "--shading_normals", "map", "--denoise", "atrous", "--spp", "4"])
    assert a.relight_photo == "p.exr" and a.relight_floor == 0.05 and a.shading_normals == "map" and a.denoise == "atrous"
    assert not render_final.parse_args(base + ["--mode", "real"]).relight_composite
    for alone in (["--relight_photo", "p.exr"], ["--relight_floor", "0.1"]):
        with pytest.raises(SystemExit):
            render_final.parse_args(base + ["--mode", "real"] + alone)
    where = ["--input_path", str(tmp_path), "--save_path", str(tmp_path)]
    refused = {"knows no --mode oi": ["--mode", "oi"], "needs integrator='path'": ["--mode", "real", "--integrator", "sh", "--env_path", "x.hdr"],
               "knows no material edit": ["--mode", "rolling", "--edit_metallic", "1"],
               "knows no edit composite": ["--mode", "real", "--env_path", "x.hdr", "--edit_roughness", "0.2", "--edit_composite"],
               "needs a new light": ["--mode", "real"]}
    for words, argv in refused.items():
        with pytest.raises(ValueError, match=words):
            render_final.main(base + where + ["--relight_composite"] + argv)
