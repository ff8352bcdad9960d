"""Material edits in the photograph on the CPU ("Material edits in the photograph"; no GPU): the header against
the binding, the refusals of `matpbr_path_render_edit_diff` before it launches anything, `relight.edit_mask`, what the existing
composite does with a differential render that has no foreground, the fp64 reference's own bracket, and the refusals of the command
line and of `render_real(composite=True)` before any work."""
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

import path_mapedit_fp64 as pm  # noqa: E402
import path_testlib as tl  # noqa: E402

INVALID_ARG = -1
NAME = "matpbr_path_render_edit_diff"
_report = tl.reporter("path mapedit host", "test_path_mapedit_host")
_u32 = lambda x: np.ascontiguousarray(x).view(np.uint32)


@pytest.fixture(scope="module")
def path_lib():
    return tl.load()


def test_the_header_declares_what_the_binding_binds(path_lib):
    with open(os.path.join(ROOT, "include", "matpbr_path.h")) as f:
        raw = f.read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(matpbr_path_\w+)\s*\(", text))
    assert path_lib.MAPEDIT_SYMBOLS == (NAME,) and NAME in declared and NAME not in path_lib.LATE_SYMBOLS
    assert re.search(r"#define MATPBR_PATH_VERSION 3\b", raw)
    lib = path_lib.load()
    assert hasattr(lib, NAME)                                              # the built library exports it
    fn = path_lib.symbol(NAME, lib)
    res, args = path_lib.SIGNATURES[NAME]
    assert fn.argtypes == args and fn.restype == res
    P = ctypes.c_void_p
    render = path_lib.SIGNATURES["matpbr_path_render"][1]
    assert args == render[:18] + render[19:] + [P] * 8                     # the render's arguments without `out`, then the eight of its own
    assert lib.matpbr_path_version() == path_lib.VERSION == 3
    for name in ("pathtrace", "path_filters"):
        mod = __import__("materialist_amd." + name, fromlist=[name])
        assert callable(mod.composite_edit) and callable(mod.composite_edit_host)
    assert callable(path_lib.PathTracer.render_edit_diff) and callable(path_lib.edit_mask)

    class Old:
        pass

    with pytest.raises(path_lib.PathError, match=NAME + ".*material edits in the photograph"):
        path_lib.symbol(NAME, Old())


def test_null_arguments_are_refused_without_a_device(path_lib):
    """Every pointer a non-null dummy that a refusing call never reads: a null edited map, mask, delta or base, and a frame invalid in
    one respect, return MATPBR_PATH_ERR_INVALID_ARG (the call these start from is accepted on the GPU: test_gpu_path_mapedit.py)."""
    raw = np.zeros(18, np.float64)
    ptr = raw[(-raw.ctypes.data % 16) // 8:][:16].ctypes.data
    frame = [ptr] * 5 + [4, 6, 35.0] + [ptr] * 4 + [2, 4, 3, 4, 0, 2]
    own = {"a_e": ptr, "r_e": ptr, "m_e": ptr, "mask": ptr, "nrm": None, "delta": ptr, "base": ptr, "rewalked": None}
    fn = path_lib.symbol(NAME)
    assert len(frame) + 2 + len(own) == len(path_lib.SIGNATURES[NAME][1])
    call = lambda frame=frame, **spoil: fn(*frame, None, None, *{**own, **spoil}.values())
    for name in ("a_e", "r_e", "m_e", "mask", "delta", "base"):
        assert call(**{name: None}) == INVALID_ARG, name
        assert call(**{name: None, "nrm": ptr, "rewalked": ptr}) == INVALID_ARG, name
    assert call(frame[:14] + [0] + frame[15:]) == INVALID_ARG              # the frame's own checks: spp = 0,
    assert call(frame[:15] + [17] + frame[16:]) == INVALID_ARG             # max_depth beyond 16,
    assert call(frame[:2] + [None] + frame[3:]) == INVALID_ARG             # a null fitted map
    assert call(frame[:5] + [0] + frame[6:]) == INVALID_ARG                # and H = 0


def test_edit_mask(path_lib):
    from materialist_amd import relight

    rng = np.random.default_rng(3)
    H, W = 5, 7
    a, r, m = (rng.uniform(0.1, 0.9, s).astype(np.float32) for s in ((H, W, 3), (H, W, 1), (H, W, 1)))
    for fn in (relight.edit_mask, path_lib.edit_mask):
        same = fn((a, r, m), (a.copy(), r.copy(), m.copy()))
        assert tuple(same.shape) == (H, W) and same.dtype == __import__("torch").bool and not bool(same.any())
        for k, (i, j, c) in enumerate([(0, 0, 0), (2, 3, 2), (4, 6, 0), (1, 5, 0)]):     # one float of one texel, in each map
            maps = [a.copy(), r.copy(), m.copy()]
            which = k % 3
            x = maps[which]
            x[i, j, c if which == 0 else 0] = np.nextafter(x[i, j, c if which == 0 else 0], np.float32(2))
            got = fn((a, r, m), tuple(maps)).numpy()
            want = np.zeros((H, W), bool)
            want[i, j] = True
            assert np.array_equal(got, want), (k, which)
        # bitwise: -0.0 is another value than 0.0, though they compare equal; a NaN is the value it is
        z, zn = np.zeros((H, W, 1), np.float32), np.zeros((H, W, 1), np.float32)
        zn[3, 2] = -0.0
        assert (z == zn).all()
        got = fn((a, r, z), (a, r, zn)).numpy()
        assert got[3, 2] and got.sum() == 1
        nan = r.copy()
        nan[1, 1] = np.nan
        assert not bool(fn((a, nan, m), (a, nan.copy(), m)).any())
        assert np.array_equal(fn((a, r[..., 0], m[..., 0]), (a, r, zn)).numpy(), (m != zn)[..., 0])        # [H,W] and [H,W,1] alike
    with pytest.raises(ValueError, match="albedo must be"):
        relight.edit_mask((r, r, m), (r, r, m))


def test_the_composite_of_a_delta_alone(path_lib):
    """`composite_host(0, delta, 0, photo)`: the photograph's bits where delta is all-zero bits, max(0, photo + delta) elsewhere;
    `composite_edit_host` is that call, and with `base` `composite_ratio_host`'s."""
    rng = np.random.default_rng(8)
    H, W = 20, 24
    photo = rng.gamma(2.0, 0.5, (H, W, 3)).astype(np.float32)
    delta = rng.normal(0.0, 0.7, (H, W, 3)).astype(np.float32)
    keep = rng.uniform(size=(H, W)) < 0.6
    delta[keep] = 0.0
    base = rng.gamma(2.0, 0.5, (H, W, 3)).astype(np.float32)
    z3, z1 = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32)
    got = path_lib.composite_host(z3, delta, z1, photo)
    assert np.array_equal(_u32(got)[keep], _u32(photo)[keep])
    assert np.array_equal(_u32(got), _u32(np.maximum(np.float32(0), photo + delta)))
    assert (photo + delta < 0).any() and (got >= 0).all()
    assert np.array_equal(_u32(path_lib.composite_edit_host(delta, photo)), _u32(got))
    ratio = path_lib.composite_edit_host(delta, photo, base)
    assert np.array_equal(_u32(ratio), _u32(path_lib.composite_ratio_host(z3, delta, base, z1, photo)))
    assert np.array_equal(_u32(ratio)[keep], _u32(photo)[keep]) and (_u32(ratio) != _u32(got)).any()
    for fn in (path_lib.composite_edit_host, path_lib.composite_edit):     # the same words on both sides, before a device is touched
        with pytest.raises(ValueError, match=r"photo must be \[H,W,3\]"):
            fn(delta, z1)
        with pytest.raises(ValueError, match=r"delta must be \[20, 24, 3\]"):
            fn(z1, photo)


def test_the_reference_alone_has_the_bracket(path_lib, oracle64):
    """The fp64 reference of the GPU tests, max_depth 4, seed 0: between 0.05 and 0.3 of the pixels differ between the two walks, at
    least 0.03 of them outside the mask (inter-reflection), and no differing pixel is untouched: the touch rule is exact in fp64."""
    s = pm.edit_scene(path_lib)
    assert s["mask"].sum() == 63 and (s["H"], s["W"]) == (20, 24)
    assert np.array_equal(path_lib.edit_mask((s["a"], s["r"], s["m"]), s["edited"]).numpy(), s["mask"])
    ref = pm.reference(oracle64, s, 4, 0)
    outside = ref["differ"] & ~s["mask"]
    _report("max_depth 4 seed 0: touched share; differing share; differing outside the mask; differing and not touched",
            f"{ref['touched'].mean():.4f}; {ref['differ'].mean():.4f}; {outside.mean():.4f}; {int((ref['differ'] & ~ref['touched']).sum())}")
    assert 0.05 <= ref["differ"].mean() <= 0.3 and outside.mean() >= 0.03
    assert not (ref["differ"] & ~ref["touched"]).any()


PATH = ["--save_name", "case", "--mode", "real", "--integrator", "path", "--edit_roughness", "0.2"]


def test_the_command_line_refuses_what_the_composite_does_not_do(path_lib):
    import render_final

    a = render_final.parse_args(PATH + ["--edit_composite"])
    assert a.edit_composite and a.edit_photo is None and a.edit_transfer is None
    a = render_final.parse_args(PATH + ["--edit_composite", "--edit_photo", "p.exr", "--edit_transfer", "ratio"])
    assert a.edit_photo == "p.exr" and a.edit_transfer == "ratio"
    assert not render_final.parse_args(PATH).edit_composite
    base = ["--save_name", "case"]
    refused = {
        "without --integrator path": base + ["--mode", "real", "--edit_roughness", "0.2", "--edit_composite"],
        "with --integrator sh": base + ["--mode", "real", "--integrator", "sh", "--edit_roughness", "0.2", "--edit_composite"],
        "without any --edit_*": base + ["--mode", "real", "--integrator", "path", "--edit_composite"],
        "with --mode oi": base + ["--mode", "oi", "--integrator", "path", "--edit_roughness", "0.2", "--edit_composite"],
        "with --mode rolling": base + ["--mode", "rolling", "--integrator", "path", "--edit_roughness", "0.2", "--edit_composite"],
        "with --denoise atrous": PATH + ["--edit_composite", "--denoise", "atrous", "--spp", "4"],
        "with --env_scale 2": PATH + ["--edit_composite", "--env_scale", "2"],
        "--edit_photo alone": PATH + ["--edit_photo", "p.exr"],
        "--edit_transfer alone": PATH + ["--edit_transfer", "ratio"],
        "--edit_transfer additive alone": PATH + ["--edit_transfer", "additive"],
        "an unknown transfer": PATH + ["--edit_composite", "--edit_transfer", "sharp"],
    }
    for what, argv in refused.items():
        with pytest.raises(SystemExit):
            render_final.parse_args(argv)
            pytest.fail(what)
    for edit in (["--edit_albedo", "0.1", "0", "0"], ["--edit_metallic", "1"]):           # every kind of edit is one
        assert render_final.parse_args(base + ["--mode", "real", "--integrator", "path", "--edit_composite"] + edit).edit_composite


def test_render_real_refuses_before_any_work(path_lib, tmp_path):
    """`render_real(composite=True)` raises ValueError for what the command line refuses, and for a missing photograph, before the scene
    is read or a device touched (there is neither here)."""
    from materialist_amd import relight

    kw = dict(input_path=str(tmp_path), save_path=str(tmp_path), device="nowhere")
    edit = {"albedo": None, "roughness": 0.2, "metallic": None}
    ok = dict(integrator="path", edit=edit, composite=True)
    with pytest.raises(ValueError, match="composite needs integrator='path'"):
        relight.render_real("nothing", **{**ok, "integrator": "sh"}, **kw)
    for none in (None, {}, {"albedo": None, "roughness": None, "metallic": None}):
        with pytest.raises(ValueError, match="composite needs an edit"):
            relight.render_real("nothing", **{**ok, "edit": none}, **kw)
    with pytest.raises(ValueError, match="composite knows no denoise='atrous'"):
        relight.render_real("nothing", denoise="atrous", spp=4, **ok, **kw)
    with pytest.raises(ValueError, match="composite needs env_scale 1"):
        relight.render_real("nothing", env_scale=2.0, **ok, **kw)
    with pytest.raises(ValueError, match="transfer must be 'additive' or 'ratio', got 'sharp'"):
        relight.render_real("nothing", transfer="sharp", **ok, **kw)
    with pytest.raises(ValueError, match="photo_path and transfer need composite=True"):
        relight.render_real("nothing", integrator="path", edit=edit, transfer="ratio", **kw)
    with pytest.raises(ValueError, match="photo_path and transfer need composite=True"):
        relight.render_real("nothing", integrator="path", edit=edit, photo_path="p.exr", **kw)
    with pytest.raises(ValueError, match="composite needs the photograph: .*gt_image.exr does not exist"):
        relight.render_real("nothing", **ok, **kw)
    with pytest.raises(ValueError, match="composite needs the photograph: .*no_such.exr does not exist"):
        relight.render_real("nothing", photo_path=os.path.join(str(tmp_path), "no_such.exr"), **ok, **kw)
    with pytest.raises(ValueError, match="No envmap found"):                # without `composite` it goes on to look for the scene
        relight.render_real("nothing", integrator="path", edit=edit, **kw)
