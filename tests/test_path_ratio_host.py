"""Ratio shadow transfer on the CPU ("Ratio shadow transfer"; no GPU): `matpbr_path_composite_ratio_host` against
the same expression in numpy float32 with every case of it built in, what each kind of channel carries, the invariance under the
model's scale that the feature exists for, the header against the binding, the refusals of the three entries, of
`render_oi(shadows=...)` and of the command line before any work, and the fp64 experiment that shows the benefit: composited from maps
whose albedo is half the true one, the ratio's shadows lie closer to the truth than the additive ones."""
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

import path_diff_fp64 as pd  # noqa: E402
import path_ratio_fp64 as prf  # noqa: E402
import path_testlib as tl  # noqa: E402

H, W = prf.H, prf.W
_report = tl.reporter("path ratio host", "test_path_ratio_host")
_u32 = lambda x: np.ascontiguousarray(x).view(np.uint32)


@pytest.fixture(scope="module")
def path_lib():
    return tl.load()


# ---- 0 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_what_the_binding_binds(path_lib):
    with open(os.path.join(ROOT, "include", "matpbr_path.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(matpbr_path_\w+)\s*\(", text))
    names = path_lib.RATIO_SYMBOLS
    assert names == ("matpbr_path_render_objects_ratio", "matpbr_path_composite_ratio", "matpbr_path_composite_ratio_host")
    assert set(names) <= declared and not set(names) & set(path_lib.LATE_SYMBOLS)
    lib = path_lib.load()
    for name in names:
        fn = path_lib.symbol(name, lib)
        assert fn.argtypes == path_lib.SIGNATURES[name][1] and fn.restype == path_lib.SIGNATURES[name][0], name
    P, sig = ctypes.c_void_p, path_lib.SIGNATURES
    assert sig[names[0]][1] == sig["matpbr_path_render_objects_through"][1] + [P]
    assert sig[names[1]][1] == sig[names[2]][1] + [P]
    host = sig["matpbr_path_composite_host"][1]
    assert sig[names[2]][1] == host[:2] + [P] + host[2:]
    assert lib.matpbr_path_version() == path_lib.VERSION == 3
    for name in ("pathtrace", "path_filters"):   # re-exported like their neighbours
        mod = __import__("materialist_amd." + name, fromlist=[name])
        assert callable(mod.composite_ratio) and callable(mod.composite_ratio_host)

    class Old:
        pass

    for name in names:   # a library from before the feature: PathError through symbol(), naming the entry and the feature
        with pytest.raises(path_lib.PathError, match=name + ".*ratio shadow transfer"):
            path_lib.symbol(name, Old())


# ---- C1, C2 ----------------------------------------------------------------------------------------------------------------------------
ROWS = {"delta = 0": 0, "delta > 0": 1, "base = 0": 2, "base + delta slightly negative": 3, "all zero": 4, "alpha = 1": 5, "a base that underflows": 6}


def _sums(rng, frames):
    """Random sums of `frames` frames at 24 x 20: delta < 0 < base nearly everywhere, and one row per case of ROWS."""
    f32 = np.float32
    alpha = rng.uniform(0, frames, (H, W)).astype(f32)
    alpha.reshape(-1)[::5] = 0.0
    fg = (rng.gamma(2.0, 0.5, (H, W, 3)) * alpha[..., None]).astype(f32)
    base = (rng.gamma(2.0, 0.5, (H, W, 3)) * frames).astype(f32)
    delta = (-base * rng.uniform(0.0, 1.0, (H, W, 3))).astype(f32)
    photo = rng.gamma(2.0, 0.5, (H, W, 3)).astype(f32)
    delta[ROWS["delta = 0"]] = 0.0
    delta[ROWS["delta > 0"]] = rng.uniform(0.01, 1.0, (W, 3)).astype(f32)
    base[ROWS["base = 0"]] = 0.0                                           # a dark model: half of the row darkens, half brightens
    delta[ROWS["base = 0"], W // 2:] = 0.25
    r = ROWS["base + delta slightly negative"]
    delta[r] = np.nextafter(-base[r], f32(-np.inf))
    r = ROWS["all zero"]
    fg[r], delta[r], base[r], alpha[r] = 0.0, 0.0, 0.0, 0.0
    alpha[ROWS["alpha = 1"]] = frames
    r = ROWS["a base that underflows"]                                      # base scale = 0 for frames > 1: 0 / 0, and fmaxf drops the NaN
    base[r], delta[r] = f32(1e-45), f32(-1e-45)
    return fg, delta, base, alpha, photo


@pytest.mark.parametrize("frames", [1, 3, 10])
def test_composite_ratio_host_is_the_expression_in_float32(path_lib, frames):
    """C1 and C2: bit for bit against the numpy transcription; an additive channel carries `matpbr_path_composite_host`'s bits; a ratio
    channel lies in [0, max(0, fg scale + K photo)]; an all-zero pixel returns the photograph's bits."""
    fg, delta, base, alpha, photo = _sums(np.random.default_rng(40 + frames), frames)
    scale = 1.0 / frames
    got = path_lib.composite_ratio_host(fg, delta, base, alpha, photo, scale)
    ref, ratio = prf.composite_ratio_f32(fg, delta, base, alpha, photo, scale)
    assert got.dtype == np.float32 and got.shape == (H, W, 3) and np.isfinite(got).all()
    assert np.array_equal(_u32(got), _u32(ref))
    # the cases are there
    assert 0.5 < ratio.mean() < 0.9
    assert not ratio[ROWS["delta = 0"]].any() and not ratio[ROWS["delta > 0"]].any() and not ratio[ROWS["base = 0"]].any()
    assert (delta[ROWS["base = 0"]] < 0).any() and (delta[ROWS["base = 0"]] > 0).any()
    r = ROWS["base + delta slightly negative"]
    assert ratio[r].all() and (base[r].astype(np.float64) + delta[r] < 0).all()
    assert np.array_equal(got[r], np.maximum(np.float32(0), fg[r] * np.float32(scale)))     # g = 0: the photograph is gone, fg stays
    assert np.array_equal(_u32(got[ROWS["all zero"]]), _u32(photo[ROWS["all zero"]]))
    assert (alpha[ROWS["alpha = 1"]] * np.float32(scale) == 1).all()
    assert ratio[ROWS["a base that underflows"]].all()
    # C2
    additive = path_lib.composite_host(fg, delta, alpha, photo, scale)
    assert np.array_equal(_u32(got)[~ratio], _u32(additive)[~ratio])
    assert (_u32(got)[ratio] != _u32(additive)[ratio]).mean() > 0.9
    sc = np.float32(scale)
    bound = np.maximum(np.float32(0), fg * sc + (np.float32(1) - alpha[..., None] * sc) * photo)
    assert (got[ratio] >= 0).all() and (got[ratio] <= bound[ratio]).all()


def test_the_ratio_does_not_see_the_models_scale(path_lib):
    """C3: delta and base times 0.5 (exact in fp32; a model half as bright): the ratio channels keep their bits, every additive channel
    with delta != 0 changes them.  (Shadows shallower than the photograph is bright, so no additive channel is clamped to 0 twice.)"""
    rng = np.random.default_rng(7)
    f32 = np.float32
    for frames in (1, 4):
        alpha = (rng.uniform(0, 0.5, (H, W)) * frames).astype(f32)
        fg = (rng.gamma(2.0, 0.5, (H, W, 3)) * alpha[..., None]).astype(f32)
        photo = rng.uniform(0.5, 2.0, (H, W, 3)).astype(f32)
        base = (rng.uniform(0.5, 2.0, (H, W, 3)) * frames).astype(f32)
        delta = (rng.uniform(-0.2, 0.2, (H, W, 3)) * frames).astype(f32)
        delta[0] = 0.0
        base[1] = 0.0
        one = path_lib.composite_ratio_host(fg, delta, base, alpha, photo, 1.0 / frames)
        half = path_lib.composite_ratio_host(fg, delta * f32(0.5), base * f32(0.5), alpha, photo, 1.0 / frames)
        ratio = (delta < 0) & (base > 0)
        moved = ~ratio & (delta != 0)
        assert ratio.mean() > 0.3 and moved.mean() > 0.3 and (~ratio & (delta < 0)).any()
        assert np.array_equal(_u32(one)[ratio], _u32(half)[ratio])
        assert (_u32(one)[moved] != _u32(half)[moved]).all()
        assert np.array_equal(_u32(one)[delta == 0], _u32(half)[delta == 0])


# ---- C4 --------------------------------------------------------------------------------------------------------------------------------
def test_composite_ratio_refusals(path_lib):
    z3, z1 = np.zeros((3, 4, 3), np.float32), np.zeros((3, 4), np.float32)
    for fn in (path_lib.composite_ratio_host, path_lib.composite_ratio):   # the same words on both sides, before a device is touched
        for scale in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError, match="scale must be finite and positive"):
                fn(z3, z3, z3, z1, z3, scale)
        with pytest.raises(ValueError, match=r"alpha must be \[3, 4\]"):
            fn(z3, z3, z3, z3, z3)
        with pytest.raises(ValueError, match=r"base must be \[3, 4, 3\], got \[3, 4\]"):
            fn(z3, z3, z1, z1, z3)
        with pytest.raises(ValueError, match="base must be"):
            fn(z3, z3, None, z1, z3)
        with pytest.raises(ValueError, match=r"photo must be \[H,W,3\]"):
            fn(z3, z3, z3, z1, z1)
    out = np.empty((3, 4, 3), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    host, dev = path_lib.symbol("matpbr_path_composite_ratio_host"), path_lib.symbol("matpbr_path_composite_ratio")
    args = [p(z3), p(z3), p(z3), p(z1), p(z3), 3, 4, 1.0, p(out)]
    assert host(*args) == 0
    cases = [(0, None), (1, None), (2, None), (3, None), (4, None), (5, 0), (6, -2), (7, 0.0), (7, -0.5), (7, float("inf")), (7, float("nan")), (8, None)]
    for j, bad in cases:
        spoiled = [bad if i == j else x for i, x in enumerate(args)]
        assert host(*spoiled) == -1, (j, bad)
        assert dev(*spoiled, None) == -1, (j, bad)   # refused before it launches anything


def test_render_objects_ratio_refusals(path_lib):
    """Every pointer a non-null dummy that a refusing call never reads, a valid one-object table: a call invalid in one respect returns
    MATPBR_PATH_ERR_INVALID_ARG (the call these start from is accepted on the GPU: test_gpu_path_ratio.py's raw call)."""
    raw = np.zeros(18, np.float64)
    ptr = raw[(-raw.ctypes.data % 16) // 8:][:16].ctypes.data
    table = (path_lib.PathObject * 1)(path_lib.PathObject(path_lib.BSDF_DIFFUSE, 1, 20, (ctypes.c_float * 3)(0.5, 0.5, 0.5)))
    frame = [ptr] * 5 + [4, 6, 35.0] + [ptr] * 4 + [2, 4, 3, 4, 0, 2]
    objects = [ctypes.cast(table, ctypes.c_void_p), 1, None, 1, None, None, None, None, None, None, None, None, 0]
    outs = {"fg": ptr, "delta": ptr, "alpha": ptr, "rewalked": None, "photo": ptr, "through": ptr, "base": ptr}
    fn = path_lib.symbol("matpbr_path_render_objects_ratio")
    assert len(frame) + 2 + len(objects) + len(outs) == len(path_lib.SIGNATURES["matpbr_path_render_objects_ratio"][1])
    call = lambda objs=objects, **spoil: fn(*frame, None, None, *objs, *{**outs, **spoil}.values())
    for name in ("fg", "delta", "alpha", "base"):
        assert call(**{name: None}) == -1, name
    assert call(photo=None) == -1 and call(through=None) == -1            # exactly one of the two
    assert call(photo=None, through=None, base=None) == -1
    assert call([None, 0] + objects[2:]) == -1                              # no objects
    assert call(objects[:3] + [2] + objects[4:]) == -1                      # the table's own check: a range starting below n_scene_tri
    assert fn(*frame[:14], 0, *frame[15:], None, None, *objects, *outs.values()) == -1   # the frame's own check: spp = 0


def test_shadows_is_refused_before_any_work(path_lib, tmp_path):
    """`render_oi(shadows="ratio")` without `composite`, and an unknown value with it, raise before the scene is even looked for (there
    is none here); the command line refuses `--oi_shadows ratio` without `--oi_composite` and an unknown value while it parses."""
    from materialist_amd import relight

    kw = dict(input_path=str(tmp_path), save_path=str(tmp_path), device="nowhere")
    with pytest.raises(ValueError, match="shadows='ratio' needs composite=True"):
        relight.render_oi("nothing", shadows="ratio", **kw)
    for composite in (False, True):
        with pytest.raises(ValueError, match="shadows must be 'additive' or 'ratio', got 'sharp'"):
            relight.render_oi("nothing", shadows="sharp", composite=composite, **kw)
    with pytest.raises(FileNotFoundError):                                  # the default goes on to look for the objects
        relight.render_oi("nothing", **kw)
    import render_final

    base = ["--save_name", "case", "--mode", "oi"]
    assert render_final.parse_args(base).oi_shadows == "additive"
    assert render_final.parse_args(base + ["--oi_composite"]).oi_shadows == "additive"
    a = render_final.parse_args(base + ["--oi_composite", "--oi_shadows", "ratio", "--oi_see_through", "--oi_composite_denoise"])
    assert a.oi_shadows == "ratio" and a.oi_composite
    for extra in (["--oi_shadows", "ratio"], ["--oi_composite", "--oi_shadows", "sharp"], ["--oi_shadows", "sharp"]):
        with pytest.raises(SystemExit):
            render_final.parse_args(base + extra)
    assert render_final.parse_args(base + ["--oi_shadows", "additive"]).oi_shadows == "additive"


# ---- C5 --------------------------------------------------------------------------------------------------------------------------------
def test_the_reference_alone_shows_the_benefit(path_lib, oracle64):
    """The groove with the visible diffuse cube, max_depth 2, seeds 0 and 1 x 8 samples, all in fp64 (`path_ratio_fp64.experiment`): the
    photograph and the truth from the true maps, both composites from maps whose albedo is half the true one.  Over the shadow pixels
    the ratio composite's mean absolute error is below the additive one's.  Recorded: 12 shadow pixels, additive 9.57e-3, ratio 2.59e-4
    (the truth's mean there is 0.304, the shadow's depth 1.95e-2: the additive shadow is half as deep as it should be, the ratio's is
    right but for the specular term, which does not scale with the albedo, and the samples' noise)."""
    s = prf.groove_scene([pd.cube_object(pd.VISIBLE_CUBE)], path_lib.env_tables)
    m = prf.experiment(oracle64, s, 2, (0, 1), 8)
    additive, ratio = prf.shadow_errors(m)
    _report("fitted albedo 0.5 x true, max_depth 2, 16 samples: shadow pixels; mean |additive - truth|; mean |ratio - truth|; the shadow's mean depth",
            f"{m['shadow'].size}; {additive:.3e}; {ratio:.3e}; {float((m['photo'] - m['truth']).mean()):.3e}")
    assert m["shadow"].size >= 8
    assert (m["delta"] < 0).all() and (m["base"] > 0).all()               # every channel there takes the ratio branch
    assert ratio < additive
