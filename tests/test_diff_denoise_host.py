"""Host side of the differential render's denoiser ("Denoiser for the differential render"): the per-pixel
routines the kernels run (on the CPU) against the fp64 restatement at every pixel, the properties that follow from the definition, bits,
the refusals of the ABI, of `relight.render_oi` and of the command line, and the gain on a synthetic differential image.  No GPU needed."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import diff_denoise_fp64 as dd  # noqa: E402
import path_diff_fp64 as pd  # noqa: E402
import path_testlib as tl  # noqa: E402


@pytest.fixture(scope="module")
def path_lib():
    return tl.load()


_report = tl.reporter("diff denoise", "test_diff_denoise_host")
_u32 = dd.u32


# ---- 1: every step against fp64 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", dd.SCALES, ids=["scale1", "scale1/3"])
@pytest.mark.parametrize("H,W", dd.SHAPES)
def test_every_step_matches_fp64(path_lib, H, W, scale):
    """Measured worst case over the three shapes and both scales with the CPU twins: see DESIGN.md section 1.4."""
    x = dd.diff_inputs(H, W, scale)
    obj, abar, kappa = dd.check_field(x)
    if (H, W) == (40, 72):
        assert (~obj & (abar > 0) & (kappa == 0)).any()                 # a scene pixel wholly covered
    dd.check_steps_against_fp64(x, path_lib.denoise_diff_prepare_host, path_lib.denoise_diff_level_host, path_lib.denoise_diff_finish_host,
                             path_lib.denoise_diff_host, f"{H}x{W} scale {scale:.3f}", _report)


# ---- 2: what follows from the definition -------------------------------------------------------------------------------------------------------
def _plain_chain_host(path_lib, A, B, geom, alb, levels=5):
    cv = path_lib.denoise_prepare_host(A, B, geom)
    for l in range(levels):
        cv = path_lib.denoise_level_host(cv, geom, alb, l, levels=levels)
    return cv[..., :3]


@pytest.mark.parametrize("H,W", dd.SHAPES)
def test_the_reduction_to_the_plain_denoiser_is_bit_for_bit(path_lib, H, W):
    """Alphas 0, ids <= 0, scale 1, delta >= 0: delta' has the bits of the plain filter of the two delta halves."""
    x = dd.reduction_inputs(H, W)
    assert set(np.unique(x["geom"][..., 7])) == {-1.0, 0.0} and (x["A"][1] >= 0).all()
    for levels in (1, 5):
        fg, delta, alpha = path_lib.denoise_diff_host(x["A"], x["B"], x["alb"], x["geom"], 1.0, levels=levels)
        ref = _plain_chain_host(path_lib, x["A"][1], x["B"][1], x["geom"], x["alb"], levels)
        assert np.array_equal(_u32(delta), _u32(ref)), levels
        assert not _u32(fg).any() and not _u32(alpha).any()


def test_sign_symmetry_scaling_and_pass_through(path_lib):
    x = dd.diff_inputs(36, 20, 1.0 / 3)
    dd.check_sign_symmetry(x, path_lib.denoise_diff_host)
    for k in (3, -2):
        dd.check_scaling(x, path_lib.denoise_diff_host, k)
    dd.check_pass_through(x, path_lib.denoise_diff_host)
    dd.check_pass_through(dd.diff_inputs(17, 9, 1.0), path_lib.denoise_diff_host)


def test_zero_reach_keeps_the_photograph(path_lib):
    dd.check_zero_reach(path_lib.denoise_diff_host, path_lib.composite_host, _report, "host")


def test_own_over_kappa_is_a_convex_combination_within_its_id(path_lib):
    dd.check_convexity(dd.diff_inputs(36, 20, 1.0 / 3), path_lib.denoise_diff_host, _report, "host 36x20")


# ---- 3: bits ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(17, 9), (40, 72)])
def test_the_chain_equals_its_steps_bit_for_bit(path_lib, H, W):
    x = dd.diff_inputs(H, W, 1.0 / 3)
    for levels in (1, 2, 5):
        one = path_lib.denoise_diff_host(x["A"], x["B"], x["alb"], x["geom"], x["scale"], levels=levels)
        cv, cov = path_lib.denoise_diff_prepare_host(x["A"], x["B"], x["geom"], x["scale"])
        for l in range(levels):
            cv = path_lib.denoise_diff_level_host(cv, cov, x["geom"], x["alb"], l, levels=levels)
        steps = path_lib.denoise_diff_finish_host(cv, cov, x["A"], x["B"], x["geom"], x["scale"])
        again = path_lib.denoise_diff_host(x["A"], x["B"], x["alb"], x["geom"], x["scale"], levels=levels)
        for a, b, c in zip(one, steps, again):
            assert np.array_equal(_u32(a), _u32(b)) and np.array_equal(_u32(a), _u32(c)), levels


# ---- 4: refusals ------------------------------------------------------------------------------------------------------------------------------
def test_the_abi_refuses_bad_arguments(path_lib):
    lib = path_lib.load()
    H, W = 17, 9
    x = dd.diff_inputs(H, W, 1.0)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    good = path_lib.PathDenoise(5, 32.0, 1.0, 0.1, 4.0)
    prm = lambda p: ctypes.cast(ctypes.byref(p), ctypes.c_void_p)
    halves = [ptr(t) for t in (*x["A"], *x["B"])]
    cv, cv2, cov = np.zeros((H, W, 4), np.float32), np.zeros((H, W, 4), np.float32), np.ones((H, W), np.float32)
    fg, delta, alpha = np.empty((H, W, 3), np.float32), np.empty((H, W, 3), np.float32), np.empty((H, W), np.float32)
    nbytes = lib.matpbr_path_denoise_diff_workspace_bytes(H, W)
    assert nbytes == H * W * 36 and lib.matpbr_path_denoise_diff_workspace_bytes(0, W) == 0
    ws = np.empty(nbytes // 4, np.float32)
    bad_scales = (0.0, -1.0, float("inf"), float("nan"))
    bad_prms = [path_lib.PathDenoise(0, 32.0, 1.0, 0.1, 4.0), path_lib.PathDenoise(9, 32.0, 1.0, 0.1, 4.0),
                path_lib.PathDenoise(5, 32.0, 1.0, 0.0, 4.0), path_lib.PathDenoise(5, float("nan"), 1.0, 0.1, 4.0)]

    def refused(fn, args, spoil, tail=()):
        assert fn(*args, *tail) == 0
        for k, values in spoil.items():
            for v in values:
                assert fn(*(v if i == k else a for i, a in enumerate(args)), *tail) == -1, (fn.__name__, k, v)

    prep = [*halves, ptr(x["geom"]), H, W, 1.0, ptr(cv), ptr(cov)]
    spoil_prep = {**{k: [None] for k in (0, 1, 2, 3, 4, 5, 6, 10, 11)}, 7: [0, -1], 8: [0], 9: bad_scales}
    refused(lib.matpbr_path_denoise_diff_prepare_host, prep, spoil_prep)
    lev = [ptr(cv), ptr(cov), ptr(x["geom"]), ptr(x["alb"]), H, W, prm(good), 0, ptr(cv2)]
    spoil_lev = {**{k: [None] for k in (0, 1, 2, 3, 6, 8)}, 4: [0], 5: [-3], 6: [None] + [prm(p) for p in bad_prms], 7: [-1, 8], 8: [None, ptr(cv)]}
    refused(lib.matpbr_path_denoise_diff_level_host, lev, spoil_lev)
    fin = [ptr(cv), ptr(cov), *halves, ptr(x["geom"]), H, W, 1.0, ptr(fg), ptr(delta), ptr(alpha)]
    spoil_fin = {**{k: [None] for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 14)}, 9: [0], 10: [0], 11: bad_scales}
    refused(lib.matpbr_path_denoise_diff_finish_host, fin, spoil_fin)
    cha = [*halves, ptr(x["geom"]), ptr(x["alb"]), H, W, 1.0, prm(good), ptr(fg), ptr(delta), ptr(alpha), ptr(ws), nbytes]
    spoil_cha = {**{k: [None] for k in (0, 1, 2, 3, 4, 5, 6, 7, 12, 13, 14, 15)}, 8: [0], 9: [0], 10: bad_scales,
                 11: [None] + [prm(p) for p in bad_prms], 15: [None, ctypes.c_void_p(ws.ctypes.data + 4)], 16: [nbytes - 1, 0]}
    refused(lib.matpbr_path_denoise_diff_host, cha, spoil_cha)
    # the device entry points check the same before they launch anything: no GPU is touched by a refused call
    for fn, args, spoil in ((lib.matpbr_path_denoise_diff_prepare, prep, spoil_prep), (lib.matpbr_path_denoise_diff_level, lev, spoil_lev),
                            (lib.matpbr_path_denoise_diff_finish, fin, spoil_fin), (lib.matpbr_path_denoise_diff, cha, spoil_cha)):
        for k, values in spoil.items():
            for v in values:
                assert fn(*(v if i == k else a for i, a in enumerate(args)), None) == -1, (fn.__name__, k, v)


def test_the_python_wrappers_refuse_wrong_shapes_and_parameters(path_lib):
    x = dd.diff_inputs(17, 9, 1.0)
    A, B = x["A"], x["B"]
    with pytest.raises(ValueError, match=r"A\[1\] \(delta\) must be"):
        path_lib.denoise_diff_host((A[0], A[1][:-1], A[2]), B, x["alb"], x["geom"])
    with pytest.raises(ValueError, match=r"B\[2\] \(alpha\) must be"):
        path_lib.denoise_diff_prepare_host(A, (B[0], B[1], B[0]), x["geom"])
    with pytest.raises(ValueError, match="triples"):
        path_lib.denoise_diff_host(A[:2], B, x["alb"], x["geom"])
    with pytest.raises(ValueError, match="scale"):
        path_lib.denoise_diff_host(A, B, x["alb"], x["geom"], 0.0)
    with pytest.raises(ValueError, match="levels"):
        path_lib.denoise_diff_host(A, B, x["alb"], x["geom"], levels=9)
    with pytest.raises(ValueError, match="cov must be"):
        path_lib.denoise_diff_level_host(np.zeros((17, 9, 4), np.float32), np.zeros((17, 9, 1), np.float32), x["geom"], x["alb"], 0)
    with pytest.raises(ValueError, match="level"):
        path_lib.denoise_diff_level_host(np.zeros((17, 9, 4), np.float32), np.zeros((17, 9), np.float32), x["geom"], x["alb"], 8)


def test_an_older_library_names_the_missing_symbol(path_lib):
    class Older:                                                     # a loaded library without the new entry points
        pass

    assert len(path_lib.DIFF_DENOISE_SYMBOLS) == 9 and set(path_lib.DIFF_DENOISE_SYMBOLS) <= set(path_lib.LATE_SYMBOLS)
    for name in path_lib.DIFF_DENOISE_SYMBOLS:
        assert name in path_lib.SIGNATURES and hasattr(path_lib.load(), name)
        with pytest.raises(path_lib.PathError, match=name + ".*differential render's denoiser"):
            path_lib.symbol(name, Older())
    assert path_lib.load().matpbr_path_version() == path_lib.VERSION == 3


def test_render_oi_refuses_before_any_gpu_work(path_lib, tmp_path):
    """Every refusal is raised with device="nowhere": a call that reached the maps' upload or a tracer would fail on the device's name."""
    from materialist_amd import mesh, relight
    from materialist_amd.imageio_exr import write_exr

    tmp = str(tmp_path)
    scene = tl.synthetic_output(tmp)
    ob = pd.cube_object(pd.VISIBLE_CUBE)
    mesh.write_ply(os.path.join(scene, "oi2.ply"), ob["vertices"].astype(np.float32), ob["triangles"])
    write_exr(os.path.join(scene, "gt_image.exr"), np.random.default_rng(1).uniform(0, 1, (32, 32, 3)).astype(np.float32))
    kw = dict(input_path=tmp, save_path=tmp, n_iter=2, device="nowhere")
    with pytest.raises(ValueError, match="composite_denoise needs composite"):
        relight.render_oi("case", spp=4, composite_denoise=True, **kw)
    for spp in (5, 1, 0):
        with pytest.raises(ValueError, match="even"):
            relight.render_oi("case", spp=spp, composite=True, composite_denoise=True, **kw)
    with pytest.raises(ValueError, match="atrous"):                    # as before: the plain filter does not take the composite
        relight.render_oi("case", spp=4, composite=True, composite_denoise=True, denoise="atrous", **kw)
    with pytest.raises(ValueError, match="env_scale 1"):
        relight.render_oi("case", spp=4, composite=True, composite_denoise=True, env_scale=0.5, **kw)
    with pytest.raises(Exception) as e:                                # a good call goes on to the device's name
        relight.render_oi("case", spp=4, composite=True, composite_denoise=True, **kw)
    assert not isinstance(e.value, ValueError)


def test_the_command_line_parses_and_refuses():
    sys.path.insert(0, ROOT)
    import render_final

    base = ["--save_name", "case", "--mode", "oi"]
    assert render_final.parse_args(base + ["--oi_composite"]).oi_composite_denoise is False
    assert render_final.parse_args(base + ["--oi_composite", "--oi_composite_denoise", "--spp", "8"]).oi_composite_denoise is True
    for extra in (["--oi_composite_denoise"], ["--oi_composite", "--oi_composite_denoise", "--spp", "7"],
                  ["--oi_composite", "--oi_composite_denoise", "--denoise", "atrous"]):
        with pytest.raises(SystemExit):
            render_final.parse_args(base + extra)


# ---- 5: the gain ------------------------------------------------------------------------------------------------------------------------------
def test_the_denoised_composite_is_closer_to_the_truth(path_lib):
    dd.check_gain(path_lib.denoise_diff_host, _report, "host")
