"""The differential render's denoiser on the GPU ("Denoiser for the differential render"): the prepare, level and
finish kernels against fp64 at every pixel, the properties that follow from the definition, bits (the chain against its steps, run to
run), the gain on the synthetic differential image, and end to end: two `render_diff` halves of a small scene through
`PathTracer.denoise_diff`, and `render_final.py --mode oi --oi_composite --oi_composite_denoise`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import diff_denoise_fp64 as dd  # noqa: E402
import path_diff_fp64 as pd  # noqa: E402
import path_objects_fp64 as pob  # noqa: E402
import path_testlib as tl  # noqa: E402
import path_texture_fp64 as px  # noqa: E402

pytestmark = pytest.mark.gpu

_report = tl.reporter("diff denoise", "test_gpu_diff_denoise")
_u32 = dd.u32


@pytest.fixture(scope="module")
def pt():
    return tl.load(gpu=True)


def _np(fn):
    """A device entry of `pathtrace` as a function from and to numpy arrays."""
    def run(*args, **kw):
        out = fn(*args, **kw)
        return tuple(t.cpu().numpy() for t in out) if isinstance(out, tuple) else out.cpu().numpy()

    return run


# ---- 1: every step against fp64 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", dd.SCALES, ids=["scale1", "scale1/3"])
@pytest.mark.parametrize("H,W", dd.SHAPES)
def test_every_step_matches_fp64(pt, H, W, scale):
    """The CPU test's fields, shapes and bounds at every pixel.  Measured (MI355X): see DESIGN.md section 1.4."""
    x = dd.diff_inputs(H, W, scale)
    dd.check_field(x)
    dd.check_steps_against_fp64(x, _np(pt.denoise_diff_prepare), _np(pt.denoise_diff_level), _np(pt.denoise_diff_finish), _np(pt.denoise_diff),
                                f"device {H}x{W} scale {scale:.3f}", _report)


# ---- 2: what follows from the definition -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", dd.SHAPES)
def test_the_reduction_to_the_plain_denoiser(pt, H, W):
    """Alphas 0, ids <= 0, scale 1, delta >= 0: delta' against `denoise` of the two delta halves, within 1e-4 of the largest mean; whether
    the bits agree is reported (the two kernels are separate instantiations, and the compiler may contract them differently)."""
    x = dd.reduction_inputs(H, W)
    fg, delta, alpha = _np(pt.denoise_diff)(x["A"], x["B"], x["alb"], x["geom"], 1.0)
    ref = pt.denoise(x["A"][1], x["B"][1], x["alb"], x["geom"]).cpu().numpy()
    worst = float(np.abs(delta.astype(np.float64) - ref).max()) / float(np.abs(0.5 * (x["A"][1] + x["B"][1])).max())
    _report(f"device {H}x{W} reduction to matpbr_path_denoise: worst error relative to the largest mean; bit for bit",
            (worst, bool(np.array_equal(_u32(delta), _u32(ref)))))
    assert worst <= 1e-4 and not _u32(fg).any() and not _u32(alpha).any()


def test_sign_symmetry_scaling_and_pass_through(pt):
    x = dd.diff_inputs(36, 20, 1.0 / 3)
    dd.check_sign_symmetry(x, _np(pt.denoise_diff))
    for k in (3, -2):
        dd.check_scaling(x, _np(pt.denoise_diff), k)
    dd.check_pass_through(x, _np(pt.denoise_diff))
    dd.check_pass_through(dd.diff_inputs(17, 9, 1.0), _np(pt.denoise_diff))


def test_zero_reach_keeps_the_photograph(pt):
    dd.check_zero_reach(_np(pt.denoise_diff), _np(pt.composite), _report, "device")


def test_own_over_kappa_is_a_convex_combination_within_its_id(pt):
    dd.check_convexity(dd.diff_inputs(36, 20, 1.0 / 3), _np(pt.denoise_diff), _report, "device 36x20")


# ---- 3: bits ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(17, 9), (40, 72)])
def test_the_chain_equals_its_steps_bit_for_bit(pt, H, W):
    x = dd.diff_inputs(H, W, 1.0 / 3)
    dev = lambda t: tuple(torch.from_numpy(a).cuda() for a in t)
    A, B = dev(x["A"]), dev(x["B"])
    geom, alb = torch.from_numpy(x["geom"]).cuda(), torch.from_numpy(x["alb"]).cuda()
    for levels in (1, 2, 5):
        one = pt.denoise_diff(A, B, alb, geom, x["scale"], levels=levels)
        cv, cov = pt.denoise_diff_prepare(A, B, geom, x["scale"])
        for l in range(levels):
            cv = pt.denoise_diff_level(cv, cov, geom, alb, l, levels=levels)
        steps = pt.denoise_diff_finish(cv, cov, A, B, geom, x["scale"])
        again = pt.denoise_diff(A, B, alb, geom, x["scale"], levels=levels)
        for a, b, c in zip(one, steps, again):
            assert np.array_equal(tl.bits(a), tl.bits(b)) and np.array_equal(tl.bits(a), tl.bits(c)), levels


# ---- 4: the gain ------------------------------------------------------------------------------------------------------------------------------
def test_the_denoised_composite_is_closer_to_the_truth(pt):
    dd.check_gain(_np(pt.denoise_diff), _report, "device")


# ---- 5: end to end ----------------------------------------------------------------------------------------------------------------------------
def test_two_render_diff_halves_through_the_filter(pt):
    """The groove at 24 x 20 under `path_texture_fp64.table_scene()`, two `render_diff` halves at spp 8: `PathTracer.denoise_diff` against
    the restatement fed the device's own sums, to the steps' criterion; and with one level, every pixel whose closed R = 3 neighbourhood
    is all zero in both halves keeps the photograph's bits.  On this scene that set is empty (measured at max_depth 2, 3, 4, 6 and 16:
    between 221 and 281 of the 480 pixels are non-zero in a half, scattered, and no 7 x 7 window is free of them), so the test asserts
    the larger set the definition also holds: fg and alpha zero at the pixel itself and delta zero within the level's own reach, 2 pixels.
    It contains the first, is not empty (the count is asserted), and each of its pixels keeps the photograph's bits."""
    s = tl.groove_with_objects(pt, px.table_scene(), pob.merged)
    tracer, maps = s["tracer"], (s["a"], s["r"], s["m"], s["env"])
    A, B = (tracer.render_diff(*maps, spp=8, max_depth=6, seed=seed)[:3] for seed in (0, 1))
    geom = tracer.features()
    from materialist_amd.relight import albedo_guide

    guide = albedo_guide(geom, torch.from_numpy(s["a"]).cuda(), [ob["bsdf"] for ob in s["objects"]], tracer.feature_tints())
    An, Bn = (tuple(t.cpu().numpy() for t in T) for T in (A, B))
    g, al = geom.cpu().numpy(), guide.cpu().numpy()
    got = [t.cpu().numpy() for t in tracer.denoise_diff(A, B, guide, geom, 1.0)]
    ref = dd.chain(An, Bn, g, al, 1.0)
    c_in = float(np.abs(dd.prepare(An, Bn, g, 1.0)[0][..., :3]).max())
    worst = max(float(np.abs(x.astype(np.float64) - r).max()) for x, r in zip(got, ref)) / c_in
    _report("groove + table 24x20, halves at spp 8: denoise_diff against the restatement, worst error relative to the largest c0", worst)
    assert worst <= 1e-4 and all(np.isfinite(x).all() for x in got)
    assert (g[..., 7] >= 1).any() and (An[1] < 0).any() and (An[1] > 0).any()
    # one level: R = 3.  `loose`: all three outputs zero within R.  `tight` holds it: fg and alpha zero at the pixel, delta zero within the
    # level's own reach 2 (2^L - 1) = 2 (the variance prefilter's extra tap enters the weights alone, and a weight times +0 is +0)
    busy, touched = np.zeros(g.shape[:2], bool), np.zeros(g.shape[:2], bool)
    for T in (An, Bn):
        busy |= (T[0] != 0).any(-1) | (T[2] != 0)
        touched |= (T[1] != 0).any(-1)
    loose = dd.chebyshev_to(busy | touched) > dd.reach(1)
    tight = ~busy & (dd.chebyshev_to(touched) > dd.reach(1) - 1)
    photo = np.random.default_rng(6).gamma(2.0, 0.5, g.shape[:2] + (3,)).astype(np.float32)
    out = pt.composite(*tracer.denoise_diff(A, B, guide, geom, 1.0, levels=1), photo, 1.0).cpu().numpy()
    kept = (_u32(out) == _u32(photo)).all(-1)
    _report("groove + table 24x20, L = 1: pixels all zero within R = 3; pixels with fg = alpha = 0 and delta zero within 2; pixels that keep the "
            "photograph's bits", (int(loose.sum()), int(tight.sum()), int(kept.sum())))
    assert not (loose & ~tight).any() and tight.sum() > 0 and int((kept & tight).sum()) == int(tight.sum())


def test_render_final_cli_composite_denoise(pt, tmp_path):
    """`render_final.py --mode oi --oi_composite --oi_composite_denoise` on a synthetic output at 32 x 32: it writes mi_oic_*, its EXR
    differs from the run without the flag and is the same from run to run."""
    from materialist_amd import mesh
    from materialist_amd.imageio_exr import read_exr, write_exr

    tmp = str(tmp_path)
    scene_dir = tl.synthetic_output(tmp)
    write_exr(os.path.join(scene_dir, "gt_image.exr"), np.random.default_rng(4).gamma(2.0, 0.3, (32, 32, 3)).astype(np.float32))
    ob = pd.cube_object(pd.VISIBLE_CUBE)
    mesh.write_ply(os.path.join(scene_dir, "oi2.ply"), ob["vertices"].astype(np.float32), ob["triangles"])
    cmd = [sys.executable, os.path.join(ROOT, "render_final.py"), "--save_name", "case", "--input_path", tmp, "--save_path", tmp, "--mode", "oi",
           "--spp", "4", "--oi_iters", "2", "--oi_composite"]
    exr, png = (os.path.join(tmp, "case", "mi_oic_case_envmap" + ext) for ext in (".exr", ".png"))

    def run(*extra):
        for p in (exr, png):
            if os.path.exists(p):
                os.remove(p)
        res = subprocess.run(cmd + list(extra), capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout + res.stderr
        assert os.path.exists(png) and not os.path.exists(os.path.join(tmp, "case", "mi_oi_case_envmap.exr"))
        return np.ascontiguousarray(read_exr(exr)[..., :3], dtype=np.float32)

    plain = run()
    one, two = run("--oi_composite_denoise"), run("--oi_composite_denoise")
    assert np.isfinite(one).all() and (one >= 0).all()
    assert np.array_equal(_u32(one), _u32(two)) and not np.array_equal(_u32(one), _u32(plain))
