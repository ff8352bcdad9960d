"""The differential render on the GPU (libmatpbr_path.so's `matpbr_path_render_objects_diff` and `matpbr_path_composite`, DESIGN.md
section 1.4, "Differential render"): every path of both walks against the fp64 restatement, exact zeros and the touch rule bracketed
from both sides, an object no path meets, the difference of the existing kernels' two renders, bits (launch splits, the raw call, the
composite's CPU twin, `render` untouched), and `render_final.py --mode oi --oi_composite`."""
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

import path_diff_fp64 as pd  # noqa: E402
import path_fp64 as pf  # noqa: E402
import path_objects_fp64 as pob  # noqa: E402
import path_rough_fp64 as pr  # noqa: E402
import path_testlib as tl  # noqa: E402
import path_texture_fp64 as px  # noqa: E402
from path_testlib import bits as _bits  # noqa: E402

pytestmark = pytest.mark.gpu

FOV = pf.FOV
_report = tl.reporter("path diff", "test_gpu_path_diff")


@pytest.fixture(scope="module")
def pt():
    return tl.load(gpu=True)


def _scene(pt, objects):
    s = tl.groove_with_objects(pt, objects, pob.merged)
    s["n_scene"] = s["rm"]["triangles"].shape[0]
    s["tab"] = pt.env_tables(s["env"])
    s["maps"] = (s["a"], s["r"], s["m"], s["env"])
    return s


@pytest.fixture(scope="module")
def tex_scene(pt):
    """The groove at 24 x 20 (a partial tile) with `path_texture_fp64.table_scene`: no light, all three flags."""
    s = _scene(pt, px.table_scene())
    assert s["tracer"].stats["n_lights"] == 0 and s["tracer"].stats["n_textured_objects"] == 3
    return s


@pytest.fixture(scope="module")
def rough_scene(pt):
    """The same groove with `path_rough_fp64.table_scene`: a light, rough and clear glass."""
    s = _scene(pt, pr.table_scene())
    assert s["tracer"].stats["n_lights"] == 1 and s["tracer"].stats["n_rough_objects"] >= 1
    return s


@pytest.fixture(scope="module")
def hidden_scene(pt):
    """The same groove with a diffuse cube of side 0.2 at (0, 0, -6), behind the depth mesh."""
    return _scene(pt, [pd.cube_object(pd.HIDDEN_CUBE)])


def _diff(s, spp, max_depth, seed, **kw):
    fg, delta, alpha, rewalked = s["tracer"].render_diff(*s["maps"], spp=spp, max_depth=max_depth, seed=seed, **kw)
    assert fg.shape == (s["H"], s["W"], 3) and delta.shape == fg.shape and alpha.shape == (s["H"], s["W"]) and rewalked.dtype == torch.int32
    return fg.cpu().numpy(), delta.cpu().numpy(), alpha.cpu().numpy(), rewalked.cpu().numpy()


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
def _parity_case(s, oracle64, name, max_depth, seed):
    fg, delta, alpha, rewalked = _diff(s, 1, max_depth, seed)
    assert np.isfinite(fg).all() and np.isfinite(delta).all()
    ref = pd.reference(oracle64, s, s["tab"], max_depth, seed)
    for what, got in (("fg", fg), ("delta", delta)):
        frac, err = pd.share_within(got.astype(np.float64), ref[what], ref["scale"], 1e-3)
        _report(f"{name} scene, max_depth {max_depth} seed {seed}: {what} against the two fp64 walks, share of pixels within 1e-3",
                f"{frac:.4f} ({int((err > 1e-3).sum())} pixels beyond, max err {err.max():.3e})")
        assert frac >= 0.98, (name, what, max_depth, seed, frac, np.argwhere(err > 1e-3)[:10])
    agree = float((alpha == ref["alpha"]).mean())
    _report(f"{name} scene, max_depth {max_depth} seed {seed}: alpha against the camera ray's brute-force coverage, share of pixels equal", f"{agree:.4f}")
    assert agree >= 0.98 and set(np.unique(alpha)) <= {0.0, 1.0}
    return ref, fg, delta, alpha, rewalked


@pytest.mark.parametrize("max_depth", [2, 6, 16])
def test_every_path_of_both_walks_matches_fp64_textures(pt, tex_scene, oracle64, max_depth):
    """spp 1, seeds 0-2: fg against c_ref L_with, delta against (1 - c_ref) (L_with - L_without), alpha against c_ref, the error of the
    worst channel relative to max(|L_with|, |L_without|, mean |L_with|): at least 0.98 of the pixels within 1e-3 (the project's 0.99 per
    walk, and there are two walks).  The reference has covered pixels, pixels whose walks differ and pixels whose walks agree."""
    for seed in (0, 1, 2):
        ref = _parity_case(tex_scene, oracle64, "texture", max_depth, seed)[0]
        differ = (ref["with"] != ref["without"]).any(-1)
        assert ref["c"].mean() > 0.1 and (differ & ~ref["c"]).any() and (~differ).mean() > 0.5


@pytest.mark.parametrize("max_depth", [6, 16])
def test_every_path_of_both_walks_matches_fp64_light_and_glass(pt, rough_scene, oracle64, max_depth):
    """The same on the table with a light (n_e differs between the walks, so every uncovered sample is walked twice), seeds 0, 1."""
    s = rough_scene
    for seed in (0, 1):
        ref, fg, delta, alpha, rewalked = _parity_case(s, oracle64, "rough", max_depth, seed)
        assert ((ref["with"] != ref["without"]).any(-1) & ~ref["c"]).mean() > 0.5


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_depth, seed", [(16, 0), (2, 1)])
def test_exact_zeros_and_the_touch_rule(pt, tex_scene, oracle64, max_depth, seed):
    """spp 1.  The reference first: between 0.2 and 0.3 of the pixels have fp64 walks that differ, and the loosest possible rule ("some
    ray of the sample meets an inserted triangle at any distance") flags about as many.  Then: (i) a pixel that was not walked twice has
    all-zero bits in delta; (ii) a pixel whose fp64 walks differ was walked twice, except at most 0.01 of the pixels -- or is covered
    (alpha = 1): there c_s = 1, the rule runs no second walk, and the difference of the walks is fg's, not delta's; (iii) a pixel
    walked twice lies inside the loosest rule's set, except at most 0.01 of the pixels: "walk everything twice" does not pass."""
    s = tex_scene
    ref = pd.reference(oracle64, s, s["tab"], max_depth, seed)
    differ = (ref["with"] != ref["without"]).any(-1)
    loosest = pd.meets_object_anywhere(oracle64, s, s["tab"], max_depth, seed)
    _report(f"max_depth {max_depth} seed {seed}: share of pixels whose fp64 walks differ; that the loosest rule flags; covered",
            f"{differ.mean():.4f}; {loosest.mean():.4f}; {ref['c'].mean():.4f}")
    assert 0.2 <= differ.mean() <= 0.3 and 0.2 <= loosest.mean() <= 0.3
    assert not (differ & ~loosest).any()                            # the reference's own bracket: a walk that differs met an object
    fg, delta, alpha, rewalked = _diff(s, 1, max_depth, seed)
    assert set(np.unique(rewalked)) <= {0, 1}
    assert not delta.view(np.uint32)[rewalked == 0].any()                                                   # (i)
    missed = differ & (rewalked == 0) & (alpha == 0)
    beyond = (rewalked >= 1) & ~loosest
    _report(f"max_depth {max_depth} seed {seed}: pixels walked twice; differing and neither covered nor walked twice (bound 0.01); walked twice "
            f"outside the loosest rule (bound 0.01)", f"{int((rewalked >= 1).sum())}; {missed.mean():.4f}; {beyond.mean():.4f}")
    assert missed.mean() <= 0.01                                                                            # (ii)
    assert beyond.mean() <= 0.01                                                                            # (iii)
    assert not ((rewalked >= 1) & (alpha > 0)).any() and (rewalked >= 1).any()


def test_a_light_rewalks_every_uncovered_sample(pt, rough_scene):
    s = rough_scene
    spp = 5
    rays = torch.zeros(s["H"], s["W"], dtype=torch.int32, device=s["tracer"].device)
    fg, delta, alpha, rewalked = _diff(s, spp, 6, 3, spp_per_launch=2, rays=rays)
    covered = np.rint(alpha * spp).astype(np.int64)
    assert np.allclose(covered, alpha * spp, atol=1e-5) and 0 < covered.sum() < covered.size * spp
    assert np.array_equal(rewalked + covered, np.full_like(covered, spp))
    # `rays` counts both walks: the render's own rays (another instantiation of the kernel: a path may flip, so in total) and, per
    # second walk, at least its camera ray and at most max_depth closest-hit and max_depth shadow rays
    once = torch.zeros_like(rays)
    s["tracer"].render(*s["maps"], spp=spp, max_depth=6, seed=3, rays=once)
    r2, r1, n2 = int(rays.sum()), int(once.sum()), int(rewalked.sum())
    _report("a table with a light, spp 5: rays of the render; of the differential render; second walks", f"{r1}; {r2}; {n2}")
    assert 0.99 * r1 + n2 <= r2 <= 1.01 * r1 + 12 * n2


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_depth", [2, 16])
def test_an_object_no_path_meets_changes_nothing(pt, hidden_scene, oracle64, max_depth):
    """A cube behind the depth mesh.  On the CPU no traversal of sample 0 of seeds 0-7 returns one of its triangles (asserted first);
    at spp 4 all four outputs are zero, and the composite is the photograph, bit for bit."""
    s = hidden_scene
    assert not pd.any_path_returns_object(oracle64, s, s["tab"], max_depth, range(8), 1)
    photo = torch.from_numpy(np.random.default_rng(3).gamma(2.0, 0.5, (s["H"], s["W"], 3)).astype(np.float32))
    for seed in range(8):
        fg, delta, alpha, rewalked = s["tracer"].render_diff(*s["maps"], spp=4, max_depth=max_depth, seed=seed, spp_per_launch=3)
        for x in (fg, delta, alpha, rewalked):
            assert not bool(x.view(torch.int32).any()), seed
        out = pt.composite(fg, delta, alpha, photo)
        assert np.array_equal(_bits(out), photo.numpy().view(np.uint32))


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_delta_is_the_difference_of_the_existing_kernels_renders(pt, tex_scene):
    """spp 16: in the pixels no camera ray of which lands on an object (alpha = 0), delta is `render` with the objects minus `render`
    of the scene alone, same seed, within 1e-4 of max(|L_with|, |L_without|, mean |L_with|) on at least 0.98 of them.  (fp32
    accumulation of 16 samples is good to 16 x 2^-24 = 1e-6; the margin covers another summation order, the share the ties that the
    scene's own tree breaks the other way.)"""
    s = tex_scene
    alone = pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], s["H"], s["W"], FOV)
    kw = dict(spp=16, max_depth=16, seed=4)
    fg, delta, alpha, rewalked = _diff(s, **kw)
    Lw = s["tracer"].render(*s["maps"], **kw).cpu().numpy().astype(np.float64)
    L0 = alone.render(*s["maps"], **kw).cpu().numpy().astype(np.float64)
    free = alpha == 0
    assert 0.5 < free.mean() < 0.9 and (rewalked[free] > 0).any()
    scale = np.maximum(np.maximum(np.abs(Lw), np.abs(L0)), np.abs(Lw).mean())
    err = (np.abs(delta - (Lw - L0)) / scale).max(-1)[free]
    _report("delta against render(with) - render(scene alone), spp 16, where alpha = 0: share within 1e-4; worst error",
            f"{(err <= 1e-4).mean():.4f}; {err.max():.3e}")
    assert (err <= 1e-4).mean() >= 0.98
    # and where every camera ray lands on an object, fg is the render itself (to the same criterion) and delta is zero
    full = alpha == 1
    err = (np.abs(fg - Lw) / scale).max(-1)[full]
    assert full.sum() > 20 and (err <= 1e-4).mean() >= 0.98 and not delta[full].any()


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_bits(pt, tex_scene, rough_scene):
    for s in (tex_scene, rough_scene):
        tracer, maps = s["tracer"], s["maps"]
        before = tracer.render(*maps, spp=6, max_depth=16, seed=7, spp_per_launch=4)   # recorded before this test's first render_diff
        # every split of a frame into launches gives the same bits in all four outputs
        whole = tracer.render_diff(*maps, spp=6, max_depth=16, seed=7, spp_per_launch=6)
        for split in (1, 3, 4):
            part = tracer.render_diff(*maps, spp=6, max_depth=16, seed=7, spp_per_launch=split)
            for k, (x, y) in enumerate(zip(whole, part)):
                assert np.array_equal(_bits(x), _bits(y)), (split, k)
        # PathTracer.render_diff is the raw call (the count is added to: it starts from zero here)
        dev = tracer.device
        fg, delta = torch.full((s["H"], s["W"], 3), 7.0, device=dev), torch.full((s["H"], s["W"], 3), -7.0, device=dev)
        alpha, rewalked = torch.full((s["H"], s["W"]), 7.0, device=dev), torch.zeros(s["H"], s["W"], dtype=torch.int32, device=dev)
        keep = tracer._inputs(*maps, None)
        args = (*tracer._frame(*keep, 6, 16, 7, 4), None, torch.cuda.current_stream().cuda_stream, *tracer.object_args()[:9], *tracer._texture_args())
        assert len(args) == 18 + 2 + 13
        fn = pt.symbol("matpbr_path_render_objects_diff")
        assert fn(*args, fg.data_ptr(), delta.data_ptr(), alpha.data_ptr(), rewalked.data_ptr()) == 0
        for k, (x, y) in enumerate(zip(whole, (fg, delta, alpha, rewalked))):
            assert np.array_equal(_bits(x), _bits(y)), k
        assert fn(*args, fg.data_ptr(), delta.data_ptr(), alpha.data_ptr(), None) == 0                       # nullable
        assert fn(*args, fg.data_ptr(), delta.data_ptr(), alpha.data_ptr(), rewalked.data_ptr()) == 0        # added to
        assert np.array_equal(rewalked.cpu().numpy(), 2 * whole[3].cpu().numpy())
        # refused: a missing sum, no objects
        for k in range(3):
            ptrs = [fg.data_ptr(), delta.data_ptr(), alpha.data_ptr(), None]
            ptrs[k] = None
            assert fn(*args, *ptrs) == -1, k
        assert fn(*args[:20], None, 0, *args[22:], fg.data_ptr(), delta.data_ptr(), alpha.data_ptr(), None) == -1
        # the composite on the device is its CPU twin
        photo = np.random.default_rng(9).gamma(2.0, 0.5, (s["H"], s["W"], 3)).astype(np.float32)
        for scale in (1.0, 1.0 / 3):
            got = pt.composite(*whole[:3], photo, scale)
            host = pt.composite_host(*(x.cpu().numpy() for x in whole[:3]), photo, scale)
            assert np.array_equal(_bits(got), host.view(np.uint32)), scale
        # `render` of the same tracer gives the bits it gave before
        assert np.array_equal(_bits(before), _bits(tracer.render(*maps, spp=6, max_depth=16, seed=7, spp_per_launch=4)))
    # a tracer without objects has nothing to differ from
    alone = pt.PathTracer(tex_scene["rm"]["vertices"], tex_scene["rm"]["triangles"], tex_scene["H"], tex_scene["W"], FOV)
    with pytest.raises(ValueError, match="objects"):
        alone.render_diff(*tex_scene["maps"], spp=1)


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_render_final_cli_composite(pt, tmp_path):
    """`render_final.py --mode oi --oi_composite` on a synthetic output at 32 x 32 with a gt_image.exr written here: with the hidden cube
    as oi2.ply the .exr is what `write_exr` writes for the photograph itself; with a visible cube the output differs from the photograph
    inside the cube's footprint and is finite.  The plain output's name is not written."""
    from materialist_amd import mesh
    from materialist_amd.imageio_exr import read_exr, write_exr

    tmp = str(tmp_path)
    scene_dir = tl.synthetic_output(tmp)
    photo = np.random.default_rng(4).gamma(2.0, 0.3, (32, 32, 3)).astype(np.float32)
    write_exr(os.path.join(scene_dir, "gt_image.exr"), photo)
    write_exr(os.path.join(tmp, "photo_alone.exr"), photo)
    cmd = [sys.executable, os.path.join(ROOT, "render_final.py"), "--save_name", "case", "--input_path", tmp, "--save_path", tmp, "--mode", "oi",
           "--spp", "4", "--oi_iters", "2", "--oi_composite"]
    exr, png = (os.path.join(tmp, "case", "mi_oic_case_envmap" + ext) for ext in (".exr", ".png"))

    def run(place):
        ob = pd.cube_object(place)
        mesh.write_ply(os.path.join(scene_dir, "oi2.ply"), ob["vertices"].astype(np.float32), ob["triangles"])
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout + res.stderr
        assert os.path.exists(png) and not os.path.exists(os.path.join(tmp, "case", "mi_oi_case_envmap.exr"))
        return ob

    run(pd.HIDDEN_CUBE)
    with open(exr, "rb") as f, open(os.path.join(tmp, "photo_alone.exr"), "rb") as g:
        assert f.read() == g.read()
    ob = run(pd.VISIBLE_CUBE)
    img = np.ascontiguousarray(read_exr(exr)[..., :3], dtype=np.float32)
    inside, outside = tl.footprints([ob], 32, 32)
    assert inside.sum() >= 4 and np.isfinite(img).all() and (img >= 0).all()
    assert (np.abs(img - photo).max(-1)[inside] > 1e-3).all()
    assert (img != photo).any(-1).mean() < 1.0
