"""Ratio shadow transfer on the GPU (libmatpbr_path.so's `matpbr_path_render_objects_ratio` and `matpbr_path_composite_ratio`, DESIGN.md
section 1.4, "Ratio shadow transfer"): every other output keeps the bits of the kernels without `base`, `base` against the fp64 walk
without the objects, the identities that tie it to `render`, bits (launch splits, the raw call, the composite's CPU twin), an object no
path meets, the denoised pipeline of `render_oi`, and `render_final.py --oi_shadows ratio`."""
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
import path_fp64 as pf  # noqa: E402
import path_objects_fp64 as pob  # noqa: E402
import path_oi_fp64 as po  # noqa: E402
import path_rough_fp64 as pr  # noqa: E402
import path_testlib as tl  # noqa: E402
import path_texture_fp64 as px  # noqa: E402
import path_through_fp64 as tf  # noqa: E402
from path_testlib import bits as _bits  # noqa: E402

pytestmark = pytest.mark.gpu

FOV = pf.FOV
_report = tl.reporter("path ratio", "test_gpu_path_ratio")
_u32 = lambda x: np.ascontiguousarray(x).view(np.uint32)


@pytest.fixture(scope="module")
def pt():
    return tl.load(gpu=True)


def _scene(pt, objects):
    s = tl.groove_with_objects(pt, objects, pob.merged)
    s["n_scene"] = s["rm"]["triangles"].shape[0]
    s["tab"] = pt.env_tables(s["env"])
    s["maps"] = (s["a"], s["r"], s["m"], s["env"])
    s["photo"] = tf.photograph(s["H"], s["W"])
    return s


@pytest.fixture(scope="module")
def tex_scene(pt):
    """The groove at 24 x 20 (a partial tile) with `path_texture_fp64.table_scene`: no light, all three flags."""
    s = _scene(pt, px.table_scene())
    assert s["tracer"].stats["n_lights"] == 0 and s["tracer"].stats["n_textured_objects"] == 3
    return s


@pytest.fixture(scope="module")
def rough_scene(pt):
    """The same groove with `path_rough_fp64.table_scene`: a light (every uncovered sample is walked twice), rough and clear glass."""
    s = _scene(pt, pr.table_scene())
    assert s["tracer"].stats["n_lights"] == 1 and s["tracer"].stats["n_rough_objects"] >= 1
    return s


@pytest.fixture(scope="module")
def glass_scene(pt):
    """The see-through test's scene S: the same groove with `path_through_fp64.scene_objects`."""
    return _scene(pt, tf.scene_objects())


def _ratio(s, photo=None, **kw):
    out = s["tracer"].render_diff_ratio(*s["maps"], photo=photo, **kw)
    assert len(out) == (5 if photo is None else 6) and out[2].shape == (s["H"], s["W"], 3) and out[-1].dtype == torch.int32
    return out


# ---- G1 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_depth", [2, 6, 16])
def test_every_other_output_keeps_its_bits(pt, tex_scene, rough_scene, max_depth):
    """fg, delta, alpha, rewalked of `render_diff_ratio` are `render_diff`'s bits, spp 1 and 8; `render`'s own bits are the ones from
    before the first `render_diff_ratio` of the tracer."""
    for s in (tex_scene, rough_scene):
        tracer = s["tracer"]
        before = tracer.render(*s["maps"], spp=8, max_depth=max_depth, seed=3)
        for spp in (1, 8):
            kw = dict(spp=spp, max_depth=max_depth, seed=3)
            fg, delta, base, alpha, rewalked = _ratio(s, **kw)
            for k, (x, y) in enumerate(zip((fg, delta, alpha, rewalked), tracer.render_diff(*s["maps"], **kw))):
                assert np.array_equal(_bits(x), _bits(y)), (spp, k)
            assert bool((rewalked > 0).any()) and bool(torch.isfinite(base).all())
        assert np.array_equal(_bits(before), _bits(tracer.render(*s["maps"], spp=8, max_depth=max_depth, seed=3)))


@pytest.mark.parametrize("max_depth", [3, 16])
def test_with_the_photograph_all_five_outputs_keep_their_bits(pt, glass_scene, max_depth):
    s = glass_scene
    for spp in (1, 8):
        kw = dict(spp=spp, max_depth=max_depth, seed=5)
        fg, delta, base, alpha, through, rewalked = _ratio(s, s["photo"], **kw)
        want = s["tracer"].render_diff_through(*s["maps"], s["photo"], **kw)
        for k, (x, y) in enumerate(zip((fg, delta, alpha, through, rewalked), want)):
            assert np.array_equal(_bits(x), _bits(y)), (spp, k)
        assert bool((through > 0).any())
        # and base does not depend on the rule the covered samples follow
        assert np.array_equal(_bits(base), _bits(_ratio(s, **kw)[2]))
    with pytest.raises(ValueError, match="photo must be"):
        s["tracer"].render_diff_ratio(*s["maps"], spp=1, photo=s["photo"][:-1])


# ---- G2 --------------------------------------------------------------------------------------------------------------------------------
def _base_case(s, oracle64, name, max_depth, seed):
    fg, delta, base, alpha, rewalked = (x.cpu().numpy() for x in _ratio(s, spp=1, max_depth=max_depth, seed=seed))
    ref = pd.reference(oracle64, s, s["tab"], max_depth, seed)
    want = np.where(ref["c"][..., None], 0.0, ref["without"])
    frac, err = pd.share_within(base.astype(np.float64), want, ref["scale"], 1e-3)
    _report(f"{name} scene, max_depth {max_depth} seed {seed}: base against (1 - c) L_without in fp64, share of pixels within 1e-3",
            f"{frac:.4f} ({int((err > 1e-3).sum())} pixels beyond, max err {err.max():.3e})")
    assert frac >= 0.98, (name, max_depth, seed, frac, np.argwhere(err > 1e-3)[:10])
    assert np.isfinite(base).all() and (base >= 0).all() and not _u32(base)[alpha == 1].any() and (alpha == 1).any()
    return ref, base, rewalked


@pytest.mark.parametrize("max_depth", [2, 6, 16])
def test_base_matches_fp64_textures(pt, tex_scene, oracle64, max_depth):
    """spp 1, seeds 0-2, the differential render's own criterion: the error of the worst channel relative to `reference()["scale"]`, at
    least 0.98 of the pixels within 1e-3.  Some uncovered pixels are walked twice and most are not: both sources of `base`."""
    for seed in (0, 1, 2):
        ref, base, rewalked = _base_case(tex_scene, oracle64, "texture", max_depth, seed)
        free = ~ref["c"]
        assert (free & (rewalked == 1)).any() and (free & (rewalked == 0)).mean() > 0.3 and (base[free & (rewalked == 0)] > 0).any()


@pytest.mark.parametrize("max_depth", [6, 16])
def test_base_matches_fp64_light_and_glass(pt, rough_scene, oracle64, max_depth):
    """The same on the table with a light: every uncovered sample is walked twice, so every `base` is a second walk's."""
    for seed in (0, 1, 2):
        ref, base, rewalked = _base_case(rough_scene, oracle64, "rough", max_depth, seed)
        assert (rewalked[~ref["c"]] == 1).mean() >= 0.98


# ---- G3 --------------------------------------------------------------------------------------------------------------------------------
def test_base_and_base_plus_delta_are_the_two_renders(pt, tex_scene):
    """spp 16, where alpha = 0: base + delta is `render` with the objects and base is `render` of a tracer over the scene alone, same
    seed, within 1e-4 of max(|L_with|, |L_without|, mean |L_with|) on at least 0.98 of those pixels: the criterion, and for its
    reasons, of test_gpu_path_diff.py's delta against the two renders."""
    s = tex_scene
    alone = pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], s["H"], s["W"], FOV)
    kw = dict(spp=16, max_depth=16, seed=4)
    fg, delta, base, alpha, rewalked = (x.cpu().numpy() for x in _ratio(s, **kw))
    Lw = s["tracer"].render(*s["maps"], **kw).cpu().numpy().astype(np.float64)
    L0 = alone.render(*s["maps"], **kw).cpu().numpy().astype(np.float64)
    free = alpha == 0
    assert 0.5 < free.mean() < 0.9 and (rewalked[free] > 0).any()
    scale = np.maximum(np.maximum(np.abs(Lw), np.abs(L0)), np.abs(Lw).mean())
    for what, got, ref in (("base + delta against render(with)", base.astype(np.float64) + delta, Lw), ("base against render(scene alone)", base, L0)):
        err = (np.abs(got - ref) / scale).max(-1)[free]
        _report(f"{what}, spp 16, where alpha = 0: share within 1e-4; worst error", f"{(err <= 1e-4).mean():.4f}; {err.max():.3e}")
        assert (err <= 1e-4).mean() >= 0.98, what


# ---- G4 --------------------------------------------------------------------------------------------------------------------------------
def test_launch_splits_and_the_raw_call(pt, tex_scene, rough_scene, glass_scene):
    for s, photo in ((tex_scene, None), (rough_scene, None), (glass_scene, glass_scene["photo"])):
        tracer, maps, dev = s["tracer"], s["maps"], s["tracer"].device
        if photo is not None:
            photo = torch.from_numpy(photo).to(dev)
        kw = dict(spp=8, max_depth=16, seed=7)
        rays = torch.zeros(s["H"], s["W"], dtype=torch.int32, device=dev)
        whole = _ratio(s, photo, spp_per_launch=8, rays=rays, **kw)
        for split in (1, 3):
            r2 = torch.zeros_like(rays)
            part = _ratio(s, photo, spp_per_launch=split, rays=r2, **kw)
            for k, (x, y) in enumerate(zip((*whole, rays), (*part, r2))):
                assert np.array_equal(_bits(x), _bits(y)), (split, k)
        # PathTracer.render_diff_ratio is the raw call (the count is added to: it starts from zero here)
        fg, delta, base, through = (torch.full((s["H"], s["W"], 3), v, device=dev) for v in (7.0, -7.0, 5.0, 3.0))
        alpha, rewalked = torch.full((s["H"], s["W"]), 7.0, device=dev), torch.zeros(s["H"], s["W"], dtype=torch.int32, device=dev)
        keep = tracer._inputs(*maps, None)
        args = (*tracer._frame(*keep, 8, 16, 7, 3), None, torch.cuda.current_stream().cuda_stream, *tracer.object_args()[:9], *tracer._texture_args())
        assert len(args) == 18 + 2 + 13
        fn = pt.symbol("matpbr_path_render_objects_ratio")
        outs = [fg.data_ptr(), delta.data_ptr(), alpha.data_ptr(), rewalked.data_ptr(), photo.data_ptr() if photo is not None else None,
                through.data_ptr() if photo is not None else None, base.data_ptr()]
        assert fn(*args, *outs) == 0
        mine = (fg, delta, base, alpha, rewalked) if photo is None else (fg, delta, base, alpha, through, rewalked)
        for k, (x, y) in enumerate(zip(whole, mine)):
            assert np.array_equal(_bits(x), _bits(y)), k
        assert fn(*args, *outs[:3], None, *outs[4:]) == 0                                                     # rewalked is nullable
        for k in (0, 1, 2, 6):                                                                                # refused: a missing sum
            assert fn(*args, *(None if i == k else x for i, x in enumerate(outs))) == -1, k
        assert fn(*args, *outs[:4], None if photo is not None else base.data_ptr(), outs[5], outs[6]) == -1   # exactly one of photo, through
        assert fn(*args[:20], None, 0, *args[22:], *outs) == -1                                               # no objects
    alone = pt.PathTracer(tex_scene["rm"]["vertices"], tex_scene["rm"]["triangles"], tex_scene["H"], tex_scene["W"], FOV)
    with pytest.raises(ValueError, match="render_diff_ratio.*objects"):
        alone.render_diff_ratio(*tex_scene["maps"], spp=1)


# ---- G5 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_depth", [2, 16])
def test_an_object_no_path_meets_changes_nothing(pt, oracle64, max_depth):
    """A cube behind the depth mesh (no traversal of sample 0 of seeds 0-3 returns one of its triangles, asserted on the CPU first): fg,
    delta, alpha and rewalked are zero, base is base + delta and the scene's radiance, and `composite_ratio` is the photograph."""
    s = _scene(pt, [pd.cube_object(pd.HIDDEN_CUBE)])
    assert not pd.any_path_returns_object(oracle64, s, s["tab"], max_depth, range(4), 1)
    photo = torch.from_numpy(s["photo"])
    for seed in range(4):
        fg, delta, base, alpha, rewalked = _ratio(s, spp=4, max_depth=max_depth, seed=seed, spp_per_launch=3)
        for x in (fg, delta, alpha, rewalked):
            assert not bool(x.view(torch.int32).any()), seed
        assert np.array_equal(_bits(base + delta), _bits(base)) and bool((base > 0).any())
        assert np.array_equal(_bits(pt.composite_ratio(fg, delta, base, alpha, photo)), photo.numpy().view(np.uint32))


# ---- G6 --------------------------------------------------------------------------------------------------------------------------------
def test_composite_bits_on_real_sums(pt, tex_scene):
    """The texture scene's sums of 3 frames at spp 8: channels of both kinds are there (asserted first); `composite_ratio` on the device
    is its CPU twin bit for bit; a channel with delta >= 0 carries `composite`'s bits, and the darkened ones do not all."""
    s = tex_scene
    sums = None
    for seed in range(3):
        frame = _ratio(s, spp=8, max_depth=16, seed=seed)[:4]
        sums = frame if sums is None else tuple(x + y for x, y in zip(sums, frame))
    fg, delta, base, alpha = sums
    d, b = delta.cpu().numpy(), base.cpu().numpy()
    dark, bright = (d < 0) & (b > 0), d > 0
    _report("texture scene, 3 frames at spp 8: share of channels with delta < 0 < base; with delta > 0; with delta = 0",
            f"{dark.mean():.4f}; {bright.mean():.4f}; {(d == 0).mean():.4f}")
    assert dark.mean() > 0.05 and bright.mean() > 0.01 and (d == 0).any()
    photo = np.random.default_rng(9).gamma(2.0, 0.5, (s["H"], s["W"], 3)).astype(np.float32)
    for scale in (1.0 / 3, 1.0):
        got = pt.composite_ratio(fg, delta, base, alpha, photo, scale)
        host = pt.composite_ratio_host(*(x.cpu().numpy() for x in (fg, delta, base, alpha)), photo, scale)
        assert np.array_equal(_bits(got), _u32(host)), scale
        plain = _bits(pt.composite(fg, delta, alpha, photo, scale))
        assert np.array_equal(_bits(got)[d >= 0], plain[d >= 0])
        assert np.array_equal(_bits(got)[~dark], plain[~dark])
        assert (_bits(got)[dark] != plain[dark]).mean() > 0.5


# ---- G7 --------------------------------------------------------------------------------------------------------------------------------
def test_the_denoised_pipeline_is_two_filters_and_the_composite(pt, tmp_path):
    """`render_oi(composite=True, composite_denoise=True, shadows="ratio")` is `composite_ratio` over the outputs of two `denoise_diff`
    calls formed by hand from the same halves, bit for bit: (fg, delta, alpha) as they are, and base in delta's place beside a zero fg."""
    from materialist_amd import mesh, relight
    from materialist_amd.imageio_exr import read_exr, write_exr

    tmp = str(tmp_path)
    scene_dir = tl.synthetic_output(tmp)
    photo = np.random.default_rng(4).gamma(2.0, 0.3, (32, 32, 3)).astype(np.float32)
    write_exr(os.path.join(scene_dir, "gt_image.exr"), photo)
    ob = pd.cube_object(pd.VISIBLE_CUBE)
    mesh.write_ply(os.path.join(scene_dir, "oi2.ply"), ob["vertices"].astype(np.float32), ob["triangles"])
    n_iter, spp, max_depth = 2, 4, 8
    relight.render_oi("case", None, tmp, tmp, spp, n_iter, max_depth, 0, composite=True, composite_denoise=True, shadows="ratio")
    got = np.ascontiguousarray(read_exr(os.path.join(tmp, "case", "mi_oic_case_envmap.exr"))[..., :3], dtype=np.float32)
    mat = relight.load_estimated_brdf(os.path.join(scene_dir, "best_results"))
    env = relight.load_image(os.path.join(scene_dir, "best_results", "envmap.hdr"))
    V, T = mesh.read_ply_any(os.path.join(scene_dir, "oi2.ply"))
    bsdf = {"type": "diffuse", "reflectance": (relight.OI_REFLECTANCE,) * 3}
    tracer = relight._path_tracer(scene_dir, "case", mat, "cuda", [{"vertices": V, "triangles": T, "bsdf": bsdf}])
    ph = torch.from_numpy(photo).to(tracer.device)
    halves = [None, None]
    for i in range(n_iter):
        for k in (0, 1):
            frame = tracer.render_diff_ratio(mat["albedo"], mat["roughness"], mat["metallic"], env, spp // 2, max_depth, 2 * i + k)[:4]
            halves[k] = frame if halves[k] is None else tuple(x + y for x, y in zip(halves[k], frame))
    geom = tracer.features()
    guide = relight.albedo_guide(geom, mat["albedo"], [bsdf], None)
    (fgA, dA, bA, alA), (fgB, dB, bB, alB) = halves
    fg, delta, alpha = tracer.denoise_diff((fgA, dA, alA), (fgB, dB, alB), guide, geom, 1.0 / n_iter)
    zero = torch.zeros_like(fgA)
    base = tracer.denoise_diff((zero, bA, alA), (zero, bB, alB), guide, geom, 1.0 / n_iter)[1]
    want = pt.composite_ratio(fg, delta, base, alpha, ph, 1.0)
    assert bool(((delta < 0) & (base > 0)).any())
    assert np.array_equal(_u32(got), _bits(want))
    assert not np.array_equal(_u32(got), _bits(pt.composite(fg, delta, alpha, ph, 1.0)))


def test_beyond_the_filters_reach_the_photograph_keeps_its_bits(pt, tex_scene):
    """The texture scene, two halves at spp 8, one level (R = 3).  `base` is non-zero nearly everywhere, so the filtered `base` is too;
    the rule is still the additive composite's, since a pixel whose filtered delta is 0 takes the additive branch and never reads
    `base`: every pixel with fg = alpha = 0 in both halves and delta zero within the level's own reach 2 of it (the set
    test_gpu_diff_denoise.py asserts this on, which holds every pixel farther than R from every touched one) keeps the photograph's bits."""
    from materialist_amd.relight import albedo_guide

    s = tex_scene
    tracer = s["tracer"]
    (fgA, dA, bA, alA, _), (fgB, dB, bB, alB, _) = (_ratio(s, spp=8, max_depth=6, seed=seed) for seed in (0, 1))
    geom = tracer.features()
    guide = albedo_guide(geom, torch.from_numpy(s["a"]).cuda(), [ob["bsdf"] for ob in s["objects"]], tracer.feature_tints())
    fg, delta, alpha = tracer.denoise_diff((fgA, dA, alA), (fgB, dB, alB), guide, geom, 1.0, levels=1)
    zero = torch.zeros_like(fgA)
    base = tracer.denoise_diff((zero, bA, alA), (zero, bB, alB), guide, geom, 1.0, levels=1)[1]
    photo = np.random.default_rng(6).gamma(2.0, 0.5, (s["H"], s["W"], 3)).astype(np.float32)
    out = pt.composite_ratio(fg, delta, base, alpha, photo, 1.0).cpu().numpy()
    busy, touched = np.zeros((s["H"], s["W"]), bool), np.zeros((s["H"], s["W"]), bool)
    for f, d, al in ((fgA, dA, alA), (fgB, dB, alB)):
        busy |= (f.cpu().numpy() != 0).any(-1) | (al.cpu().numpy() != 0)
        touched |= (d.cpu().numpy() != 0).any(-1)
    loose = dd.chebyshev_to(busy | touched) > dd.reach(1)
    tight = ~busy & (dd.chebyshev_to(touched) > dd.reach(1) - 1)
    kept = (_u32(out) == _u32(photo)).all(-1)
    _report("texture scene, L = 1: pixels all zero within R = 3; with fg = alpha = 0 and delta zero within 2; that keep the photograph's bits; "
            "with a non-zero filtered base", (int(loose.sum()), int(tight.sum()), int(kept.sum()), int((base.cpu().numpy() != 0).any(-1).sum())))
    assert not (loose & ~tight).any() and tight.sum() > 0 and int((kept & tight).sum()) == int(tight.sum())
    assert (base.cpu().numpy()[tight] != 0).any() and not kept.all()


# ---- G8 --------------------------------------------------------------------------------------------------------------------------------
def _cli_scene(tmp):
    """`path_testlib.synthetic_output` at 32 x 32 with gt_image.exr, a glass cube as oi.ply and the visible diffuse cube as oi2.ply ->
    (scene_dir, the photograph, the command without the feature's flag, the .exr it writes)."""
    from materialist_amd import mesh
    from materialist_amd.imageio_exr import write_exr

    scene_dir = tl.synthetic_output(tmp)
    photo = np.random.default_rng(4).gamma(2.0, 0.3, (32, 32, 3)).astype(np.float32)
    write_exr(os.path.join(scene_dir, "gt_image.exr"), photo)
    for name, ob in (("oi.ply", pd.cube_object(((-0.16, 0.02, -0.9), 0.12, (0.2, 0.3, 0.1)), po.GLASS)), ("oi2.ply", pd.cube_object(pd.VISIBLE_CUBE))):
        mesh.write_ply(os.path.join(scene_dir, name), ob["vertices"].astype(np.float32), ob["triangles"])
    cmd = [sys.executable, os.path.join(ROOT, "render_final.py"), "--save_name", "case", "--input_path", tmp, "--save_path", tmp, "--mode", "oi",
           "--spp", "4", "--oi_iters", "2", "--oi_max_depth", "8", "--oi_composite"]
    return scene_dir, photo, cmd, os.path.join(tmp, "case", "mi_oic_case_envmap.exr")


@pytest.mark.parametrize("extra", [[], ["--oi_composite_denoise"], ["--oi_see_through"], ["--oi_composite_denoise", "--oi_see_through"]],
                         ids=["plain", "denoise", "see_through", "denoise+see_through"])
def test_render_final_cli_ratio(pt, tmp_path, extra):
    """`render_final.py --mode oi --oi_composite --oi_shadows ratio` in a fresh process: mi_oic_* is written, finite and >= 0, and is
    what `render_oi` writes for the same arguments in this process."""
    from materialist_amd import relight
    from materialist_amd.imageio_exr import read_exr

    tmp = str(tmp_path)
    scene_dir, photo, cmd, exr = _cli_scene(tmp)
    res = subprocess.run(cmd + ["--oi_shadows", "ratio"] + extra, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert os.path.exists(exr[:-4] + ".png") and not os.path.exists(os.path.join(tmp, "case", "mi_oi_case_envmap.exr"))
    img = np.ascontiguousarray(read_exr(exr)[..., :3], dtype=np.float32)
    assert np.isfinite(img).all() and (img >= 0).all() and (img != photo).any()
    with open(exr, "rb") as f:
        cli = f.read()
    relight.render_oi("case", None, tmp, tmp, 4, 2, 8, 0, composite=True, shadows="ratio", composite_denoise="--oi_composite_denoise" in extra,
                      see_through="--oi_see_through" in extra)
    with open(exr, "rb") as f:
        assert f.read() == cli


def test_render_final_cli_without_the_flag_is_the_additive_composite(pt, tmp_path):
    """The same command without `--oi_shadows`: the bytes are those of the additive pipeline formed by hand from `render_diff` and
    `composite`, the kernels and the code path from before the flag; `--oi_shadows ratio` writes other bytes."""
    from materialist_amd import mesh, relight
    from materialist_amd.imageio_exr import write_exr

    tmp = str(tmp_path)
    scene_dir, photo, cmd, exr = _cli_scene(tmp)
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    with open(exr, "rb") as f:
        cli = f.read()
    mat = relight.load_estimated_brdf(os.path.join(scene_dir, "best_results"))
    env = relight.load_image(os.path.join(scene_dir, "best_results", "envmap.hdr"))
    bsdfs = ({"type": "dielectric", "int_ior": relight.OI_INT_IOR, "ext_ior": relight.OI_EXT_IOR}, {"type": "diffuse", "reflectance": (relight.OI_REFLECTANCE,) * 3})
    objects = []
    for name, bsdf in zip(("oi.ply", "oi2.ply"), bsdfs):
        V, T = mesh.read_ply_any(os.path.join(scene_dir, name))
        objects.append({"vertices": V, "triangles": T, "bsdf": bsdf})
    tracer = relight._path_tracer(scene_dir, "case", mat, "cuda", objects)
    sums = None
    for i in range(2):
        frame = tracer.render_diff(mat["albedo"], mat["roughness"], mat["metallic"], env, 4, 8, i)[:3]
        sums = frame if sums is None else tuple(x + y for x, y in zip(sums, frame))
    by_hand = os.path.join(tmp, "by_hand.exr")
    write_exr(by_hand, pt.composite(*sums, torch.from_numpy(photo).to(tracer.device), 0.5).cpu().numpy())
    with open(by_hand, "rb") as f:
        assert f.read() == cli
    relight.render_oi("case", None, tmp, tmp, 4, 2, 8, 0, composite=True, shadows="ratio")
    with open(exr, "rb") as f:
        assert f.read() != cli
