"""The photograph seen through inserted glass on the GPU (libmatpbr_path.so's `matpbr_path_render_objects_through`, DESIGN.md section
1.4, "Seen through glass"): every output against the fp64 statement of `path_through_fp64`, what the feature must not touch, a table
without glass, linearity in the photograph, index-matched glass, the untouched tail, bits and refusals, the count of second walks, the
denoiser's plumbing in `render_oi`, and `render_final.py --oi_see_through`."""
import json
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
import path_oi_fp64 as po  # noqa: E402
import path_testlib as tl  # noqa: E402
import path_through_fp64 as tf  # noqa: E402
from path_testlib import bits as _bits  # noqa: E402

pytestmark = pytest.mark.gpu

FOV = pf.FOV
MATCHED = {"type": "dielectric", "int_ior": 1.5, "ext_ior": 1.5}
_report = tl.reporter("path through", "test_gpu_path_through")


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
def scene(pt):
    """Scene S: the groove at 24 x 20 (a partial tile) with `path_through_fp64.scene_objects`."""
    s = _scene(pt, tf.scene_objects())
    assert s["tracer"].stats["n_lights"] == 0 and s["tracer"].stats["n_smooth_objects"] == 1
    return s


@pytest.fixture(scope="module")
def light_scene(pt):
    """S_light: S plus `path_light_fp64`'s small area light."""
    s = _scene(pt, tf.scene_objects(light=True))
    assert s["tracer"].stats["n_lights"] == 1
    return s


def _through(s, spp, max_depth, seed, photo=None, **kw):
    out = s["tracer"].render_diff_through(*s["maps"], s["photo"] if photo is None else photo, spp=spp, max_depth=max_depth, seed=seed, **kw)
    fg, delta, alpha, through, rewalked = out
    assert fg.shape == (s["H"], s["W"], 3) and delta.shape == fg.shape and through.shape == fg.shape
    assert alpha.shape == (s["H"], s["W"]) and rewalked.shape == alpha.shape and rewalked.dtype == torch.int32
    return tuple(x.cpu().numpy() for x in out)


def _diff(s, spp, max_depth, seed, **kw):
    return tuple(x.cpu().numpy() for x in s["tracer"].render_diff(*s["maps"], spp=spp, max_depth=max_depth, seed=seed, **kw))


def _u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
def _parity_case(s, oracle64, name, max_depth, seed):
    fg, delta, alpha, through, rewalked = _through(s, 1, max_depth, seed)
    assert all(np.isfinite(x).all() for x in (fg, delta, through))
    ref = tf.reference(oracle64, s, s["tab"], s["photo"], max_depth, seed)
    scales = {"fg": ref["scale"], "delta": ref["scale"], "through": np.maximum(np.abs(ref["through"]), np.abs(ref["through"]).mean())}
    for what, got in (("fg", fg), ("through", through), ("delta", delta)):
        frac, err = pd.share_within(got.astype(np.float64), ref[what], scales[what], 1e-3)
        _report(f"{name}, max_depth {max_depth} seed {seed}: {what} against the fp64 statement, share of pixels within 1e-3",
                f"{frac:.4f} ({int((err > 1e-3).sum())} pixels beyond, max err {err.max():.3e})")
        assert frac >= 0.98, (name, what, max_depth, seed, frac, np.argwhere(err > 1e-3)[:10])
    agree = float((alpha == ref["alpha"]).mean())
    _report(f"{name}, max_depth {max_depth} seed {seed}: alpha against the camera ray's brute-force coverage, share of pixels equal; see-through "
            f"lanes; of them with a tail that differs", f"{agree:.4f}; {int(ref['see'].sum())}; {int((ref['tail'] != ref['with'])[ref['see']].any(-1).sum())}")
    assert agree >= 0.98 and set(np.unique(alpha)) <= {0.0, 1.0}
    return ref


@pytest.mark.parametrize("max_depth", [3, 6, 16])
def test_every_output_matches_fp64(pt, scene, oracle64, max_depth):
    """S, spp 1, seeds 0-2: fg against c (L_with - [see-through] L_tail), through against thr_k photo[q], delta and alpha as the
    differential render's own parity test, the error of the worst channel relative to `path_diff_fp64`'s scale (through: relative to
    max(|ref|, mean |ref|)); at least 0.98 of the pixels within 1e-3, that test's criterion for the same reason: two walks."""
    tf.preconditions(scene, oracle64)
    for seed in (0, 1, 2):
        ref = _parity_case(scene, oracle64, "S", max_depth, seed)
        assert ref["see"].mean() >= 0.2 and (ref["through"] > 0).any()
        if max_depth > 3:   # some tails differ (the diffuse cube, the other glass) and some are exactly equal
            differs = (ref["tail"] != ref["with"]).any(-1) & ref["see"]
            assert differs.any() and (ref["see"] & ~differs).any()


@pytest.mark.parametrize("seed", [0, 1])
def test_every_output_matches_fp64_with_a_light(pt, light_scene, oracle64, seed):
    """The same on S_light, max_depth 6: n_e differs between the walks, so every see-through sample with a tail is walked twice."""
    ref = _parity_case(light_scene, oracle64, "S_light", 6, seed)
    assert ref["see"].mean() >= 0.1


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["S", "S_light"])
def test_what_the_feature_must_not_touch(pt, scene, light_scene, oracle64, which):
    """spp 6, max_depth 16: delta and alpha have `render_diff`'s bits; through is all-zero bits where alpha = 0; fg has `render_diff`'s
    bits in every pixel with alpha > 0 no sample of which is see-through by the fp64 chain, but for at most 0.01 of the pixels (chains
    that flip on a tie); `render` and `render_diff` of the same tracer give the bits they gave before the first `render_diff_through`."""
    s = scene if which == "S" else light_scene
    kw = dict(spp=6, max_depth=16, seed=5)
    tracer = s["tracer"]
    before = tracer.render(*s["maps"], **kw).cpu().numpy()
    d_fg, d_delta, d_alpha, d_rewalked = _diff(s, **kw)
    fg, delta, alpha, through, rewalked = _through(s, **kw)
    assert np.array_equal(_u32(delta), _u32(d_delta)) and np.array_equal(_u32(alpha), _u32(d_alpha))
    assert not _u32(through)[alpha == 0].any() and (through > 0).any()
    see_any = np.zeros(s["H"] * s["W"], bool)
    for sample in range(6):
        see_any |= tf.chains(oracle64, s, 16, 5, sample)["k"] >= 0
    plain = (alpha > 0) & ~see_any.reshape(s["H"], s["W"])
    differ = plain & (_u32(fg) != _u32(d_fg)).any(-1)
    _report(f"{which}: pixels with alpha > 0 and no see-through sample in fp64; of them with other fg bits than render_diff (bound 0.01 of the "
            f"pixels)", f"{int(plain.sum())}; {int(differ.sum())}")
    assert plain.sum() >= 20 and differ.mean() <= 0.01
    assert (_u32(fg) != _u32(d_fg)).any()                                     # and the see-through pixels did change
    assert np.array_equal(_u32(before), _u32(tracer.render(*s["maps"], **kw).cpu().numpy()))
    for x, y in zip((d_fg, d_delta, d_alpha, d_rewalked), _diff(s, **kw)):
        assert np.array_equal(_u32(x), _u32(y))


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_table_without_glass(pt, oracle64):
    """A diffuse cube in front of the mesh: fg, delta, alpha and rewalked are `render_diff`'s bits and through is all-zero bits.  A cube
    behind the mesh: all five outputs are zero and the composite is the photograph bit for bit."""
    s = _scene(pt, [pd.cube_object(pd.VISIBLE_CUBE)])
    kw = dict(spp=4, max_depth=16, seed=2, spp_per_launch=3)
    fg, delta, alpha, through, rewalked = _through(s, **kw)
    assert (alpha > 0).any() and (rewalked > 0).any()
    for x, y in zip((fg, delta, alpha, rewalked), _diff(s, **kw)):
        assert np.array_equal(_u32(x), _u32(y))
    assert not _u32(through).any()
    h = _scene(pt, [pd.cube_object(pd.HIDDEN_CUBE)])
    assert not pd.any_path_returns_object(oracle64, h, h["tab"], 16, range(2), 1)
    photo = torch.from_numpy(h["photo"])
    for seed in range(2):
        out = h["tracer"].render_diff_through(*h["maps"], photo, spp=4, max_depth=16, seed=seed, spp_per_launch=3)
        for x in out:
            assert not bool(x.view(torch.int32).any()), seed
        fg, delta, alpha, through, _ = out
        assert np.array_equal(_bits(pt.composite(fg + through, delta, alpha, photo)), photo.numpy().view(np.uint32))


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_photograph_enters_linearly_and_only_through_through(pt, scene):
    kw = dict(spp=3, max_depth=16, seed=4)
    one = _through(scene, **kw)
    two = _through(scene, photo=2.0 * scene["photo"], **kw)
    assert (one[3] > 0).any() and np.array_equal(two[3], 2.0 * one[3])
    for k in (0, 1, 2, 4):
        assert np.array_equal(_u32(one[k]), _u32(two[k])), k
    none = _through(scene, photo=np.zeros_like(scene["photo"]), **kw)
    assert not _u32(none[3]).any()
    for k in (0, 1, 2, 4):
        assert np.array_equal(_u32(one[k]), _u32(none[k])), k
    with pytest.raises(ValueError, match="photo must be"):
        scene["tracer"].render_diff_through(*scene["maps"], scene["photo"][:-1], spp=1)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_index_matched_glass_shows_the_photograph(pt, oracle64):
    """One flat glass cube with int_ior = ext_ior in front of the mesh, spp 4, max_depth 16.  In the fp64 chain first: of the covered
    lanes, at least 0.98 are see-through with thr_k = 1 and q the lane's own pixel.  Then on the device: in the pixels with alpha = 1,
    through is within 1e-5 relative of the photograph at that pixel on at least 0.98 of them."""
    s = _scene(pt, [pd.cube_object(((0.0, 0.0, -1.2), 0.3, (0.4, 0.5, 0.3)), MATCHED)])
    n = s["H"] * s["W"]
    for sample in range(4):
        ch = tf.chains(oracle64, s, 16, 3, sample)
        cov = ch["covered"]
        good = cov & (ch["k"] >= 0) & (ch["thr"] == 1.0) & (ch["q"] == np.arange(n))
        assert cov.sum() >= 40 and good.sum() >= 0.98 * cov.sum(), (sample, int(cov.sum()), int(good.sum()))
    fg, delta, alpha, through, rewalked = _through(s, 4, 16, 3)
    full = alpha == 1
    err = (np.abs(through - s["photo"]) / s["photo"]).max(-1)[full]
    _report("index-matched glass: pixels with alpha = 1; share with through within 1e-5 of the photograph (bound 0.98); worst error",
            f"{int(full.sum())}; {(err <= 1e-5).mean():.4f}; {err.max():.3e}")
    assert full.sum() >= 30 and (err <= 1e-5).mean() >= 0.98


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_untouched_tail_is_exact(pt):
    """The far glass cube of S alone, max_depth 2, spp 4: every landing is cut, so no second walk can run.  rewalked is 0 in every pixel
    with alpha = 1, fg there has `render_diff`'s bits, and through > 0 somewhere, where `render_diff`'s fg is 0."""
    s = _scene(pt, [pd.cube_object(tf.FAR_GLASS_CUBE, po.GLASS)])
    kw = dict(spp=4, max_depth=2, seed=1)
    fg, delta, alpha, through, rewalked = _through(s, **kw)
    d_fg = _diff(s, **kw)[0]
    full = alpha == 1
    assert full.sum() >= 10 and not rewalked[full].any()
    assert np.array_equal(_u32(fg)[full], _u32(d_fg)[full])
    seen = (through > 0).any(-1)
    assert (seen & ~d_fg.any(-1)).any()


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_bits_and_refusals(pt, scene, light_scene):
    for s in (scene, light_scene):
        tracer, maps = s["tracer"], s["maps"]
        photo = torch.from_numpy(s["photo"]).to(tracer.device)
        kw = dict(spp=6, max_depth=16, seed=7)
        whole = tracer.render_diff_through(*maps, photo, spp_per_launch=6, **kw)
        for split in (1, 3, 4):
            part = tracer.render_diff_through(*maps, photo, spp_per_launch=split, **kw)
            for k, (x, y) in enumerate(zip(whole, part)):
                assert np.array_equal(_bits(x), _bits(y)), (split, k)
        # PathTracer.render_diff_through is the raw call (the count is added to: it starts from zero here)
        dev = tracer.device
        fg, delta, through = (torch.full((s["H"], s["W"], 3), v, device=dev) for v in (7.0, -7.0, 3.0))
        alpha, rewalked = torch.full((s["H"], s["W"]), 7.0, device=dev), torch.zeros(s["H"], s["W"], dtype=torch.int32, device=dev)
        keep = tracer._inputs(*maps, None)
        args = (*tracer._frame(*keep, 6, 16, 7, 4), None, torch.cuda.current_stream().cuda_stream,
                *tracer.object_args()[:pt.OBJECT_ENTRIES["matpbr_path_render_objects_through"] - 4], *tracer._texture_args())
        assert len(args) == 18 + 2 + 13
        fn = pt.symbol("matpbr_path_render_objects_through")
        outs = [fg.data_ptr(), delta.data_ptr(), alpha.data_ptr(), rewalked.data_ptr(), photo.data_ptr(), through.data_ptr()]
        assert fn(*args, *outs) == 0
        for k, (x, y) in enumerate(zip(whole, (fg, delta, alpha, through, rewalked))):
            assert np.array_equal(_bits(x), _bits(y)), k
        assert fn(*args, *outs[:3], None, *outs[4:]) == 0                                                     # nullable
        assert fn(*args, *outs) == 0                                                                          # added to
        assert np.array_equal(rewalked.cpu().numpy(), 2 * whole[4].cpu().numpy())
        for k in (0, 1, 2, 4, 5):                                                                             # refused: a missing buffer, no objects
            ptrs = list(outs)
            ptrs[k] = None
            assert fn(*args, *ptrs) == -1, k
        assert fn(*args[:20], None, 0, *args[22:], *outs) == -1
    alone = pt.PathTracer(scene["rm"]["vertices"], scene["rm"]["triangles"], scene["H"], scene["W"], FOV)
    with pytest.raises(ValueError, match="objects"):
        alone.render_diff_through(*scene["maps"], scene["photo"], spp=1)


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_rewalked_counts_both_kinds(pt, scene):
    s = scene
    spp, max_depth = 5, 6
    rays = torch.zeros(s["H"], s["W"], dtype=torch.int32, device=s["tracer"].device)
    fg, delta, alpha, through, rewalked = _through(s, spp, max_depth, 3, spp_per_launch=2, rays=rays)
    assert rewalked.min() >= 0 and rewalked.max() <= spp
    assert ((alpha == 1) & (rewalked >= 1)).any() and ((alpha == 0) & (rewalked >= 1)).any()
    assert not _diff(s, spp, max_depth, 3)[3][alpha == 1].any()              # that cannot happen in render_diff
    once = torch.zeros_like(rays)
    s["tracer"].render(*s["maps"], spp=spp, max_depth=max_depth, seed=3, rays=once)
    r2, r1, n2 = int(rays.sum()), int(once.sum()), int(rewalked.sum())
    _report("S, spp 5: rays of the render; of the see-through differential render; second walks", f"{r1}; {r2}; {n2}")
    assert 0.99 * r1 + n2 <= r2 <= 1.01 * r1 + 2 * max_depth * n2


# ---- 9, 10 -----------------------------------------------------------------------------------------------------------------------------
def _glass_listing(tmp, bsdf):
    """`path_testlib.synthetic_output` at 32 x 32 with gt_image.exr and a one-object list, a glass cube in front of the mesh ->
    (scene_dir, the photograph, the list's path, the object)."""
    from materialist_amd import mesh
    from materialist_amd.imageio_exr import write_exr

    scene_dir = tl.synthetic_output(tmp)
    photo = np.random.default_rng(4).gamma(2.0, 0.3, (32, 32, 3)).astype(np.float32)
    write_exr(os.path.join(scene_dir, "gt_image.exr"), photo)
    ob = pd.cube_object(((0.02, 0.0, -0.9), 0.2, (0.4, 0.5, 0.3)), bsdf)
    os.makedirs(os.path.join(tmp, "lists"))
    mesh.write_ply(os.path.join(tmp, "lists", "glass.ply"), ob["vertices"].astype(np.float32), ob["triangles"])
    listing = os.path.join(tmp, "lists", "glass.json")
    with open(listing, "w") as f:
        json.dump({"objects": [{"ply": "glass.ply", "bsdf": bsdf}]}, f)
    return scene_dir, photo, listing, ob


def test_the_denoiser_takes_fg_and_leaves_through(pt, tmp_path):
    """`render_oi(composite=True, composite_denoise=True, see_through=True)` is `composite(fg' + through_mean, delta', alpha', photo, 1)`
    formed by hand from the same halves, bit for bit: through does not pass the filter."""
    from materialist_amd import mesh, relight
    from materialist_amd.imageio_exr import read_exr

    tmp = str(tmp_path)
    scene_dir, photo, listing, _ = _glass_listing(tmp, po.GLASS)
    n_iter, spp, max_depth = 2, 4, 8
    relight.render_oi("case", None, tmp, tmp, spp, n_iter, max_depth, 0, objects_file=listing, composite=True, composite_denoise=True, see_through=True)
    got = np.ascontiguousarray(read_exr(os.path.join(tmp, "case", "mi_oic_case_envmap.exr"))[..., :3], dtype=np.float32)
    mat = relight.load_estimated_brdf(os.path.join(scene_dir, "best_results"))
    env = relight.load_image(os.path.join(scene_dir, "best_results", "envmap.hdr"))
    V, T = mesh.read_ply_any(os.path.join(tmp, "lists", "glass.ply"))
    tracer = relight._path_tracer(scene_dir, "case", mat, "cuda", [{"vertices": V, "triangles": T, "bsdf": po.GLASS}])
    ph = torch.from_numpy(photo).to(tracer.device)
    halves = [None, None]
    for i in range(n_iter):
        for k in (0, 1):
            frame = tracer.render_diff_through(mat["albedo"], mat["roughness"], mat["metallic"], env, ph, spp // 2, max_depth, 2 * i + k)[:4]
            halves[k] = frame if halves[k] is None else tuple(x + y for x, y in zip(halves[k], frame))
    geom = tracer.features()
    guide = relight.albedo_guide(geom, mat["albedo"], [po.GLASS], None)
    fg, delta, alpha = tracer.denoise_diff(halves[0][:3], halves[1][:3], guide, geom, 1.0 / n_iter)
    through = (halves[0][3] + halves[1][3]) * (0.5 / n_iter)
    assert bool((through > 0).any())
    want = pt.composite(fg + through, delta, alpha, ph, 1.0)
    assert np.array_equal(got.view(np.uint32), _bits(want))
    assert not np.array_equal(got.view(np.uint32), _bits(pt.composite(fg, delta, alpha, ph, 1.0)))


def test_render_final_cli_see_through(pt, tmp_path):
    """`render_final.py --mode oi --oi_composite --oi_see_through --oi_scene glass.json` against the same command without the flag, one
    index-matched glass cube in front of the mesh: both exit 0; the two .exr agree bit for bit outside the cube's footprint and differ
    inside it; both are finite and >= 0; with the flag the fully covered pixels lie closer to the photograph than without it on at
    least 0.9 of them (closer, not equal: the glass still shadows the tail)."""
    from materialist_amd.imageio_exr import read_exr

    tmp = str(tmp_path)
    scene_dir, photo, listing, ob = _glass_listing(tmp, MATCHED)
    cmd = [sys.executable, os.path.join(ROOT, "render_final.py"), "--save_name", "case", "--input_path", tmp, "--save_path", tmp, "--mode", "oi",
           "--spp", "4", "--oi_iters", "2", "--oi_composite", "--oi_scene", listing]
    exr = os.path.join(tmp, "case", "mi_oic_case_envmap.exr")

    def run(extra):
        if os.path.exists(exr):
            os.remove(exr)
        res = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout + res.stderr
        img = np.ascontiguousarray(read_exr(exr)[..., :3], dtype=np.float32)
        assert np.isfinite(img).all() and (img >= 0).all()
        return img

    plain, seen = run([]), run(["--oi_see_through"])
    inside, outside = tl.footprints([ob], 32, 32)
    assert inside.sum() >= 9 and outside.sum() >= 100
    assert np.array_equal(plain.view(np.uint32)[outside], seen.view(np.uint32)[outside])
    assert (plain != seen).any(-1)[inside].mean() > 0.9
    closer = np.abs(seen - photo).max(-1)[inside] < np.abs(plain - photo).max(-1)[inside]
    _report("render_final.py --oi_see_through, index-matched glass: fully covered pixels; share closer to the photograph than without the flag "
            "(bound 0.9)", f"{int(inside.sum())}; {closer.mean():.4f}")
    assert closer.mean() >= 0.9
