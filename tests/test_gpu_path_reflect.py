"""The photograph reflected in inserted objects on the GPU (libmatpbr_path.so's `matpbr_path_render_objects_reflect`, DESIGN.md section
1.4, "Reflected in inserted objects"): every output against the fp64 statement of `path_reflect_fp64`, what the feature must not
touch, linearity in the photograph, the untouched tail, the white object in a white room, bits and plumbing, the gain where the fit is
off, and `render_final.py --oi_reflect_photo`."""
import json
import math
import os
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
import path_oi_fp64 as po  # noqa: E402
import path_reflect_fp64 as rf  # noqa: E402
import path_testlib as tl  # noqa: E402
import path_through_fp64 as tf  # noqa: E402
from path_testlib import bits as _bits  # noqa: E402

pytestmark = pytest.mark.gpu

FOV = pf.FOV
_report = tl.reporter("path reflect", "test_gpu_path_reflect")


@pytest.fixture(scope="module")
def pt():
    return tl.load(gpu=True)


def _scene(pt, objects):
    s = tl.groove_with_objects(pt, objects, rf.merged)
    s["n_scene"] = s["rm"]["triangles"].shape[0]
    s["tab"] = pt.env_tables(s["env"])
    s["maps"] = (s["a"], s["r"], s["m"], s["env"])
    s["photo"] = rf.photograph(s["H"], s["W"])
    return s


@pytest.fixture(scope="module")
def scene(pt):
    """Scene R: the groove at 24 x 20 (a partial tile) with `path_reflect_fp64.scene_objects`."""
    s = _scene(pt, rf.scene_objects())
    assert s["tracer"].stats["n_photo_objects"] == 3 and s["tracer"].reflect and s["tracer"].stats["n_lights"] == 0
    return s


@pytest.fixture(scope="module")
def light_scene(pt):
    """R_light: R plus `path_light_fp64`'s small area light."""
    s = _scene(pt, rf.scene_objects(light=True))
    assert s["tracer"].stats["n_lights"] == 1 and s["tracer"].stats["n_photo_objects"] == 3
    return s


@pytest.fixture(scope="module")
def plain_scene(pt):
    """`path_through_fp64`'s scene S: no object carries the flag."""
    s = _scene(pt, tf.scene_objects())
    assert s["tracer"].stats["n_photo_objects"] == 0 and not s["tracer"].reflect
    return s


def _through(s, spp, max_depth, seed, photo=None, maps=None, **kw):
    out = s["tracer"].render_diff_through(*(s["maps"] if maps is None else maps), s["photo"] if photo is None else photo, spp=spp,
                                          max_depth=max_depth, seed=seed, **kw)
    fg, delta, alpha, through, rewalked = out
    assert fg.shape == (s["H"], s["W"], 3) and delta.shape == fg.shape and through.shape == fg.shape
    assert alpha.shape == (s["H"], s["W"]) and rewalked.shape == alpha.shape and rewalked.dtype == torch.int32
    return tuple(x.cpu().numpy() for x in out)


def _diff(s, spp, max_depth, seed, **kw):
    return tuple(x.cpu().numpy() for x in s["tracer"].render_diff(*s["maps"], spp=spp, max_depth=max_depth, seed=seed, **kw))


def _u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _raw(pt, s, entry, spp, max_depth, seed, base=False, media=False, flag=False, spp_per_launch=4, rewalked_in=None):
    """The library's `entry` called past `PathTracer` on scene `s` with its photograph -> (code, fg, delta, [base,] alpha, through,
    rewalked) as `PathTracer` orders them; `flag`: the table with OBJECT_PHOTO."""
    tracer, dev = s["tracer"], s["tracer"].device
    H, W = s["H"], s["W"]
    fg, delta, through, bs = (torch.full((H, W, 3), v, device=dev) for v in (7.0, -7.0, 3.0, 5.0))
    alpha = torch.full((H, W), 7.0, device=dev)
    rewalked = torch.zeros(H, W, dtype=torch.int32, device=dev) if rewalked_in is None else rewalked_in
    photo = torch.from_numpy(s["photo"]).to(dev)
    keep = tracer._inputs(*s["maps"], None)
    args = (*tracer._frame(*keep, spp, max_depth, seed, spp_per_launch), None, torch.cuda.current_stream().cuda_stream,
            *tracer.object_args(flag)[:9], *tracer._texture_args())
    assert len(args) == 18 + 2 + 13
    outs = [fg.data_ptr(), delta.data_ptr(), alpha.data_ptr(), rewalked.data_ptr(), photo.data_ptr(), through.data_ptr()]
    if entry.endswith("_ratio"):
        outs.append(bs.data_ptr())
    elif not entry.endswith("_through"):
        outs += [bs.data_ptr() if base else None, tracer.media_arg() if media else None]
    code = pt.symbol(entry)(*args, *outs)
    torch.cuda.synchronize()
    return (code, fg, delta, *((bs,) if base else ()), alpha, through, rewalked), (args, outs)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
def _parity_case(s, oracle64, name, max_depth, seed):
    fg, delta, alpha, through, rewalked = _through(s, 1, max_depth, seed)
    assert all(np.isfinite(x).all() for x in (fg, delta, through))
    ref = rf.reference(oracle64, s, s["tab"], s["photo"], max_depth, seed)
    scales = {"fg": ref["scale"], "delta": ref["scale"], "through": np.maximum(np.abs(ref["through"]), np.abs(ref["through"]).mean())}
    for what, got in (("fg", fg), ("through", through), ("delta", delta)):
        frac, err = pd.share_within(got.astype(np.float64), ref[what], scales[what], 1e-3)
        _report(f"{name}, max_depth {max_depth} seed {seed}: {what} against the fp64 statement, share of pixels within 1e-3",
                f"{frac:.4f} ({int((err > 1e-3).sum())} pixels beyond, max err {err.max():.3e})")
        assert frac >= 0.98, (name, what, max_depth, seed, frac, np.argwhere(err > 1e-3)[:10])
    agree = float((alpha == ref["alpha"]).mean())
    _report(f"{name}, max_depth {max_depth} seed {seed}: alpha against the camera ray's brute-force coverage, share of pixels equal; see-through "
            f"lanes; of them through a flagged vertex; of them with a touched tail",
            f"{agree:.4f}; {int(ref['see'].sum())}; {int((ref['chain']['flagged'] & (ref['chain']['k'] >= 0)).sum())}; {int(ref['touched'].sum())}")
    assert agree >= 0.98 and set(np.unique(alpha)) <= {0.0, 1.0}
    return ref


@pytest.mark.parametrize("max_depth", [2, 3, 6])
def test_every_output_matches_fp64(pt, scene, oracle64, max_depth):
    """R, spp 1, seeds 0 and 1: fg against c (L_with - [see-through] tail), through against thr_k photo[q], delta and alpha as the
    differential render's own parity test, with `test_gpu_path_through.py`'s error scales; at least 0.98 of the pixels within 1e-3, the
    criterion for two walks in use there: fp32 / fp64 hit decisions flip a few paths."""
    rf.preconditions(scene, oracle64, scene["tab"])
    for seed in (0, 1):
        ref = _parity_case(scene, oracle64, "R", max_depth, seed)
        # of the fp64 statement itself: max_depth 2 lands at depth 1 alone, 45 and 38 lanes by seed, 14 and 8 of them with light of the chain's own
        assert ref["see"].sum() >= 30 and (ref["through"] > 0).any()
        assert (np.abs(ref["lchain"]).max(-1) > 0)[ref["see"]].sum() >= (5 if max_depth == 2 else 20)
        if max_depth > 3:
            assert ref["touched"].sum() >= 20 and (ref["see"] & ~ref["touched"]).sum() >= 20


def test_every_output_matches_fp64_with_a_light(pt, light_scene, oracle64):
    """The same on R_light, max_depth 6, seed 0: n_e differs between the walks, so the chain's emitter samples must not be subtracted."""
    ref = _parity_case(light_scene, oracle64, "R_light", 6, 0)
    assert ref["see"].mean() >= 0.1


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_delta_and_alpha_are_render_diffs_bits(pt, scene, light_scene):
    for s in (scene, light_scene):
        kw = dict(spp=4, max_depth=6, seed=5)
        d_fg, d_delta, d_alpha, _ = _diff(s, **kw)
        fg, delta, alpha, through, _ = _through(s, **kw)
        assert np.array_equal(_u32(delta), _u32(d_delta)) and np.array_equal(_u32(alpha), _u32(d_alpha))
        assert not _u32(through)[alpha == 0].any() and (through > 0).any() and (_u32(fg) != _u32(d_fg)).any()


def test_a_table_without_the_flag_gives_the_existing_entries_bits(pt, plain_scene):
    """On S the new entry returns the bits of `matpbr_path_render_objects_through` in all five outputs, of `_ratio` with `base`, and, on
    S with an absorbing and scattering medium in its sunk cube, of `_diff_media` in both shapes."""
    new = "matpbr_path_render_objects_reflect"
    kw = dict(spp=5, max_depth=8, seed=3)
    cases = [(plain_scene, "matpbr_path_render_objects_through", False, False), (plain_scene, "matpbr_path_render_objects_ratio", True, False)]
    objects = tf.scene_objects()
    objects[1] = dict(objects[1], bsdf=dict(po.GLASS, medium={"sigma_a": (0.5, 1.0, 2.0), "scatter": 1.5, "g": 0.3}))
    med = _scene(pt, objects)
    assert med["tracer"].stats["n_medium_objects"] == 1
    cases += [(med, "matpbr_path_render_objects_diff_media", False, True), (med, "matpbr_path_render_objects_diff_media", True, True)]
    for s, old, base, media in cases:
        (code_o, *want), _ = _raw(pt, s, old, base=base, media=media, **kw)
        (code_n, *got), _ = _raw(pt, s, new, base=base, media=media, **kw)
        assert code_o == 0 and code_n == 0, (old, code_o, code_n)
        assert bool((want[-2] > 0).any()) and len(want) == (6 if base else 5)
        for k, (x, y) in enumerate(zip(want, got)):
            assert np.array_equal(_bits(x), _bits(y)), (old, base, k)


def test_existing_renders_keep_their_bits_around_a_call(pt, scene, plain_scene):
    """`render`, `render_diff` and `render_diff_through` of S's tracer give the same bits before and after the new entry ran on R; and
    on R's own tracer `render` and `render_diff`, which never see the flag, are the unflagged table's bits."""
    s, kw = plain_scene, dict(spp=4, max_depth=6, seed=2)
    before = (s["tracer"].render(*s["maps"], **kw).cpu().numpy(), _diff(s, **kw), _through(s, **kw))
    assert (_through(scene, **kw)[3] > 0).any()
    after = (s["tracer"].render(*s["maps"], **kw).cpu().numpy(), _diff(s, **kw), _through(s, **kw))
    assert np.array_equal(_u32(before[0]), _u32(after[0]))
    for x, y in zip(before[1] + before[2], after[1] + after[2]):
        assert np.array_equal(_u32(x), _u32(y))
    bare = _scene(pt, rf.scene_objects(photo=False))
    assert np.array_equal(_bits(scene["tracer"].render(*scene["maps"], **kw)), _bits(bare["tracer"].render(*bare["maps"], **kw)))
    for x, y in zip(_diff(scene, **kw), _diff(bare, **kw)):
        assert np.array_equal(_u32(x), _u32(y))
    assert np.array_equal(_bits(scene["tracer"].features()), _bits(bare["tracer"].features()))


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_photograph_enters_linearly_and_only_through_through(pt, scene):
    kw = dict(spp=3, max_depth=6, seed=4)
    one = _through(scene, **kw)
    two = _through(scene, photo=2.0 * scene["photo"], **kw)
    assert (one[3] > 0).any() and np.array_equal(two[3], 2.0 * one[3])
    for k in (0, 1, 2, 4):
        assert np.array_equal(_u32(one[k]), _u32(two[k])), k


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_untouched_tail_is_exact(pt, scene, oracle64):
    """R at max_depth 2, spp 4: every landing is cut, so no second trip runs: rewalked is 0 in every pixel with alpha = 1; through > 0
    in every pixel where the fp64 chain lands in two or more of the four samples (one flipped hit decision cannot empty it) and in at
    least 0.98 of those where it lands at all; fg is `render_diff`'s within 1e-5 relative to max(|fg|, mean |fg|), the tolerance between
    two instantiations of the kernel (there fg = L_with, here it is L_chain, the same terms)."""
    s, kw = scene, dict(spp=4, max_depth=2, seed=1)
    fg, delta, alpha, through, rewalked = _through(s, **kw)
    d_fg = _diff(s, **kw)[0].astype(np.float64)
    full = alpha == 1
    assert full.sum() >= 100 and not rewalked[full].any()
    lands = sum(((rf.chains(oracle64, s, 2, 1, sample)["k"] >= 0) & (rf.chains(oracle64, s, 2, 1, sample)["thr"] > 0).any(-1)).astype(int)
                for sample in range(4)).reshape(s["H"], s["W"])
    seen = (through > 0).any(-1)
    assert (lands >= 2).sum() >= 40 and seen[lands >= 2].all() and seen[lands >= 1].mean() >= 0.98
    rel = (np.abs(fg - d_fg) / np.maximum(np.abs(d_fg), np.abs(d_fg).mean())).max(-1)
    _report("R, max_depth 2: pixels with alpha = 1; pixels where the fp64 chain lands; worst relative difference of fg to render_diff's (bound 1e-5)",
            f"{int(full.sum())}; {int((lands >= 1).sum())}; {rel.max():.3e}")
    assert rel.max() <= 1e-5 and (d_fg[full] > 0).any()


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
WHITE_C, WHITE_RHO = 0.7, (0.6, 0.5, 0.4)
WHITE_SEEDS = range(16)


def test_a_white_object_in_a_white_room(pt):
    """A flagged diffuse cube of reflectance rho inside the groove, in front of the sheet (in fp64 0.14 of the chains of its fully
    covered pixels land on the walls, none on the sheet's back), a constant envmap c, a constant photograph c, max_depth 2, 16 seeds x
    spp 16 = 256 samples: every direction from the cube escapes to the envmap or lands on the sheet's front, so E[fg + through] = rho c
    on the fully covered pixels (one pixel in from the footprint's edge): |mean - rho c| <= 5 se + 1e-3 rho c, the form of
    `test_gpu_path_rough.py`'s furnace test.  The same cube without the flag fails the identity, the same assertion: its landings add
    nothing at max_depth 2."""
    cube = pd.cube_object(((0.0, 0.1, -2.2), 0.34, (0.4, 0.5, 0.3)), {"type": "diffuse", "reflectance": WHITE_RHO})
    inside = tl.erode(tl.footprints([cube], 20, 24)[0])
    assert inside.sum() >= 12
    want = np.asarray(WHITE_RHO) * WHITE_C
    excess = {}
    for flag in (True, False):
        s = _scene(pt, [dict(cube, photo=flag)])
        env, photo = np.full((4, 8, 3), WHITE_C, np.float32), np.full((20, 24, 3), WHITE_C, np.float32)
        vals = []
        for seed in WHITE_SEEDS:
            fg, delta, alpha, through, _ = _through(s, 16, 2, seed, photo=photo, maps=(s["a"], s["r"], s["m"], env))
            assert (alpha[inside] == 1).all()
            vals.append(fg.astype(np.float64) + through)
        vals = np.stack(vals)
        mean, se = vals.mean(0), vals.std(0, ddof=1) / math.sqrt(vals.shape[0])
        excess[flag] = (np.abs(mean - want) / (5 * se + 1e-3 * want))[inside]
        if flag:
            assert (through[inside] > 0).any()
    _report(f"white object in a white room: worst |mean - rho c| / (5 se + 1e-3 rho c) over {int(inside.sum())} pixels, flagged; the worst without the "
            f"flag; the share of the pixels that fail without it", f"{excess[True].max():.3f}; {excess[False].max():.3f}; {(excess[False] > 1.0).any(-1).mean():.3f}")
    assert excess[True].max() <= 1.0
    assert excess[False].max() > 1.0


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_bits_and_plumbing(pt, scene, light_scene):
    """Every split into launches gives the same bits; `PathTracer.render_diff_through` and `render_diff_ratio` are the raw call of the
    new entry with the flagged table; the raw entry refuses what it must with a valid call beside it."""
    new = "matpbr_path_render_objects_reflect"
    for s in (scene, light_scene):
        tracer, maps = s["tracer"], s["maps"]
        photo = torch.from_numpy(s["photo"]).to(tracer.device)
        kw = dict(spp=6, max_depth=8, seed=7)
        whole = tracer.render_diff_through(*maps, photo, spp_per_launch=6, **kw)
        for split in (1, 4):
            part = tracer.render_diff_through(*maps, photo, spp_per_launch=split, **kw)
            for k, (x, y) in enumerate(zip(whole, part)):
                assert np.array_equal(_bits(x), _bits(y)), (split, k)
        (code, *got), (args, outs) = _raw(pt, s, new, flag=True, **kw)
        assert code == 0
        for k, (x, y) in enumerate(zip(whole, got)):
            assert np.array_equal(_bits(x), _bits(y)), k
        ratio = tracer.render_diff_ratio(*maps, photo=photo, **kw)
        (code, *got), _ = _raw(pt, s, new, base=True, flag=True, **kw)
        assert code == 0 and len(ratio) == 6
        for k, (x, y) in enumerate(zip(ratio, got)):
            assert np.array_equal(_bits(x), _bits(y)), k
        for k, j in ((0, 0), (1, 1), (3, 3), (4, 4), (5, 5)):                       # the ratio shape adds base and leaves the rest
            assert np.array_equal(_bits(ratio[k]), _bits(whole[j if j < 2 else j - 1])), k
        fn = pt.symbol(new)
        for k in (0, 1, 2, 4, 5):                                                    # refused: a missing buffer (photo and through among them)
            ptrs = list(outs)
            ptrs[k] = None
            assert fn(*args, *ptrs) == -1, k
        assert fn(*args, *outs[:3], None, *outs[4:]) == 0                            # rewalked is nullable
        table = list(tracer.objects)
        for k, t in enumerate(table):                                                # the flag on kind 1 or 4
            if t.kind & 0xff in (pt.BSDF_DIELECTRIC, pt.BSDF_AREA):
                bad = (pt.PathObject * len(table))(*(pt.PathObject(u.kind | pt.OBJECT_PHOTO if j == k else u.kind, u.first_tri, u.n_tri, u.p)
                                                      for j, u in enumerate(table)))
                import ctypes

                assert fn(*args[:20], ctypes.cast(bad, ctypes.c_void_p), *args[21:], *outs) == -1, k
        for old in ("matpbr_path_render_objects_through", "matpbr_path_render_objects_diff_media"):   # and the raw entries from before it
            (code, *_), _ = _raw(pt, s, old, flag=True, **kw)
            assert code == -1, old
        torch.cuda.synchronize()


def test_rewalked_and_rays_count_both_kinds(pt, scene):
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
    _report("R, spp 5: rays of the render; of the flagged differential render; second walks", f"{r1}; {r2}; {n2}")
    assert 0.99 * r1 + n2 <= r2 <= 1.01 * r1 + 2 * max_depth * n2


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_it_helps_where_the_fit_is_off(pt):
    """The groove with R's chrome sphere alone.  The photograph is a spp-256 `render` of the scene alone under the maps with metallic 0;
    the truth a spp-256 `render` with the sphere under the same maps; "the fit" has the albedo halved.  Over the sphere's fully covered
    pixels the composite's mean absolute error against the truth, per seed of 8 (spp 128, max_depth 4), is smaller with the flag than
    without it by more than 5 standard errors of the difference."""
    on, off = _scene(pt, [rf.chrome_sphere(True)]), _scene(pt, [rf.chrome_sphere(False)])
    a, r, env = on["a"], on["r"], on["env"]
    m = np.zeros_like(on["m"])
    alone = pt.PathTracer(on["rm"]["vertices"], on["rm"]["triangles"], on["H"], on["W"], FOV)
    photo = alone.render(a, r, m, env, spp=256, max_depth=4, seed=100)
    truth = on["tracer"].render(a, r, m, env, spp=256, max_depth=4, seed=101).cpu().numpy().astype(np.float64)
    inside = tl.footprints([rf.chrome_sphere()], on["H"], on["W"])[0]
    assert inside.sum() >= 60
    errs = {True: [], False: []}
    for seed in range(8):
        for flag, s in ((True, on), (False, off)):
            fg, delta, alpha, through, _ = s["tracer"].render_diff_through(0.5 * a, r, m, env, photo, spp=128, max_depth=4, seed=seed)
            img = pt.composite(fg + through, delta, alpha, photo).cpu().numpy().astype(np.float64)
            errs[flag].append(np.abs(img - truth)[inside].mean())
    gain = np.asarray(errs[False]) - np.asarray(errs[True])
    se = gain.std(ddof=1) / math.sqrt(gain.size)
    _report("the fit's albedo halved, chrome sphere: mean absolute error over its covered pixels without the flag; with it; the gain in standard errors",
            f"{np.mean(errs[False]):.4f}; {np.mean(errs[True]):.4f}; {gain.mean() / se:.1f}")
    assert gain.mean() > 5 * se and gain.mean() > 0


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------------
CLI_CUBE = ((0.02, 0.0, -0.9), 0.2, (0.4, 0.5, 0.3))
CLI_SLIDE = (0.05, 0.0, 0.0)


@pytest.mark.parametrize("extra", [[], ["--oi_composite_denoise"], ["--oi_shadows", "ratio"], ["--oi_frames", "2"]], ids=["plain", "denoise", "ratio", "frames"])
def test_render_final_cli_reflect_photo(pt, tmp_path, extra):
    """`render_final.py --mode oi --oi_scene ... --oi_composite --oi_reflect_photo` (its `main`, in this process) on
    `path_testlib.synthetic_output` with one frosted-glass cube whose entry carries a "motion", against the same command with
    `--oi_see_through` in the option's place (the same code path without the flag): the files exist, are finite and >= 0, differ from
    the unflagged run, and only inside the cube's footprint dilated by a pixel (of both poses, for the two frames); the pixels the
    unflagged run leaves at the photograph's bits keep them."""
    import render_final
    from materialist_amd import mesh
    from materialist_amd.imageio_exr import read_exr, write_exr
    from PIL import Image

    tmp = str(tmp_path)
    tl.synthetic_output(tmp)
    photo = np.random.default_rng(4).gamma(2.0, 0.3, (32, 32, 3)).astype(np.float32)
    write_exr(os.path.join(tmp, "case", "gt_image.exr"), photo)
    ob = pd.cube_object(CLI_CUBE, rf.FROSTED)
    os.makedirs(os.path.join(tmp, "lists"))
    mesh.write_ply(os.path.join(tmp, "lists", "cube.ply"), ob["vertices"].astype(np.float32), ob["triangles"])
    listing = os.path.join(tmp, "lists", "cube.json")
    with open(listing, "w") as f:
        json.dump({"objects": [{"ply": "cube.ply", "bsdf": rf.FROSTED, "motion": {"slide": list(CLI_SLIDE)}}]}, f)
    frames = "--oi_frames" in extra
    argv = ["--save_name", "case", "--input_path", tmp, "--save_path", tmp, "--mode", "oi", "--spp", "4", "--oi_iters", "2", "--oi_max_depth", "6",
            "--oi_composite", "--oi_scene", listing, *extra]
    names = [os.path.join(tmp, "case", "oi_animation", f"frame_{f:04d}.png") for f in range(2)] if frames else [os.path.join(tmp, "case", "mi_oic_case_envmap.exr")]

    def run(option):
        for name in names:
            if os.path.exists(name):
                os.remove(name)
        render_final.main(argv + [option])
        out = []
        for name in names:
            assert os.path.isfile(name), name
            img = np.asarray(Image.open(name).convert("RGB")) if frames else np.ascontiguousarray(read_exr(name)[..., :3], dtype=np.float32)
            assert np.isfinite(img.astype(np.float64)).all() and (img >= 0).all()
            out.append(img)
        return out

    plain, seen = run("--oi_see_through"), run("--oi_reflect_photo")
    moved = dict(ob, vertices=ob["vertices"] + np.asarray(CLI_SLIDE))
    outside = tl.footprints([ob, moved] if frames else [ob], 32, 32)[1]
    assert outside.sum() >= 100
    for x, y in zip(plain, seen):
        changed = (x != y).any(-1)
        assert changed.any() and not changed[outside].any()
    if frames:
        assert os.path.isfile(os.path.join(tmp, "case", "mi_oic_case_envmap.mp4")) and os.path.isfile(os.path.join(tmp, "case", "mi_oic_case_envmap.gif"))
        return
    kept = (plain[0].view(np.uint32) == photo.view(np.uint32)).all(-1)
    _report(f"render_final.py --oi_reflect_photo {' '.join(extra)}: pixels that differ from the unflagged run; pixels at the photograph's bits without the flag",
            f"{int((plain[0] != seen[0]).any(-1).sum())}; {int(kept.sum())}")
    assert kept.sum() >= 10 and np.array_equal(seen[0].view(np.uint32)[kept], photo.view(np.uint32)[kept])
