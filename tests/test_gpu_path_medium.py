"""Media inside glass objects on the GPU (libmatpbr_path.so's `matpbr_path_render_objects_media` and
`matpbr_path_render_objects_diff_media`, DESIGN.md section 1.4, "Media inside glass"): every path of a table with a tinted clear
sphere and a cloudy rough-glass cube around a lamp against the fp64 restatement, bits (launch splits, the raw calls, an all-zero
record, every earlier level's table through level 8), Beer-Lambert's law and the white furnace against their analytic values, the
differential family with a medium, and `render_final.py --mode oi --oi_scene` with a "medium"."""
import json
import math
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

import path_color_fp64 as pc  # noqa: E402
import path_diff_fp64 as pd  # noqa: E402
import path_fp64 as pf  # noqa: E402
import path_light_fp64 as pl  # noqa: E402
import path_medium_fp64 as pm  # noqa: E402
import path_oi_fp64 as po  # noqa: E402
import path_oi_pbr_fp64 as pp  # noqa: E402
import path_oi_smooth_fp64 as ps  # noqa: E402
import path_rough_fp64 as pr  # noqa: E402
import path_testlib as tl  # noqa: E402
import path_texture_fp64 as ptx  # noqa: E402
import path_through_fp64 as tf  # noqa: E402
from path_testlib import bits as _bits, parity as _parity, raw_args as _raw_args  # noqa: E402

pytestmark = pytest.mark.gpu

FOV = pf.FOV
SEEDS = list(range(100, 164))      # the 64 fixed seeds of the scenes in expectation
MATCHED = {"type": "dielectric", "int_ior": 1.5, "ext_ior": 1.5}
SPHERE = ((0.02, -0.01, -1.2), 0.2)                                # centre, radius R: `path_rough_fp64.FURNACE_SPHERE`
ENV_C = (0.7, 0.5, 0.9)
_report = tl.reporter("path medium", "test_gpu_path_medium")


@pytest.fixture(scope="module")
def pt():
    return tl.load(gpu=True)


@pytest.fixture(scope="module")
def scene(pt):
    """The groove at 24 x 20 (a partial tile) with `path_medium_fp64.table_scene` in front of it: a smooth-flagged tinted clear sphere,
    a cloudy rough-glass cube around a small emitter quad, a diffuse cube."""
    s = tl.groove_with_objects(pt, pm.table_scene(), pm.merged)
    st = s["tracer"].stats
    assert st["n_objects"] == 4 and st["n_medium_objects"] == 2 and st["n_rough_objects"] == 1 and st["n_lights"] == 1 and st["n_smooth_objects"] == 1
    assert s["tracer"].media is not None and len(s["tracer"].media) == 4
    return s


def _media_tail(tracer):
    """The object arguments of the level-8 entry after `stream`."""
    return (*tracer.object_args()[:9], *tracer._texture_args(), tracer.media_arg())


def _sphere(medium, bsdf=MATCHED, levels=2):
    V, T, _ = ps.icosphere(*SPHERE, levels)
    V = V.astype(np.float32).astype(np.float64)
    return {"vertices": V, "triangles": T, "bsdf": dict(bsdf, medium=medium) if medium is not None else dict(bsdf)}


def _u32(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_every_path_matches_the_fp64_restatement(pt, scene, oracle64):
    """At least 0.99 of the pixels within 1e-3 at spp 1 (`path_testlib.parity`, rough glass's criterion; on the CPU the restatement over
    the library's fp32 traversal and over the fp64 brute force meets it on these renders, test_path_medium_host.py).  Across the nine
    renders every kind of path through a medium occurs."""
    s = scene
    H, W = s["H"], s["W"]
    tab = pt.env_tables(s["env"])
    seen = {k: 0 for k in pm.RECORD_KEYS}
    for max_depth in (2, 6, 16):
        for seed in (0, 1, 2):
            got = s["tracer"].render(s["a"], s["r"], s["m"], s["env"], spp=1, max_depth=max_depth, seed=seed).cpu().numpy().astype(np.float64)
            assert np.isfinite(got).all()
            ref, rec = pm.replay_medium(oracle64, s["V"], s["T"], s["a"], s["r"], s["m"], s["env"], tab, H, W, max_depth, seed, s["table"])
            frac, err = _parity(got, ref)
            _report(f"per-path parity with media, max_depth {max_depth} seed {seed}: share of pixels within 1e-3",
                    f"{frac:.4f} ({int((err > 1e-3).sum())} flipped paths, max err {err.max():.3e})")
            assert frac >= 0.99, (max_depth, seed, frac, np.argwhere(err > 1e-3)[:10])
            for k in pm.RECORD_KEYS:
                seen[k] += int(rec[k].sum())
    _report("pixels with " + " / ".join(pm.RECORD_KEYS) + " (9 renders)", " / ".join(str(seen[k]) for k in pm.RECORD_KEYS))
    assert all(seen[k] > 0 for k in pm.RECORD_KEYS), seen


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_bits(pt, scene):
    s = scene
    maps = (s["a"], s["r"], s["m"], s["env"])
    H, W, rm = s["H"], s["W"], s["rm"]
    media, textures = pt.symbol("matpbr_path_render_objects_media"), pt.symbol("matpbr_path_render_objects_textures")
    # every split of a frame into launches gives the same bits
    whole = s["tracer"].render(*maps, spp=6, max_depth=16, seed=7, spp_per_launch=6)
    for split in (1, 3, 4):
        assert np.array_equal(_bits(whole), _bits(s["tracer"].render(*maps, spp=6, max_depth=16, seed=7, spp_per_launch=split))), split
    # PathTracer.render with a medium is the raw level-8 call
    out = torch.empty(H, W, 3, device=s["tracer"].device)
    keep, args = _raw_args(s["tracer"], maps, 6, 16, 5, 4, out)
    assert media(*args, *_media_tail(s["tracer"])) == 0
    assert np.array_equal(_bits(s["tracer"].render(*maps, spp=6, max_depth=16, seed=5, spp_per_launch=4)), _bits(out))
    # level 7 refuses the flagged table
    assert textures(*args, *_media_tail(s["tracer"])[:13]) == -1
    # a flagged object whose record is all zero: the bits of the unflagged table through level 7
    zero = [dict(ob, bsdf=dict(ob["bsdf"], medium={})) if "medium" in ob["bsdf"] else ob for ob in pm.table_scene()]
    bare = [dict(ob, bsdf={k: v for k, v in ob["bsdf"].items() if k != "medium"}) for ob in pm.table_scene()]
    tz = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV, objects=zero)
    tb = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV, objects=bare)
    assert tz.stats["n_medium_objects"] == 2 and tb.stats["n_medium_objects"] == 0 and tb.media is None
    ref = torch.empty(H, W, 3, device=tb.device)
    keep2, args2 = _raw_args(tb, maps, 6, 16, 5, 4, ref)
    assert textures(*args2, *_media_tail(tb)[:13]) == 0
    assert np.array_equal(_bits(tz.render(*maps, spp=6, max_depth=16, seed=5, spp_per_launch=4)), _bits(ref))
    assert np.array_equal(_bits(tb.render(*maps, spp=6, max_depth=16, seed=5, spp_per_launch=4)), _bits(ref))
    assert not np.array_equal(_bits(out), _bits(ref))                       # and the media of the scene do change the picture

    def through_level_8(objects):
        """`render` of a tracer without a medium, whatever route it takes: the bits of level 8 called raw, with and without records."""
        tracer = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV, objects=objects)
        assert tracer.media is None and tracer.stats["n_medium_objects"] == 0
        want = tracer.render(*maps, spp=6, max_depth=16, seed=5, spp_per_launch=4)
        got = torch.empty(H, W, 3, device=tracer.device)
        keep3, args3 = _raw_args(tracer, maps, 6, 16, 5, 4, got)
        assert media(*args3, *_media_tail(tracer)) == 0
        assert np.array_equal(_bits(got), _bits(want))
        if objects:
            records = (pt.PathObjectMedium * len(objects))()
            assert media(*args3, *_media_tail(tracer)[:13], pt._ref(records)) == 0
            assert np.array_equal(_bits(got), _bits(want))

    for objects in (po.two_cubes(), ps.table_scene(), pp.table_scene(), pl.table_scene(), pr.table_scene(), pc.table_scene(), ptx.table_scene(), None):
        through_level_8(objects)


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------------
def _far(pt, objects, H=10, W=12):
    Vs, Ts = pp.FAR_TRIANGLE
    tracer = pt.PathTracer(Vs, Ts, H, W, FOV, objects=objects)
    maps = (np.zeros((H, W, 3), np.float32), np.ones((H, W, 1), np.float32), np.zeros((H, W, 1), np.float32))
    env = np.tile(np.float32(ENV_C), (16, 32, 1))
    return tracer, maps, env


def test_beer_lambert(pt):
    """An index-matched icosphere (int_ior = ext_ior: the ray goes straight through) with sigma_a = (0.5, 1, 2) / R and no scattering
    in a constant envmap c over a depth mesh no ray meets, 12 x 10, spp 1: every pixel is c exp(-sigma_a l) in fp64, l the chord of
    that sample's camera ray through the mesh by brute force (`path_medium_fp64.chords`); `path_testlib.parity`'s criterion, test 6's.
    A pixel whose ray misses the mesh is c exactly."""
    R = SPHERE[1]
    sa = np.float32([0.5 / R, 1.0 / R, 2.0 / R])
    ob = _sphere({"sigma_a": [float(x) for x in sa]})
    H, W = 10, 12
    tracer, maps, env = _far(pt, [ob], H, W)
    assert tracer.stats["n_medium_objects"] == 1
    c = np.float32(ENV_C)
    for seed in (0, 1, 2):
        got = tracer.render(*maps, env, spp=1, max_depth=16, seed=seed).cpu().numpy()
        o, d = pd.camera_rays(H, W, seed, 0)
        length, n = pm.chords(ob["vertices"], ob["triangles"], o, d)
        assert set(np.unique(n)) <= {0, 2} and (n == 2).sum() >= 20 and (n == 0).sum() >= 20
        ref = (c.astype(np.float64)[None, :] * np.exp(-sa.astype(np.float64)[None, :] * length[:, None])).reshape(H, W, 3)
        frac, err = _parity(got.astype(np.float64), ref)
        _report(f"Beer-Lambert, seed {seed}: share of pixels within 1e-3; longest chord / R", f"{frac:.4f} (max err {err.max():.3e}); {length.max() / R:.3f}")
        assert frac >= 0.99, (seed, frac, np.argwhere(err > 1e-3)[:10])
        miss = (n == 0).reshape(H, W)
        assert np.array_equal(_u32(got[miss]), _u32(np.broadcast_to(c, got[miss].shape)))
        assert (got[~miss] < c).all()


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [0.0, 0.7])
def test_white_furnace(pt, g):
    """The same sphere with sigma_a = 0 and sigma_s 2 R = 0.5 in the constant envmap c, 64 seeds x spp 16, max_depth 16: no vertex
    changes the throughput but by roundings (16 vertices of weights within a few ulp of 1), so every covered pixel is at most
    c (1 + 1e-5), and a path loses its energy only where max_depth cuts it, so the covered mean is at least c (1 - 1e-5 - q), q the
    probability of 14 scatterings or more (the boundary's two vertices and 13 scatterings end at depth 15) from the Poisson law of
    the scatter count on the longest chord, mean sigma_s 2 R = 0.5: below 1e-15."""
    R = SPHERE[1]
    ob = _sphere({"scatter": 0.5 / (2.0 * R), "g": g})
    H, W = 10, 12
    tracer, maps, env = _far(pt, [ob], H, W)
    tabs = tracer.tables(env)
    vals = np.stack([tracer.render(*maps, env, spp=16, max_depth=16, seed=sd, spp_per_launch=16, tables=tabs).cpu().numpy() for sd in SEEDS]).astype(np.float64)
    assert np.isfinite(vals).all()
    lam = 0.5
    q = sum(math.exp(-lam) * lam ** n / math.factorial(n) for n in range(14, 80))
    assert q < 1e-15
    inside, _ = tl.footprints([ob], H, W)
    assert inside.sum() >= 12
    c = np.float64(np.float32(ENV_C))
    cov = vals[:, inside]
    _report(f"white furnace g = {g}: covered pixels; max and mean of value / c - 1 over them (bounds +1e-5, -1e-5 - q)",
            f"{int(inside.sum())}; {(cov / c - 1).max():+.3e} {(cov.mean((0, 1)) / c - 1).min():+.3e}")
    assert (cov <= c * (1.0 + 1e-5)).all()
    assert (cov.mean((0, 1)) >= c * (1.0 - 1e-5 - q)).all()
    rays = torch.zeros(H, W, dtype=torch.int32, device=tracer.device)     # and the medium does scatter: more rays than the three of a straight passage
    tracer.render(*maps, env, spp=16, max_depth=16, seed=1, spp_per_launch=16, tables=tabs, rays=rays)
    assert int(rays.cpu().numpy()[inside].max()) > 3 * 16


# ---- 10 --------------------------------------------------------------------------------------------------------------------------------
def _diff_scene(pt, objects):
    s = tl.groove_with_objects(pt, objects, pm.merged)
    s["n_scene"] = s["rm"]["triangles"].shape[0]
    s["tab"] = pt.env_tables(s["env"])
    s["maps"] = (s["a"], s["r"], s["m"], s["env"])
    s["photo"] = tf.photograph(s["H"], s["W"])
    return s


def test_the_composite(pt, oracle64):
    """The differential family with the tinted index-matched sphere in front of the groove: `through` per path against fp64, the bits of
    an all-zero record, the launch splits, `render_diff_ratio` against the superset entry called raw, and the sphere hidden behind the
    scene, where the composite is the photograph bit for bit."""
    R = SPHERE[1]
    sa = np.float32([0.5 / R, 1.0 / R, 2.0 / R])
    tint = {"sigma_a": [float(x) for x in sa]}
    s = _diff_scene(pt, [_sphere(tint)])
    H, W, tracer = s["H"], s["W"], s["tracer"]
    ob = s["objects"][0]
    photo = torch.from_numpy(s["photo"]).to(tracer.device)
    # through at spp 1 against exp(-sigma_a l) photo[texel] at the landing of the fp64 chain; l is what the chain flies inside the mesh:
    # from the point it spawns at, spawn_eps inside the face the camera ray enters by, to its next hit (brute force)
    P = ob["vertices"][ob["triangles"]]
    for seed in (0, 1, 2):
        fg, delta, alpha, through, rewalked = (x.cpu().numpy() for x in tracer.render_diff_through(*s["maps"], photo, spp=1, max_depth=16, seed=seed))
        ch = tf.chains(oracle64, s, 16, seed, 0)
        o, d = pd.camera_rays(H, W, seed, 0)
        _, n = pm.chords(ob["vertices"], ob["triangles"], o, d)
        see = ch["k"] >= 0
        assert see.sum() >= 60 and (n[see] == 2).all()
        t0, k0 = pf.brute(P, o, d)
        hit = k0 >= 0
        kk = np.where(hit, k0, 0)
        ng = np.cross(P[kk, 1] - P[kk, 0], P[kk, 2] - P[kk, 0])
        ng /= np.linalg.norm(ng, axis=-1, keepdims=True)
        p0 = o + np.where(hit, t0, 0.0)[:, None] * d
        length = np.zeros(H * W)
        length[hit] = pf.brute(P, (p0 - (1e-5 * (1 + np.abs(p0).max(-1)))[:, None] * ng)[hit], d[hit])[0]
        assert np.isfinite(length[see]).all() and (length[see] > 0).all()
        ref = np.where(see[:, None], ch["thr"].reshape(-1, 1) * np.exp(-sa.astype(np.float64)[None, :] * length[:, None]) *
                       s["photo"].reshape(-1, 3).astype(np.float64)[np.where(see, ch["q"], 0)], 0.0).reshape(H, W, 3)
        frac, err = _parity(through.astype(np.float64), ref)
        _report(f"through with a tinted sphere, seed {seed}: share of pixels within 1e-3; see-through lanes", f"{frac:.4f} (max err {err.max():.3e}); {int(see.sum())}")
        assert frac >= 0.99, (seed, frac, np.argwhere(err > 1e-3)[:10])
        assert (alpha.reshape(-1) == ch["covered"]).mean() >= 0.99 and np.isfinite(fg).all() and np.isfinite(delta).all()
    # an all-zero record: the bits of the unflagged table, in all three renders
    tz = pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], H, W, FOV, objects=[_sphere({})])
    tb = pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], H, W, FOV, objects=[_sphere(None)])
    assert tz.media is not None and tb.media is None
    kw = dict(spp=6, max_depth=16, seed=5, spp_per_launch=4)
    for call, own in (("render_diff_through", (photo,)), ("render_diff", ()), ("render_diff_ratio", ())):
        for k, (x, y) in enumerate(zip(getattr(tz, call)(*s["maps"], *own, **kw), getattr(tb, call)(*s["maps"], *own, **kw))):
            assert np.array_equal(_bits(x), _bits(y)), (call, k)
    # every split into launches gives the same bits, and the tint changes `through` and nothing the glass does not touch
    whole = tracer.render_diff_through(*s["maps"], photo, spp=6, max_depth=16, seed=5, spp_per_launch=6)
    for split in (1, 4):
        for k, (x, y) in enumerate(zip(whole, tracer.render_diff_through(*s["maps"], photo, spp=6, max_depth=16, seed=5, spp_per_launch=split))):
            assert np.array_equal(_bits(x), _bits(y)), (split, k)
    clear = tb.render_diff_through(*s["maps"], photo, spp=6, max_depth=16, seed=5, spp_per_launch=6)
    assert np.array_equal(_bits(whole[2]), _bits(clear[2])) and not np.array_equal(_bits(whole[3]), _bits(clear[3]))
    assert bool((whole[3] <= clear[3]).all())
    # render_diff_ratio with base is the superset entry called raw
    fn = pt.symbol("matpbr_path_render_objects_diff_media")
    for with_photo in (False, True):
        got = tracer.render_diff_ratio(*s["maps"], photo=photo if with_photo else None, **kw)
        dev = tracer.device
        fg, delta, base, through = (torch.full((H, W, 3), v, device=dev) for v in (7.0, -7.0, 3.0, 5.0))
        alpha, rewalked = torch.full((H, W), 7.0, device=dev), torch.zeros(H, W, dtype=torch.int32, device=dev)
        keep = tracer._inputs(*s["maps"], None)
        args = (*tracer._frame(*keep, 6, 16, 5, 4), None, torch.cuda.current_stream().cuda_stream, *tracer.object_args()[:9], *tracer._texture_args())
        assert fn(*args, fg.data_ptr(), delta.data_ptr(), alpha.data_ptr(), rewalked.data_ptr(), photo.data_ptr() if with_photo else None,
                  through.data_ptr() if with_photo else None, base.data_ptr(), tracer.media_arg()) == 0
        raw = (fg, delta, base, alpha, through, rewalked) if with_photo else (fg, delta, base, alpha, rewalked)
        assert len(got) == len(raw)
        for k, (x, y) in enumerate(zip(got, raw)):
            assert np.array_equal(_bits(x), _bits(y)), (with_photo, k)
    # the object hidden behind the scene: every output zero, and the composite is the photograph bit for bit
    hid = dict(_sphere(tint), vertices=_sphere(tint)["vertices"] + np.array([0.0, 0.0, -4.8]))
    h = _diff_scene(pt, [hid])
    assert h["tracer"].media is not None
    assert not pd.any_path_returns_object(oracle64, h, h["tab"], 16, range(2), 1)
    for seed in range(2):
        out = h["tracer"].render_diff_through(*h["maps"], photo, spp=4, max_depth=16, seed=seed, spp_per_launch=3)
        for x in out:
            assert not bool(x.view(torch.int32).any()), seed
        fg, delta, alpha, through, _ = out
        assert np.array_equal(_bits(pt.composite(fg + through, delta, alpha, photo)), s["photo"].view(np.uint32))


# ---- 11 --------------------------------------------------------------------------------------------------------------------------------
def test_render_final_cli_medium(pt, tmp_path):
    """`render_final.py --mode oi --oi_scene glass.json` with a "medium" on its one glass cube, once plain and once with --oi_composite
    --oi_see_through: both exit 0 and write finite images that differ from the same command's without the key."""
    from materialist_amd import mesh
    from materialist_amd.imageio_exr import read_exr, write_exr

    tmp = str(tmp_path)
    scene_dir = tl.synthetic_output(tmp)
    write_exr(os.path.join(scene_dir, "gt_image.exr"), np.random.default_rng(4).gamma(2.0, 0.3, (32, 32, 3)).astype(np.float32))
    ob = pd.cube_object(((0.02, 0.0, -0.9), 0.2, (0.4, 0.5, 0.3)), po.GLASS)
    os.makedirs(os.path.join(tmp, "lists"))
    mesh.write_ply(os.path.join(tmp, "lists", "glass.ply"), ob["vertices"].astype(np.float32), ob["triangles"])
    listings = {}
    for name, extra in (("clear", {}), ("tinted", {"medium": {"color": [0.9, 0.4, 0.1], "at": 0.2, "scatter": 2.0, "g": 0.3}})):
        listings[name] = os.path.join(tmp, "lists", name + ".json")
        with open(listings[name], "w") as f:
            json.dump({"objects": [dict({"ply": "glass.ply", "bsdf": po.GLASS}, **extra)]}, f)
    cmd = [sys.executable, os.path.join(ROOT, "render_final.py"), "--save_name", "case", "--input_path", tmp, "--save_path", tmp, "--mode", "oi",
           "--spp", "4", "--oi_iters", "2", "--oi_max_depth", "8"]

    def run(name, extra, exr):
        path = os.path.join(tmp, "case", exr)
        if os.path.exists(path):
            os.remove(path)
        res = subprocess.run(cmd + ["--oi_scene", listings[name]] + extra, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout + res.stderr
        img = np.ascontiguousarray(read_exr(path)[..., :3], dtype=np.float32)
        assert np.isfinite(img).all() and (img >= 0).all() and float(img.std()) > 0
        return img

    inside, _ = tl.footprints([ob], 32, 32)
    for extra, exr in (([], "mi_oi_case_envmap.exr"), (["--oi_composite", "--oi_see_through"], "mi_oic_case_envmap.exr")):
        clear, tinted = run("clear", extra, exr), run("tinted", extra, exr)
        assert inside.sum() >= 9 and (clear != tinted).any(-1)[inside].mean() > 0.9, extra


def test_render_final_cli_tint_route(pt, tmp_path):
    """`render_final.py --mode oi --oi_tint r g b` tints <scene>/oi.ply, the default route's glass (the distance defaults to the largest
    side of its bounding box): a finite image that differs, inside the glass's footprint, from the same command's without the option."""
    from materialist_amd import mesh
    from materialist_amd.imageio_exr import read_exr

    tmp = str(tmp_path)
    scene_dir = tl.synthetic_output(tmp)
    ob = pd.cube_object(((0.02, 0.0, -0.9), 0.2, (0.4, 0.5, 0.3)), po.GLASS)
    mesh.write_ply(os.path.join(scene_dir, "oi.ply"), ob["vertices"].astype(np.float32), ob["triangles"])
    cmd = [sys.executable, os.path.join(ROOT, "render_final.py"), "--save_name", "case", "--input_path", tmp, "--save_path", tmp, "--mode", "oi",
           "--spp", "4", "--oi_iters", "2", "--oi_max_depth", "8"]
    exr = os.path.join(tmp, "case", "mi_oi_case_envmap.exr")
    imgs = []
    for extra in ([], ["--oi_tint", "0.9", "0.4", "0.1"]):
        if os.path.exists(exr):
            os.remove(exr)
        res = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout + res.stderr
        imgs.append(np.ascontiguousarray(read_exr(exr)[..., :3], dtype=np.float32))
        assert np.isfinite(imgs[-1]).all() and (imgs[-1] >= 0).all()
    inside, _ = tl.footprints([ob], 32, 32)
    assert inside.sum() >= 9 and (imgs[0] != imgs[1]).any(-1)[inside].mean() > 0.9


def test_render_final_cli_medium_with_the_other_options(pt, tmp_path):
    """A "medium" in the object list beside the options it has to work with: the ratio composite with its denoiser and the photograph
    seen through the glass, the plain render's denoiser, and a two-frame video of the spinning object.  Each exits 0 and writes a
    finite picture."""
    from materialist_amd import mesh
    from materialist_amd.imageio_exr import read_exr, write_exr

    tmp = str(tmp_path)
    scene_dir = tl.synthetic_output(tmp)
    write_exr(os.path.join(scene_dir, "gt_image.exr"), np.random.default_rng(4).gamma(2.0, 0.3, (32, 32, 3)).astype(np.float32))
    ob = pd.cube_object(((0.02, 0.0, -0.9), 0.2, (0.4, 0.5, 0.3)), po.GLASS)
    os.makedirs(os.path.join(tmp, "lists"))
    mesh.write_ply(os.path.join(tmp, "lists", "glass.ply"), ob["vertices"].astype(np.float32), ob["triangles"])
    listing = os.path.join(tmp, "lists", "tinted.json")
    with open(listing, "w") as f:
        json.dump({"objects": [{"ply": "glass.ply", "bsdf": po.GLASS, "medium": {"sigma_a": [1.0, 4.0, 9.0], "scatter": 3.0, "g": -0.3},
                                "motion": {"spin": {"axis": [0, 1, 0], "deg_per_frame": 20}}}]}, f)
    cmd = [sys.executable, os.path.join(ROOT, "render_final.py"), "--save_name", "case", "--input_path", tmp, "--save_path", tmp, "--mode", "oi",
           "--spp", "4", "--oi_iters", "1", "--oi_max_depth", "8", "--oi_scene", listing]
    for extra, name in ((["--oi_composite", "--oi_shadows", "ratio", "--oi_composite_denoise", "--oi_see_through"], "mi_oic_case_envmap.exr"),
                        (["--denoise", "atrous"], "mi_oi_case_envmap.exr"), (["--oi_frames", "2"], None)):
        res = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, (extra, res.stdout + res.stderr)
        if name is None:
            assert os.path.exists(os.path.join(tmp, "case", "oi_animation", "frame_0001.png"))
        else:
            img = np.ascontiguousarray(read_exr(os.path.join(tmp, "case", name))[..., :3], dtype=np.float32)
            assert np.isfinite(img).all() and (img >= 0).all() and float(img.std()) > 0
