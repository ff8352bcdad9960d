"""Rough dielectric inserted objects on the GPU (libmatpbr_path.so's `matpbr_path_render_objects_rough`, DESIGN.md section 1.4, "Rough
dielectric objects"): every path of a table with two rough-glass objects, a light inside one of them and every other transparent kind
against the fp64 restatement, bits (launch splits, a table without rough objects, the routes `render` took before), the two scenes of
tests/test_path_rough_host.py in expectation on the device, the features of a rough object, and `render_final.py --mode oi
--oi_scene globe.json` with and without the denoiser."""
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

import path_fp64 as pf  # noqa: E402
import path_light_fp64 as pl  # noqa: E402
import path_objects_fp64 as pob  # noqa: E402
import path_oi_fp64 as po  # noqa: E402
import path_oi_pbr_fp64 as pp  # noqa: E402
import path_oi_smooth_fp64 as ps  # noqa: E402
import path_rough_fp64 as pr  # noqa: E402
import path_testlib as tl  # noqa: E402
from path_testlib import bits as _bits, parity as _parity, raw_args as _raw_args  # noqa: E402

pytestmark = pytest.mark.gpu

FOV = pf.FOV
SEEDS = list(range(100, 164))      # the 64 fixed seeds of the scenes in expectation (tests/test_path_rough_host.py)


@pytest.fixture(scope="module")
def pt():
    return tl.load(gpu=True)


_report = tl.reporter("path rough", "test_gpu_path_rough")


@pytest.fixture(scope="module")
def scene(pt):
    """The groove at 24 x 20 (a partial tile) with `path_rough_fp64.table_scene` in front of it: a smooth-flagged rough-glass
    icosphere (alpha 0.2), a flat rough-glass cube (alpha 0.05) around a small emitter quad, a diffuse cube, a clear-glass icosphere."""
    s = tl.groove_with_objects(pt, pr.table_scene(), pob.merged)
    st = s["tracer"].stats
    assert st["n_objects"] == 5 and st["n_rough_objects"] == 2 and st["n_lights"] == 1 and st["n_smooth_objects"] == 2
    assert s["tracer"].rough and s["tracer"].lights is not None
    return s


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_on", [True, False])
def test_every_path_matches_the_fp64_restatement(pt, scene, oracle64, env_on):
    """At least 0.99 of the pixels within 1e-3 at spp 1 (`path_testlib.parity`; on the CPU the restatement over the library's fp32
    traversal and over the fp64 brute force disagrees in no pixel of these renders, test_path_rough_host.py), with the envmap on
    (n_e = 2) and zero (n_e = 1: the lamp inside the cube alone).  Across the nine renders every kind of rough-glass path occurs."""
    s = scene
    H, W = s["H"], s["W"]
    env = s["env"] if env_on else np.zeros_like(s["env"])
    tab = pt.env_tables(env)
    seen = {k: 0 for k in pr.RECORD_KEYS}
    for max_depth in (2, 6, 16):
        for seed in (0, 1, 2):
            got = s["tracer"].render(s["a"], s["r"], s["m"], env, spp=1, max_depth=max_depth, seed=seed).cpu().numpy().astype(np.float64)
            assert np.isfinite(got).all()
            ref, rec = pob.replay_objects(oracle64, s["V"], s["T"], s["a"], s["r"], s["m"], env, tab, H, W, max_depth, seed, s["table"])
            assert rec["n_e"] == 1 + env_on
            frac, err = _parity(got, ref)
            _report(f"per-path parity with rough glass, envmap {'on' if env_on else 'zero'}, max_depth {max_depth} seed {seed}: share of pixels within 1e-3",
                    f"{frac:.4f} ({int((err > 1e-3).sum())} flipped paths, max err {err.max():.3e})")
            assert frac >= 0.99, (max_depth, seed, frac, np.argwhere(err > 1e-3)[:10])
            for k in pr.RECORD_KEYS:
                seen[k] += int(rec[k].sum())
    _report(f"envmap {'on' if env_on else 'zero'}: pixels with " + " / ".join(pr.RECORD_KEYS) + " (9 renders)", " / ".join(str(seen[k]) for k in pr.RECORD_KEYS))
    assert all(seen[k] > 0 for k in pr.RECORD_KEYS), seen


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_bits(pt, scene):
    s = scene
    maps = (s["a"], s["r"], s["m"], s["env"])
    H, W, rm = s["H"], s["W"], s["rm"]
    rough, lights = pt.symbol("matpbr_path_render_objects_rough"), pt.symbol("matpbr_path_render_objects_lights")
    # every split of a frame into launches gives the same bits
    whole = s["tracer"].render(*maps, spp=6, max_depth=16, seed=7, spp_per_launch=6)
    for split in (1, 3, 4):
        assert np.array_equal(_bits(whole), _bits(s["tracer"].render(*maps, spp=6, max_depth=16, seed=7, spp_per_launch=split))), split
    # PathTracer.render with rough glass is the raw call
    out = torch.empty(H, W, 3, device=s["tracer"].device)
    keep, args = _raw_args(s["tracer"], maps, 6, 16, 5, 4, out)
    assert rough(*args, *tl.object_tail(s["tracer"])) == 0
    assert np.array_equal(_bits(s["tracer"].render(*maps, spp=6, max_depth=16, seed=5, spp_per_launch=4)), _bits(out))

    def routed(objects, entry, n_tail, direct=None):
        """`render` of a tracer without rough glass: the bits of its earlier entry point called directly, and of the new one."""
        tracer = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV, objects=objects)
        assert not tracer.rough and tracer.stats["n_rough_objects"] == 0
        ref = torch.empty(H, W, 3, device=tracer.device)
        keep, args = _raw_args(tracer, maps, 6, 16, 5, 4, ref)
        tail = tl.object_tail(tracer) if objects else ()
        assert (direct or pt.symbol(entry))(*args, *tail[:n_tail]) == 0
        assert np.array_equal(_bits(tracer.render(*maps, spp=6, max_depth=16, seed=5, spp_per_launch=4)), _bits(ref)), entry
        if objects:
            out = torch.empty(H, W, 3, device=tracer.device)
            _, args2 = _raw_args(tracer, maps, 6, 16, 5, 4, out)
            assert rough(*args2, *tail) == 0
            assert np.array_equal(_bits(out), _bits(ref)), entry

    routed(pl.table_scene(), "matpbr_path_render_objects_lights", 8)
    routed(pp.table_scene(), "matpbr_path_render_objects_pbr", 5)
    routed(ps.table_scene(), "matpbr_path_render_objects_normals", 4)
    routed(po.two_cubes(), "matpbr_path_render_objects", 2)
    routed(None, "matpbr_path_render", 0)
    # the older light entry point refuses the table with rough glass
    out = torch.empty(H, W, 3, device=s["tracer"].device)
    _, args3 = _raw_args(s["tracer"], maps, 1, 2, 0, 1, out)
    assert lights(*args3, *tl.object_tail(s["tracer"])) == -1


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------------
def _device_means(pt, objects, env, H=10, W=12):
    Vs, Ts = pp.FAR_TRIANGLE
    tracer = pt.PathTracer(Vs, Ts, H, W, FOV, objects=objects)
    maps = (np.zeros((H, W, 3), np.float32), np.ones((H, W, 1), np.float32), np.zeros((H, W, 1), np.float32))
    tabs = tracer.tables(env)
    vals = np.stack([tracer.render(*maps, env, spp=16, max_depth=16, seed=sd, spp_per_launch=16, tables=tabs).cpu().numpy() for sd in SEEDS])
    assert np.isfinite(vals).all()
    return vals.astype(np.float64)


def test_rough_sphere_in_a_constant_envmap(pt):
    """Host test 4's first scene on the device, the same 64 seeds x spp 16 at 12 x 10 and the same bound: the pixels that miss are c
    exactly, the covered ones at most c."""
    objects = pr.furnace_scene(False)
    inside, outside = tl.footprints(objects, 10, 12)
    c = np.float32(pr.FURNACE_C)
    vals = _device_means(pt, objects, np.full((4, 8, 3), pr.FURNACE_C, np.float32))
    assert inside.sum() >= 12 and outside.sum() >= 12
    assert np.abs(vals[:, outside] - float(c)).max() <= 2e-7                    # the mean of 16 equal fp32 values
    mean, se = vals.mean(0), vals.std(0, ddof=1) / math.sqrt(vals.shape[0])
    excess = ((mean - float(c)) / (5 * se + 1e-3 * float(c)))[inside]
    _report(f"rough sphere in a constant envmap, on the device: worst (mean - c) / (5 se + 1e-3 c) over {int(inside.sum())} pixels; the least mean / c",
            f"{excess.max():.3f}; {mean[inside].min() / float(c):.4f}")
    assert excess.max() <= 1.0 and mean[inside].min() > 0.5 * float(c)


def test_lamp_inside_the_rough_sphere(pt):
    """Host test 4's second scene on the device: finite, non-negative, non-zero, and within 5 standard errors of the difference + 1e-3
    of the restatement's mean without emitter samples (the two-sided MIS bookkeeping sums to one on the device as well)."""
    objects = pr.furnace_scene(True)
    inside, _ = tl.footprints(objects[:1], 10, 12)
    env = np.zeros((4, 8, 3), np.float32)
    vals = _device_means(pt, objects, env)
    Vs, Ts = pp.FAR_TRIANGLE
    V, T, table = pob.merged(Vs, Ts, objects)
    alone = pob.replay_mean(10, 12, 16, SEEDS, 16, V, T, env, pt.env_tables(env), table, emitter_sample=False)
    assert (vals >= 0).all() and vals[:, inside].max() > 0 and inside.sum() >= 12
    se = np.sqrt(vals.var(0, ddof=1) / vals.shape[0] + alone.var(0, ddof=1) / alone.shape[0])
    excess = (np.abs(vals.mean(0) - alone.mean(0)) / (5 * se + 1e-3 * np.abs(alone.mean(0)) + 1e-300))[inside]
    _report(f"lamp inside the rough sphere, on the device: worst |mean - mean without emitter samples| / (5 se + 1e-3) over {int(inside.sum())} pixels",
            f"{excess.max():.3f}")
    assert excess.max() <= 1.0


def test_features_of_a_rough_object(pt, scene):
    """id 1 + k and the normal the render shades the camera vertex with: the interpolated one on the smooth rough sphere, the face
    normal on the flat rough cube; the device agrees with the CPU routine."""
    s = scene
    H, W = s["H"], s["W"]
    geom = s["tracer"].features().cpu().numpy()
    Vm, Tm, tb, corner, _ = pt.merge_objects(s["rm"]["vertices"], s["rm"]["triangles"], s["objects"], normals=True, pbr=True)
    n_scene = s["rm"]["triangles"].shape[0]
    host = pt.features_host(pt.build_bvh(Vm, Tm, n_scene), H, W, FOV, tb, corner, n_scene)
    ids = host[..., 7]
    assert np.array_equal(geom[..., 7], ids) and set(np.unique(ids)) >= {0.0, 1.0, 2.0}
    assert np.abs(geom[..., 4:7] - host[..., 4:7]).max() <= 1e-5
    P = Vm[Tm]
    fn = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    fn /= np.linalg.norm(fn, axis=-1, keepdims=True)
    sl = slice(tb[1].first_tri, tb[1].first_tri + tb[1].n_tri)                               # the flat cube: some face normal of its own
    px = host[ids == 2][:, 4:7]
    assert px.shape[0] > 0 and (np.abs(px[:, None] - fn[sl][None]).max(-1).min(-1) <= 1e-5).all()
    ball = host[ids == 1]                                                                    # the smooth sphere: near the radial direction
    radial = ball[:, 0:3] - np.asarray(pr.ROUGH_SPHERE[0])
    radial /= np.linalg.norm(radial, axis=-1, keepdims=True)
    sl = slice(tb[0].first_tri, tb[0].first_tri + tb[0].n_tri)
    assert ball.shape[0] > 0 and (ball[:, 4:7] * radial).sum(-1).min() > 0.9
    assert (np.abs(ball[:, 4:7][:, None] - fn[sl][None]).max(-1).min(-1) > 1e-4).any()      # not the face normals


def test_render_final_cli_frosted_globe(pt, tmp_path):
    """`render_final.py --mode oi --oi_scene globe.json` with a lamp inside a frosted globe and a diffuse block: without the denoiser
    the bits of the direct PathTracer calls; with `--denoise atrous` finite and not constant."""
    from materialist_amd import mesh, relight
    from materialist_amd.imageio_exr import read_exr

    tmp = str(tmp_path)
    scene_dir = tl.synthetic_output(tmp)
    Vg, Tg, _ = ps.icosphere((0.03, 0.02, -0.9), 0.07, 1)
    Vl, Tl = pr.inner_quad((0.03, 0.02, -0.9), 0.02)
    Vb, Tb = po.cube((-0.09, -0.03, -0.9), 0.1, (0.4, 0.5, 0.3))
    Vg, Vl = (x.astype(np.float32).astype(np.float64) for x in (Vg, Vl))
    os.makedirs(os.path.join(tmp, "lists"))
    for name, (V, T) in (("globe.ply", (Vg, Tg)), ("lamp.ply", (Vl, Tl)), ("block.ply", (Vb, Tb))):
        mesh.write_ply(os.path.join(tmp, "lists", name), V, T)
    frosted = {"type": "roughdielectric", "int_ior": 1.49, "ext_ior": 1.000277, "alpha": 0.1}
    lamp = {"type": "area", "radiance": [30.0, 28.0, 22.0]}
    entries = [("globe.ply", frosted, "vertex"), ("lamp.ply", lamp, "flat"), ("block.ply", po.DIFFUSE_08, "flat")]
    listing = os.path.join(tmp, "lists", "globe.json")
    with open(listing, "w") as f:
        json.dump({"objects": [{"ply": n, "bsdf": b, "normals": nm} for n, b, nm in entries]}, f)
    cli = [sys.executable, os.path.join(ROOT, "render_final.py"), "--save_name", "case", "--input_path", tmp, "--save_path", tmp,
           "--mode", "oi", "--spp", "4", "--oi_iters", "2", "--oi_max_depth", "8", "--oi_scene", listing]
    mat = relight.load_estimated_brdf(os.path.join(scene_dir, "best_results"))
    env = relight.load_image(os.path.join(scene_dir, "best_results", "envmap.hdr"))
    objects = []
    for name, bsdf, normals in entries:
        V, T = mesh.read_ply_any(os.path.join(tmp, "lists", name))
        ob = {"vertices": V, "triangles": T, "bsdf": bsdf}
        if normals == "vertex":
            ob["normals"] = mesh.angle_weighted_normals(V, T)
        objects.append(ob)
    tracer = relight._path_tracer(scene_dir, "case", mat, "cuda", objects)
    assert tracer.stats["n_rough_objects"] == 1 and tracer.stats["n_lights"] == 1 and tracer.stats["n_smooth_objects"] == 1
    exr, png = (os.path.join(tmp, "case", "mi_oi_case_envmap" + ext) for ext in (".exr", ".png"))
    maps = (mat["albedo"], mat["roughness"], mat["metallic"])

    def run(extra):
        for path in (exr, png):
            if os.path.exists(path):
                os.remove(path)
        res = subprocess.run(cli + extra, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout + res.stderr
        assert os.path.exists(png)
        img = np.ascontiguousarray(read_exr(exr)[..., :3], dtype=np.float32)
        assert np.isfinite(img).all() and (img >= 0).all() and float(img.std()) > 0
        return img

    acc = torch.zeros_like(mat["albedo"])
    for seed in (0, 1):
        acc += tracer.render(*maps, env, spp=4, max_depth=8, seed=seed)
    assert np.array_equal(run([]).view(np.uint32), (acc / 2).cpu().numpy().view(np.uint32))
    run(["--denoise", "atrous"])
