"""PBR inserted objects on the GPU (libmatpbr_path.so's `matpbr_path_render_objects_pbr`, DESIGN.md section 1.4, "PBR inserted
objects"): every path of a table with all four object code paths against the fp64 restatement, a quad as depth mesh against the same
quad as a PBR object, bits (launch splits, tables without a PBR object, face normals as vertex normals, the routes `render` took
before), a furnace property, the refusals, and `render_final.py --mode oi --oi_scene` with and without the denoiser."""
import ctypes
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

import denoise_fp64 as dn  # noqa: E402
import path_fp64 as pf  # noqa: E402
import path_objects_fp64 as pob  # noqa: E402
import path_oi_fp64 as po  # noqa: E402
import path_oi_pbr_fp64 as pp  # noqa: E402
import path_oi_smooth_fp64 as ps  # noqa: E402
import path_testlib as tl  # noqa: E402
from path_testlib import bits as _bits, parity as _parity, raw_args as _raw_args, footprints as _footprints  # noqa: E402

pytestmark = pytest.mark.gpu

FOV = pf.FOV


@pytest.fixture(scope="module")
def pt():
    return tl.load(gpu=True)


_report = tl.reporter("path oi pbr", "test_gpu_path_oi_pbr")


@pytest.fixture(scope="module")
def scene(pt):
    """The groove at 24 x 20 (a partial tile) with `path_oi_pbr_fp64.table_scene` in front of it: a smooth metal icosphere, a flat PBR
    cube, a smooth glass icosphere and a flat diffuse cube in one table."""
    s = tl.groove_with_objects(pt, pp.table_scene(), pob.merged)
    tracer = s["tracer"]
    assert tracer.stats["n_objects"] == 4 and tracer.stats["n_pbr_objects"] == 2 and tracer.stats["n_smooth_objects"] == 2
    assert tracer.stats["n_object_tris"] == 184 and tracer.pbr is not None
    return s


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_every_path_matches_the_fp64_restatement(pt, scene, oracle64):
    """At least 0.99 of the pixels within 1e-3 (the rest: paths whose fp32 and fp64 hit decisions differ; on the CPU the restatement
    over the library's fp32 traversal and over the fp64 brute force disagree in no pixel of these six renders,
    test_path_oi_pbr_host.py)."""
    s = scene
    H, W = s["H"], s["W"]
    tab = pt.env_tables(s["env"])
    keys = ("pbr_vertex", "pbr_smooth_vertex", "blocked_by_object", "pbr_below_ng", "pbr_below_ng_carrying", "pbr_emitter_below_ng", "fallback")
    seen = {k: 0 for k in keys}
    for max_depth in (6, 16):
        for seed in (0, 1, 2):
            got = s["tracer"].render(s["a"], s["r"], s["m"], s["env"], spp=1, max_depth=max_depth, seed=seed).cpu().numpy().astype(np.float64)
            assert np.isfinite(got).all()
            ref, rec = pob.replay_objects(oracle64, s["V"], s["T"], s["a"], s["r"], s["m"], s["env"], tab, H, W, max_depth, seed, s["table"])
            frac, err = _parity(got, ref)
            _report(f"per-path parity with PBR objects, max_depth {max_depth} seed {seed}: share of pixels within 1e-3",
                    f"{frac:.4f} ({int((err > 1e-3).sum())} flipped paths, max err {err.max():.3e})")
            assert frac >= 0.99, (max_depth, seed, frac, np.argwhere(err > 1e-3)[:10])
            for k in ("pbr_vertex", "pbr_smooth_vertex", "blocked_by_object"):
                assert rec[k].any(), (k, max_depth, seed)     # the scene does what it is for, in every one of the renders
            for k in seen:
                seen[k] += int(rec[k].sum())
    _report("pixels with " + " / ".join(keys) + " (6 renders)", " / ".join(str(seen[k]) for k in keys))
    assert seen["pbr_below_ng"] >= 1 and seen["fallback"] >= 1


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
def _quad_setup(pt, H=10, W=12):
    Vq, Tq = pp.quad()
    const = {"type": "pbr", "albedo": (0.8, 0.45, 0.3), "roughness": 0.35, "metallic": 0.6}
    ca, cr, cm = pp.pbr_constants(const)
    a = np.broadcast_to(ca.astype(np.float32), (H, W, 3)).copy()
    r, m = np.full((H, W, 1), cr, np.float32), np.full((H, W, 1), cm, np.float32)
    env = pf.groove_env(np.random.default_rng(5))
    return Vq, Tq, const, a, r, m, env


def test_a_quad_as_depth_mesh_and_as_a_pbr_object(pt):
    """CPU test 4 on the device, spp 16: `matpbr_path_render` on the quad with constant maps against the quad as a flat PBR object
    (over a far-off triangle, maps that the object never reads), by the parity criterion.  The two instantiations run the same
    expressions on the same triangle records; whether the bits agree as well is reported, not asserted (the compiler may contract
    the two differently)."""
    H, W = 10, 12
    Vq, Tq, const, a, r, m, env = _quad_setup(pt, H, W)
    Vs, Ts = pp.FAR_TRIANGLE
    as_mesh = pt.PathTracer(Vq, Tq, H, W, FOV)
    as_object = pt.PathTracer(Vs, Ts, H, W, FOV, objects=[{"vertices": Vq, "triangles": Tq, "bsdf": const}])
    assert as_object.stats["n_pbr_objects"] == 1 and as_mesh.stats["n_objects"] == 0
    other = (np.zeros_like(a), np.ones_like(r), np.ones_like(m))
    for max_depth in (2, 4):
        ref = as_mesh.render(a, r, m, env, spp=16, max_depth=max_depth, seed=3)
        got = as_object.render(*other, env, spp=16, max_depth=max_depth, seed=3)
        frac, err = _parity(got.cpu().numpy().astype(np.float64), ref.cpu().numpy().astype(np.float64))
        same = np.array_equal(_bits(got), _bits(ref))
        _report(f"quad as depth mesh vs as PBR object, spp 16 max_depth {max_depth}: share within 1e-3, max err, bits equal",
                f"{frac:.4f}, {err.max():.3e}, {same}")
        assert bool(torch.isfinite(got).all()) and float(ref.mean()) > 0
        assert frac >= 0.99, (max_depth, frac)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_bits(pt, scene):
    s = scene
    maps = (s["a"], s["r"], s["m"], s["env"])
    H, W, rm = s["H"], s["W"], s["rm"]
    # every split of a frame into launches gives the same bits
    whole = s["tracer"].render(*maps, spp=6, max_depth=16, seed=7, spp_per_launch=6)
    for split in (1, 3):
        assert np.array_equal(_bits(whole), _bits(s["tracer"].render(*maps, spp=6, max_depth=16, seed=7, spp_per_launch=split))), split
    # a table without kind 3 through the new entry point: matpbr_path_render_objects_normals' bits, with and without records
    no_pbr = ps.table_scene()
    old = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV, objects=no_pbr)
    assert old.stats["n_pbr_objects"] == 0 and old.pbr is None and old.obj_nrm is not None
    ref = torch.empty(H, W, 3, device=old.device)
    keep, args = _raw_args(old, maps, 6, 16, 5, 4, ref)
    tail = (ctypes.cast(old.objects, ctypes.c_void_p), len(old.objects), old.obj_nrm.data_ptr(), old.n_scene_tris)
    assert pt.symbol("matpbr_path_render_objects_normals")(*args, *tail) == 0
    records = (pt.PathObjectPbr * len(old.objects))()
    for rec in (None, ctypes.cast(records, ctypes.c_void_p)):
        out = torch.empty(H, W, 3, device=old.device)
        _, args2 = _raw_args(old, maps, 6, 16, 5, 4, out)
        assert pt.symbol("matpbr_path_render_objects_pbr")(*args2, *tail, rec) == 0
        assert np.array_equal(_bits(out), _bits(ref))
    # PathTracer.render without PBR objects takes the routes it took: smooth objects, flat objects, no objects
    assert np.array_equal(_bits(old.render(*maps, spp=6, max_depth=16, seed=5, spp_per_launch=4)), _bits(ref))
    flat = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV, objects=po.two_cubes())
    assert flat.pbr is None and flat.obj_nrm is None and flat.stats["n_pbr_objects"] == 0
    ref = torch.empty(H, W, 3, device=flat.device)
    keep, args = _raw_args(flat, maps, 6, 16, 5, 4, ref)
    assert pt.load().matpbr_path_render_objects(*args, ctypes.cast(flat.objects, ctypes.c_void_p), len(flat.objects)) == 0
    assert np.array_equal(_bits(flat.render(*maps, spp=6, max_depth=16, seed=5, spp_per_launch=4)), _bits(ref))
    bare = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV)
    assert bare.pbr is None and bare.stats["n_pbr_objects"] == 0
    ref = torch.empty(H, W, 3, device=bare.device)
    keep, args = _raw_args(bare, maps, 6, 4, 5, 4, ref)
    assert pt.load().matpbr_path_render(*args) == 0
    assert np.array_equal(_bits(bare.render(*maps, spp=6, max_depth=4, seed=5, spp_per_launch=4)), _bits(ref))
    assert not np.array_equal(_bits(s["tracer"].render(*maps, spp=6, max_depth=16, seed=5)), _bits(old.render(*maps, spp=6, max_depth=16, seed=5)))


def test_face_normals_as_vertex_normals_give_the_flat_bits(pt):
    """A PBR object whose vertex normals are its face normals renders the flat object's bits.  The object is the unit square of
    `path_oi_pbr_fp64.quad`, behind a glass sphere and a diffuse cube that send paths to it from many directions: its edges are
    (1, 0, 0), (1, 1, 0), (0, 1, 0), so the kernel's face normal is (0, 0, 1) times the reciprocal square root of 1, exactly, and the
    interpolated normal is (0, 0, x) / sqrt(x^2) with x = ((1 - u) - v) + u + v within a few ulp of 1, which the correctly rounded
    square root and division return as 1 exactly (x^2 rounds to 1 +- 2 k ulp, its root to x, and x (1 / x) to 1).  On any other
    triangle the two normals may differ by an ulp, as test_gpu_path_oi_smooth.py notes, and so would the bits."""
    H, W = 20, 24
    Vq, Tq = pp.quad()
    Vs, Ts = pp.FAR_TRIANGLE
    Vg, Tg, Ng = ps.icosphere((-0.12, 0.05, -1.0), 0.1, 1)
    Vd, Td = po.cube((0.12, -0.06, -1.1), 0.12, (-0.3, 0.7, 0.2))
    front = [{"vertices": Vg, "triangles": Tg, "bsdf": po.GLASS, "normals": Ng}, {"vertices": Vd, "triangles": Td, "bsdf": po.DIFFUSE_08}]
    square = {"vertices": Vq, "triangles": Tq, "bsdf": pp.METAL}
    flat = pt.PathTracer(Vs, Ts, H, W, FOV, objects=[square] + front)
    smooth = pt.PathTracer(Vs, Ts, H, W, FOV, objects=[dict(square, normals=np.tile([0.0, 0.0, 2.5], (4, 1)))] + front)
    assert flat.stats["n_smooth_objects"] == 1 and smooth.stats["n_smooth_objects"] == 2 and smooth.stats["n_pbr_objects"] == 1
    assert smooth.objects[0].kind == 0x103 and flat.objects[0].kind == 3
    rng = np.random.default_rng(3)
    a, r, m = pf.groove_maps(H, W, rng)
    env = pf.groove_env(rng)
    for seed, max_depth in ((0, 4), (1, 16)):
        f = flat.render(a, r, m, env, spp=4, max_depth=max_depth, seed=seed)
        g = smooth.render(a, r, m, env, spp=4, max_depth=max_depth, seed=seed)
        assert float(f.mean()) > 0 and np.array_equal(_bits(g), _bits(f)), (seed, max_depth)
    tilted = pt.PathTracer(Vs, Ts, H, W, FOV, objects=[dict(square, normals=np.tile([0.3, 0.0, 1.0], (4, 1)))] + front)
    assert not np.array_equal(_bits(tilted.render(a, r, m, env, spp=4, max_depth=4, seed=0)), _bits(flat.render(a, r, m, env, spp=4, max_depth=4, seed=0)))


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_black_dielectric_ball_in_a_furnace(pt):
    """A smooth PBR icosphere (80 triangles) with a = 0, m = 0, r = 1 under a constant envmap c: every pixel inside its footprint is
    finite, not above c (1 + 1e-5) and darker than the same pixel with a = 1; the pixels outside it are c."""
    H, W = 20, 24
    c = np.float32(0.75)
    env = np.full((4, 8, 3), c, np.float32)
    Vs, Ts = pp.FAR_TRIANGLE
    Vb, Tb, Nb = ps.icosphere((0.01, -0.02, -1.2), 0.2, 1)
    maps = (np.full((H, W, 3), 0.5, np.float32), np.full((H, W, 1), 0.5, np.float32), np.zeros((H, W, 1), np.float32))
    img = {}
    for alb in (0.0, 1.0):
        ball = [{"vertices": Vb, "triangles": Tb, "bsdf": {"type": "pbr", "albedo": alb, "roughness": 1.0, "metallic": 0.0}, "normals": Nb}]
        tracer = pt.PathTracer(Vs, Ts, H, W, FOV, objects=ball)
        img[alb] = tracer.render(*maps, env, spp=64, max_depth=8, seed=0).cpu().numpy()
    inside, outside = _footprints(ball, H, W)
    assert inside.sum() > 20 and outside.sum() > 200
    black, white = img[0.0], img[1.0]
    _report("furnace, a = 0 m = 0 r = 1 ball: max over its pixels / c, mean / c; a = 1: mean / c; smallest white - black",
            f"{black[inside].max() / c:.6f}, {black[inside].mean() / c:.4f}; {white[inside].mean() / c:.4f}; {(white[inside] - black[inside]).min():.4f}")
    assert np.isfinite(black).all() and np.isfinite(white).all()
    assert np.all(black[outside] == c) and np.all(white[outside] == c)
    assert np.all(black[inside] <= c * (1 + 1e-5)), black[inside].max()
    assert np.all(black[inside] < white[inside])


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals(pt, scene):
    s = scene
    with pytest.raises(ValueError, match="objects"):
        s["tracer"].render_bwd(s["a"], s["r"], s["m"], s["env"], np.ones((s["H"], s["W"], 3), np.float32), spp=1)
    with pytest.raises(ValueError, match="objects"):
        s["tracer"].render_trans(s["a"], s["r"], s["m"], s["env"], np.ones((s["H"], s["W"]), bool), np.ones((s["H"], s["W"], 3), np.float32), spp=1)
    with pytest.raises(ValueError, match="objects"):
        s["tracer"].render(s["a"], s["r"], s["m"], s["env"], spp=1, normal=np.tile(np.float32([0, 0, 1]), (s["H"], s["W"], 1)))
    Vc, Tc = po.cube(*pp.PBR_CUBE)
    for field, value in (("roughness", 0.05), ("albedo", 1.5), ("metallic", float("nan"))):
        with pytest.raises(ValueError, match=field):
            pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], s["H"], s["W"], FOV,
                          objects=[{"vertices": Vc, "triangles": Tc, "bsdf": {"type": "pbr", field: value}}])
    # a record spoiled behind the binding's back: the library refuses it
    Vs, Ts = pp.FAR_TRIANGLE
    tracer = pt.PathTracer(Vs, Ts, 8, 8, FOV, objects=[{"vertices": Vc, "triangles": Tc, "bsdf": pp.PLASTIC}])
    tracer.pbr[0].r = 0.01
    maps = (np.full((8, 8, 3), 0.5, np.float32), np.full((8, 8, 1), 0.5, np.float32), np.zeros((8, 8, 1), np.float32))
    with pytest.raises(pt.PathError, match="matpbr_path_render_objects_pbr"):
        tracer.render(*maps, np.ones((4, 8, 3), np.float32), spp=1)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_render_final_cli_oi_scene(pt, tmp_path):
    """`render_final.py --mode oi --oi_scene scene.json` with one PBR and one glass object writes mi_oi_<name>_<env>.exr/.png, the
    bits of the direct PathTracer calls, finite and not constant; with `--denoise atrous` the image stays inside the per-id convex
    hull of its two half renders (test_gpu_denoise.py's property)."""
    from materialist_amd import mesh, relight
    from materialist_amd.imageio_exr import read_exr

    tmp = str(tmp_path)
    scene_dir = tl.synthetic_output(tmp)
    Vb, Tb, _ = ps.icosphere((0.08, -0.03, -0.95), 0.1, 1)
    Vb = Vb.astype(np.float32).astype(np.float64)
    Vg, Tg = po.cube((-0.09, 0.03, -0.9), 0.1, (0.4, 0.5, 0.3))
    os.makedirs(os.path.join(tmp, "lists", "meshes"))
    mesh.write_ply(os.path.join(tmp, "lists", "meshes", "chrome_ball.ply"), Vb, Tb)          # no normals: angle-weighted ones under "vertex"
    mesh.write_ply(os.path.join(tmp, "lists", "block.ply"), Vg, Tg)
    chrome = {"type": "pbr", "albedo": [0.95, 0.93, 0.88], "roughness": 0.1, "metallic": 1.0}
    listing = os.path.join(tmp, "lists", "scene.json")
    with open(listing, "w") as f:
        json.dump({"objects": [{"ply": "meshes/chrome_ball.ply", "bsdf": chrome, "normals": "vertex"}, {"ply": "block.ply", "bsdf": po.GLASS}]}, f)
    assert not os.path.exists(os.path.join(scene_dir, "oi.ply")) and not os.path.exists(os.path.join(scene_dir, "oi2.ply"))
    cli = [sys.executable, os.path.join(ROOT, "render_final.py"), "--save_name", "case", "--input_path", tmp, "--save_path", tmp,
           "--mode", "oi", "--spp", "4", "--oi_iters", "2", "--oi_max_depth", "8", "--oi_scene", listing]
    mat = relight.load_estimated_brdf(os.path.join(scene_dir, "best_results"))
    env = relight.load_image(os.path.join(scene_dir, "best_results", "envmap.hdr"))
    Vb_read, Tb_read = mesh.read_ply_any(os.path.join(tmp, "lists", "meshes", "chrome_ball.ply"))
    Vg_read, Tg_read = mesh.read_ply_any(os.path.join(tmp, "lists", "block.ply"))
    objects = [{"vertices": Vb_read, "triangles": Tb_read, "bsdf": chrome, "normals": mesh.angle_weighted_normals(Vb_read, Tb_read)},
               {"vertices": Vg_read, "triangles": Tg_read, "bsdf": po.GLASS}]
    tracer = relight._path_tracer(scene_dir, "case", mat, "cuda", objects)
    assert tracer.stats["n_pbr_objects"] == 1 and tracer.stats["n_smooth_objects"] == 1 and tracer.stats["n_objects"] == 2
    exr, png = (os.path.join(tmp, "case", "mi_oi_case_envmap" + ext) for ext in (".exr", ".png"))
    maps = (mat["albedo"], mat["roughness"], mat["metallic"])

    res = subprocess.run(cli, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert os.path.exists(png)
    img = np.ascontiguousarray(read_exr(exr)[..., :3], dtype=np.float32)
    assert np.isfinite(img).all() and float(img.std()) > 0
    acc = torch.zeros_like(mat["albedo"])
    for seed in (0, 1):                                                    # two renders averaged as render_oi averages them
        acc += tracer.render(*maps, env, spp=4, max_depth=8, seed=seed)
    acc /= 2
    assert np.array_equal(acc.cpu().numpy().view(np.uint32), img.view(np.uint32))
    geom = tracer.features()
    ids = geom[..., 7].cpu().numpy()
    assert set(np.unique(ids)) >= {0.0, 1.0, 2.0}                            # the mesh, the ball and the block are in view
    os.remove(exr)
    os.remove(png)

    res = subprocess.run(cli + ["--denoise", "atrous"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert os.path.exists(png)
    out = np.ascontiguousarray(read_exr(exr)[..., :3], dtype=np.float64)
    assert np.isfinite(out).all() and (out >= 0).all() and float(out.std()) > 0
    A, B = torch.zeros_like(mat["albedo"]), torch.zeros_like(mat["albedo"])
    for i in range(2):                                                      # render_oi's halves: seeds 2 i and 2 i + 1, spp / 2 each
        A += tracer.render(*maps, env, spp=2, max_depth=8, seed=2 * i)
        B += tracer.render(*maps, env, spp=2, max_depth=8, seed=2 * i + 1)
    mean = (A.cpu().numpy().astype(np.float64) + B.cpu().numpy().astype(np.float64)) / 4
    worst = dn.convex_hull_violation(out, mean, ids)
    _report("--oi_scene --denoise atrous, 32x32: worst excess over the per-id convex hull, relative to the largest input", worst)
    assert worst <= 1e-6
    guide = relight.albedo_guide(geom, mat["albedo"], [chrome, po.GLASS]).cpu().numpy()
    assert np.all(guide[ids == 1] == np.float32(chrome["albedo"])) and np.all(guide[ids == 2] == 1.0)
