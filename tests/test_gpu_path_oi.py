"""Object insertion on the GPU (libmatpbr_path.so's `matpbr_path_render_objects`, DESIGN.md section 1.4, "Inserted objects"): the
render without objects keeps its bits, every path with a glass and a diffuse cube against the fp64 restatement, a glass furnace,
bit-reproducibility and max_depth, the refusals, the `render_final.py --mode oi` command line, and the rate of one indoor2 frame."""
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
import path_oi_fp64 as po  # noqa: E402
import path_testlib as tl  # noqa: E402
from path_testlib import bits as _bits, footprints as _footprints, erode as _erode  # noqa: E402

pytestmark = pytest.mark.gpu

FOV = pf.FOV


@pytest.fixture(scope="module")
def pt():
    return tl.load(gpu=True)


_report = tl.reporter("path oi", "test_gpu_path_oi")


@pytest.fixture(scope="module")
def scene(pt):
    """The groove at 24 x 20 with the glass and the diffuse cube in front of it."""
    s = tl.groove_with_objects(pt, po.two_cubes(), po.merged)
    s["plain"] = pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], s["H"], s["W"], FOV)
    return s


def test_no_objects_same_bits(pt, scene):
    s = scene
    args = (s["a"], s["r"], s["m"], s["env"])
    for objects in ([], None):
        tracer = pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], s["H"], s["W"], FOV, objects=objects)
        assert tracer.stats["n_objects"] == 0 and tracer.stats["n_object_tris"] == 0
        for seed in (0, 7):
            assert np.array_equal(_bits(tracer.render(*args, spp=8, seed=seed)), _bits(s["plain"].render(*args, spp=8, seed=seed)))
    assert s["tracer"].stats["n_objects"] == 2 and s["tracer"].stats["n_object_tris"] == 24
    assert s["tracer"].stats["n_tris"] == s["rm"]["triangles"].shape[0] + 24


def test_every_path_matches_an_fp64_restatement(pt, scene, oracle64):
    """test_gpu_path.py's criterion: per-pixel error relative to max(|ref|, mean |ref|), at least 0.99 of the pixels within 1e-3 (the
    rest: paths whose fp32 and fp64 hit decisions differ; on the CPU the restatement over the library's fp32 traversal and over the
    fp64 brute force disagree in no pixel of these six renders)."""
    s = scene
    H, W = s["H"], s["W"]
    tab = pt.env_tables(s["env"])
    seen = {"transmitted": 0, "diffuse_object": 0, "blocked_by_object": 0}
    for max_depth in (6, 16):
        for seed in (0, 1, 2):
            got = s["tracer"].render(s["a"], s["r"], s["m"], s["env"], spp=1, max_depth=max_depth, seed=seed).cpu().numpy().astype(np.float64)
            assert np.isfinite(got).all()
            ref, rec = po.replay_oi(oracle64, s["V"], s["T"], s["a"], s["r"], s["m"], s["env"], tab, H, W, max_depth, seed, s["table"])
            err = (np.abs(got - ref) / np.maximum(np.abs(ref), np.abs(ref).mean())).max(-1)
            frac = float((err <= 1e-3).mean())
            _report(f"per-path parity with objects, max_depth {max_depth} seed {seed}: share of pixels within 1e-3",
                    f"{frac:.4f} ({int((err > 1e-3).sum())} flipped paths, max err {err.max():.3e})")
            assert frac >= 0.99, (max_depth, seed, frac, np.argwhere(err > 1e-3)[:10])
            for k in seen:
                seen[k] += int(rec[k].sum())
                assert rec[k].any(), (k, max_depth, seed)     # the scene does what it is for, in every one of the renders
    _report("pixels with a transmitted vertex / a diffuse-object vertex / an emitter sample an object blocks (6 renders)",
            f"{seen['transmitted']} / {seen['diffuse_object']} / {seen['blocked_by_object']}")


def test_glass_furnace(pt):
    """A glass cube under a constant envmap c: every path that escapes carries c (the eta^2 factors of a closed object cancel, to fp32
    rounding), a truncated path carries 0.  c = 0.75, so that the 64 samples of a pixel that misses sum without rounding."""
    H = W = 32
    c = np.float32(0.75)
    env = np.full((4, 8, 3), c, np.float32)
    # the tracer needs a depth mesh: one triangle far out of view, too small (4e-10 sr) for a ray off the cube to find
    Vs = np.array([[50.0, 50.0, -1.0], [50.001, 50.0, -1.0], [50.0, 50.001, -1.0]])
    Vc, Tc = po.cube((0.01, -0.02, -1.2), 0.3, (0.4, 0.5, 0.3))
    glass = [{"vertices": Vc, "triangles": Tc, "bsdf": po.GLASS}]
    tracer = pt.PathTracer(Vs, np.array([[0, 1, 2]], np.int32), H, W, FOV, objects=glass)
    maps = (np.full((H, W, 3), 0.5, np.float32), np.full((H, W, 1), 0.5, np.float32), np.zeros((H, W, 1), np.float32))
    img = tracer.render(*maps, env, spp=64, max_depth=16, seed=0).cpu().numpy()
    inside, outside = _footprints(glass, H, W)
    core = _erode(inside)
    assert core.sum() > 50 and outside.sum() > 400
    assert np.all(img[outside] == c)
    assert np.all(img <= c * (1 + 1e-5)), img.max()
    assert np.all(img[core] > 0)
    _report("glass furnace: mean over the cube's inner pixels / c (what max_depth 16 truncates is missing)", f"{img[core].mean() / c:.4f}")


def test_splits_and_max_depth(pt, scene, oracle64):
    s = scene
    args = (s["a"], s["r"], s["m"], s["env"])
    x8 = s["tracer"].render(*args, spp=64, max_depth=16, seed=7, spp_per_launch=8)
    for split in (5, 64):
        assert np.array_equal(_bits(x8), _bits(s["tracer"].render(*args, spp=64, max_depth=16, seed=7, spp_per_launch=split))), split
    d2, d6, d16 = (s["tracer"].render(*args, spp=8, max_depth=k, seed=3).cpu().numpy() for k in (2, 6, 16))
    assert np.all(d16 >= d6) and np.all(d6 >= d2), (np.argwhere(d16 < d6)[:5], np.argwhere(d6 < d2)[:5])
    assert (d6 - d2).mean() > 1e-3 * d6.mean()
    # max_depth 2: a camera ray that enters the glass finds the cube's far side, a surface beyond the last vertex, and the pixel
    # is exactly 0; so is one whose reflection off the cube finds the mesh.  (A reflection that escapes sees the envmap: that ray
    # is the path's second, which max_depth 2 still traces.)  The cubes' shadows: emitter samples the objects block.
    tab = pt.env_tables(s["env"])
    shadowed = 0
    for seed in (0, 1, 2):
        got = s["tracer"].render(*args, spp=1, max_depth=2, seed=seed).cpu().numpy()
        bare = s["plain"].render(*args, spp=1, max_depth=2, seed=seed).cpu().numpy()
        _, rec = po.replay_oi(oracle64, s["V"], s["T"], s["a"], s["r"], s["m"], s["env"], tab, s["H"], s["W"], 2, seed, s["table"])
        first = np.full(s["H"] * s["W"], -1)
        for v in rec["object_vertices"]:
            first[v["pix"]] = v["kind"]
        for v in rec["vertices"]:
            first[v["pix"]] = po.SCENE
        escaped = np.zeros(s["H"] * s["W"], bool)
        for e in rec["escapes"]:
            escaped[e["pix"]] = True
        glass = first == po.DIELECTRIC
        gl = got.reshape(-1, 3).sum(-1)
        print(f"[path oi] max_depth 2 seed {seed}: transmitted {int(rec['transmitted'].sum())} (nonzero {int((gl[rec['transmitted']] != 0).sum())}), "
              f"glass not escaped {int((glass & ~escaped).sum())} (nonzero {int((gl[glass & ~escaped] != 0).sum())}), "
              f"glass escaped {int((glass & escaped).sum())} (zero {int((gl[glass & escaped] == 0).sum())})")
        assert rec["transmitted"].sum() > 40 and np.all(got.reshape(-1, 3)[rec["transmitted"]] == 0.0)
        assert np.all(got.reshape(-1, 3)[glass & ~escaped] == 0.0) and np.all(got.reshape(-1, 3)[glass & escaped].sum(-1) > 0)
        # where the camera sees the mesh, objects only take light away: the emitter sample or the second ray they block.  The
        # two renders run two instantiations of the kernel, whose fp32 contractions may differ, so "no brighter" holds to fp32
        # rounding of the same path: the parity criterion, 1e-3 of max(value, image mean), far below any term an object removes.
        on_mesh = first == po.SCENE
        g, b = got.reshape(-1, 3)[on_mesh].astype(np.float64), bare.reshape(-1, 3)[on_mesh].astype(np.float64)
        excess = ((g - b) / np.maximum(b, bare.mean())).max()
        print(f"[path oi] max_depth 2 seed {seed}: largest excess over the render without objects on the mesh: {excess:.3e}")
        assert excess <= 1e-3
        # the cubes' shadows: pixels of the mesh whose emitter sample an object blocks and nothing else does
        _, rec0 = pf.replay(oracle64, s["rm"]["vertices"].astype(np.float32).astype(np.float64), s["rm"]["triangles"], s["a"], s["r"], s["m"],
                            s["env"], tab, s["H"], s["W"], 2, seed)
        lit = np.zeros(s["H"] * s["W"], bool)
        lit[rec0["vertices"][0]["pix"]] = rec0["vertices"][0]["em"]
        shadow = on_mesh & rec["blocked_by_object"] & lit
        shadowed += int(shadow.sum())
        print(f"[path oi] max_depth 2 seed {seed}: shadow pixels {np.nonzero(shadow)[0].tolist()}, with objects "
              f"{got.reshape(-1, 3)[shadow].sum(-1).tolist()}, without {bare.reshape(-1, 3)[shadow].sum(-1).tolist()}")
        assert np.all(got.reshape(-1, 3)[shadow].sum(-1) < bare.reshape(-1, 3)[shadow].sum(-1))
    assert shadowed > 0


def test_refusals(pt, scene):
    s = scene
    with pytest.raises(ValueError, match="objects"):
        s["tracer"].render_bwd(s["a"], s["r"], s["m"], s["env"], np.ones((s["H"], s["W"], 3), np.float32), spp=1)
    with pytest.raises(ValueError, match="at most 8"):
        pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], s["H"], s["W"], FOV, objects=[s["objects"][0]] * 9)
    bad = dict(s["objects"][0], triangles=np.array([[0, 1, 8]], np.int32))
    with pytest.raises(ValueError, match="indices"):
        pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], s["H"], s["W"], FOV, objects=[bad])
    for bsdf in ({"type": "glass"}, {"type": "dielectric", "int_ior": 0.0, "ext_ior": 1.0}, {"type": "diffuse", "reflectance": (0.5, 1.2, 0.5)}):
        with pytest.raises(ValueError):
            pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], s["H"], s["W"], FOV, objects=[dict(s["objects"][0], bsdf=bsdf)])


def test_render_final_cli_inserts_objects(pt, tmp_path):
    from materialist_amd import mesh, relight
    from materialist_amd.imageio_exr import read_exr
    from materialist_amd.imageio_hdr import write_hdr

    tmp = str(tmp_path)
    H = W = 32
    scene_dir = tl.synthetic_output(tmp)
    Vg, Tg = po.cube((-0.05, 0.03, -0.9), 0.16, (0.4, 0.5, 0.3))
    Vd, Td = po.cube((0.10, -0.04, -1.0), 0.14, (-0.3, 0.7, 0.2))
    Vg = Vg.astype(np.float32).astype(np.float64)
    with open(os.path.join(scene_dir, "oi.ply"), "w") as f:                    # somebody else's file: ASCII, float vertices
        f.write("ply\nformat ascii 1.0\ncomment a cube\nelement vertex 8\nproperty float x\nproperty float y\nproperty float z\n"
                "element face 12\nproperty list uchar int vertex_indices\nend_header\n" +
                "".join(f"{v[0]!r} {v[1]!r} {v[2]!r}\n" for v in Vg.tolist()) + "".join(f"3 {t[0]} {t[1]} {t[2]}\n" for t in Tg.tolist()))
    mesh.write_ply(os.path.join(scene_dir, "oi2.ply"), Vd, Td)
    cli = [sys.executable, os.path.join(ROOT, "render_final.py"), "--save_name", "case", "--input_path", tmp, "--save_path", tmp]
    oi = cli + ["--mode", "oi", "--spp", "4", "--oi_iters", "2", "--oi_max_depth", "8"]
    res = subprocess.run(oi, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    exr = os.path.join(tmp, "case", "mi_oi_case_envmap.exr")
    assert os.path.exists(exr) and os.path.exists(exr[:-4] + ".png")
    img = read_exr(exr)
    assert img.shape[:2] == (H, W) and np.isfinite(img).all()
    res = subprocess.run(cli + ["--mode", "real", "--integrator", "path", "--spp", "8"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    real = read_exr(os.path.join(tmp, "case", "mi_case_envmap_.exr"))
    objects = [{"vertices": Vg, "triangles": Tg, "bsdf": po.GLASS}, {"vertices": Vd, "triangles": Td, "bsdf": po.DIFFUSE_08}]
    inside, _ = _footprints(objects, H, W)
    assert inside.sum() > 20 and np.abs(img[..., :3] - real[..., :3])[inside].mean() > 0.02 * real[..., :3].mean()
    # the same image from PathTracer.render: two renders, seeds 0 and 1, averaged as render_oi averages them
    mat = relight.load_estimated_brdf(os.path.join(scene_dir, "best_results"))
    tracer = relight._path_tracer(scene_dir, "case", mat, "cuda", objects)
    env = relight.load_image(os.path.join(scene_dir, "best_results", "envmap.hdr"))
    acc = torch.zeros_like(mat["albedo"])
    for seed in (0, 1):
        acc += tracer.render(mat["albedo"], mat["roughness"], mat["metallic"], env, spp=4, max_depth=8, seed=seed)
    acc /= 2
    assert np.array_equal(acc.cpu().numpy().view(np.uint32), np.ascontiguousarray(img[..., :3], dtype=np.float32).view(np.uint32))
    # best_results/envmap_opt.hdr goes before envmap.hdr
    write_hdr(os.path.join(scene_dir, "best_results", "envmap_opt.hdr"), np.full((8, 16, 3), 0.5, np.float32))
    res = subprocess.run(oi, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    opt = os.path.join(tmp, "case", "mi_oi_case_envmap_opt.exr")
    assert os.path.exists(opt) and os.path.exists(opt[:-4] + ".png") and not np.array_equal(read_exr(opt), img)


def _icosphere(centre, radius, levels=3):
    """An icosahedron subdivided `levels` times (20 x 4^levels triangles), outward winding."""
    t = (1 + 5 ** 0.5) / 2
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    V = [np.array(v, np.float64) / np.linalg.norm(v) for v in V]
    T = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(levels):
        mid, T2 = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                v = V[i] + V[j]
                V.append(v / np.linalg.norm(v))
                mid[key] = len(V) - 1
            return mid[key]

        for a, b, c in T:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            T2 += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        T = T2
    return np.array(V) * radius + np.asarray(centre, np.float64), np.array(T, np.int32)


def test_indoor2_frame_with_objects(pt, golden_dir):
    """One 512 x 512 frame of tests/golden/indoor2.npz (set up as test_gpu_path.py's Mitsuba test sets it up) with a glass sphere of
    1280 triangles and a diffuse cube in front of the scene, spp 32, max_depth 16: the time and the rate go to the report; the bound is
    that test's generous "finishes"."""
    from materialist_amd import mesh

    dev = torch.device("cuda:0")
    z = np.load(os.path.join(golden_dir, "indoor2.npz"))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    a = t(z["ref_albedo_u8"].astype(np.float32) / 255.0)
    r = t(z["ref_roughness_u8"].astype(np.float32)[..., None] / 255.0).clamp(0.07, 1.0)
    m = t(z["ref_metallic_u8"].astype(np.float32)[..., None] / 255.0)
    env = z["ref_envmap_f32"]
    depth = z["depth_pred_f32"]
    depth = 2 * depth.max() - depth                                                  # inverse_img_w_mi.py:722
    H, W = depth.shape
    rm = mesh.reference_mesh(depth, FOV)
    z0 = 0.6 * float(depth[depth > 0].min())                                         # in front of everything
    Vs, Ts = _icosphere((-0.10 * z0, 0.0, -z0), 0.09 * z0)
    Vc, Tc = po.cube((0.13 * z0, -0.05 * z0, -z0), 0.13 * z0, (0.3, 0.6, 0.2))
    objects = [{"vertices": Vs, "triangles": Ts, "bsdf": po.GLASS}, {"vertices": Vc, "triangles": Tc, "bsdf": po.DIFFUSE_08}]
    c = Vs.mean(0)
    P = Vs[Ts]
    assert Ts.shape[0] == 1280 and np.all((np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]) * (P.mean(1) - c)).sum(-1) > 0)
    tracer = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV, objects=objects)
    assert tracer.stats["n_object_tris"] == 1292
    for _ in range(2):
        img = tracer.render(a, r, m, env, spp=32, max_depth=16, seed=1)
    assert bool(torch.isfinite(img).all())
    rays = torch.zeros(H, W, dtype=torch.int32, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    tracer.render(a, r, m, env, spp=32, max_depth=16, seed=1, rays=rays)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    n_rays = float(rays.to(torch.float64).sum())
    _report("512x512 spp 32 max_depth 16 frame with a glass sphere (1280 triangles) and a diffuse cube: ms, Mrays, Mrays/s",
            f"{ms:.1f}, {n_rays / 1e6:.1f}, {n_rays / 1e3 / ms:.0f}")
    assert ms < 5000.0
