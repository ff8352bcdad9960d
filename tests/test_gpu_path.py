"""The path-traced re-render on the GPU (libmatpbr_path.so): per-path parity with an fp64 numpy restatement,
agreement with the pinned deterministic render where the two must agree, Mitsuba's max_depth semantics, bit-reproducibility, the
reference's own Mitsuba render, and the render_final.py command line."""
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

import path_testlib as tl  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import path_fp64 as pf  # noqa: E402  (the fp64 restatement of the integrator)

pytestmark = pytest.mark.gpu

FOV = pf.FOV
groove_scene, _maps, _env = pf.groove_scene, pf.groove_maps, pf.groove_env


@pytest.fixture(scope="module")
def pt():
    return tl.load(gpu=True)


_report = tl.reporter("path", "test_gpu_path")


@pytest.fixture(scope="module")
def groove(pt):
    from materialist_amd import mesh

    H = W = 24
    rm = mesh.reference_mesh(groove_scene(H, W), FOV)
    rng = np.random.default_rng(11)
    a, r, m = _maps(H, W, rng)
    env = _env(rng)
    tracer = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV)
    return {"rm": rm, "a": a, "r": r, "m": m, "env": env, "tracer": tracer, "H": H, "W": W}


def test_every_path_matches_an_fp64_restatement(pt, groove, oracle64):
    g = groove
    H, W = g["H"], g["W"]
    tab = pt.env_tables(g["env"])
    V = g["rm"]["vertices"].astype(np.float32).astype(np.float64)
    worst = []
    for seed in (0, 1, 2):
        got = g["tracer"].render(g["a"], g["r"], g["m"], g["env"], spp=1, max_depth=4, seed=seed).cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all()
        ref, _ = pf.replay(oracle64, V, g["rm"]["triangles"], g["a"], g["r"], g["m"], g["env"], tab, H, W, 4, seed)
        scale = np.abs(ref).mean()
        err = (np.abs(got - ref) / np.maximum(np.abs(ref), scale)).max(-1)
        frac = float((err <= 1e-3).mean())
        worst.append(frac)
        _report(f"per-path parity seed {seed}: share of pixels within 1e-3", f"{frac:.4f} ({int((err > 1e-3).sum())} flipped paths, "
                f"max err {err.max():.3e})")
        assert frac >= 0.99, (seed, frac, np.argwhere(err > 1e-3)[:10])
    # the scene exercises what it is meant to: light arrives after more than one bounce
    d2 = g["tracer"].render(g["a"], g["r"], g["m"], g["env"], spp=16, max_depth=2, seed=5).cpu().numpy()
    d4 = g["tracer"].render(g["a"], g["r"], g["m"], g["env"], spp=16, max_depth=4, seed=5).cpu().numpy()
    assert (d4 - d2).mean() > 1e-3 * d4.mean()


def test_plane_agrees_with_the_deterministic_render(pt):
    _plane_vs_deterministic(pt, 48, 48)


def test_plane_agrees_with_the_deterministic_render_when_h_is_not_w(pt):
    """The same at 32 x 56: the texel a hit reads is the inverse of the camera, so each pixel's path shades
    with the pixel's own texel, as the deterministic render does (a lookup by a6 world_to_screen with fov_x would read another
    pixel's texel for nearly every pixel here)."""
    _plane_vs_deterministic(pt, 32, 56)


def _plane_vs_deterministic(pt, H, W):
    """A camera-facing plane cannot occlude or reflect onto itself, and a constant envmap is exact in SH25: the path render converges
    to the deterministic render's integral.  Bound: K independent renders (seeds) give per-pixel estimates X_k; per 8 x 8 block b the
    mean over its 64 pixels and the K renders has standard error sigma_b = sd(X) / sqrt(64 K) (pixels and seeds use disjoint RNG
    streams, so the 64 K estimates are independent).  The deterministic render has its own quadrature error; its size is bounded by
    the difference of its spp-64 and spp-128 rules, delta_b.  Every block must agree within 4 sigma_b + delta_b (a block fails by
    chance with p < 1e-4), and the image mean within 0.5 %."""
    from materialist_amd import mesh, render

    dev = torch.device("cuda:0")
    depth = np.full((H, W), 2.0, np.float32)
    rm = mesh.reference_mesh(depth, FOV)
    rng = np.random.default_rng(5)
    a, r, m = _maps(H, W, rng)
    env = np.full((16, 32, 3), 0.8, np.float32)
    tracer = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV)
    K = 8
    X = np.stack([tracer.render(a, r, m, env, spp=256, max_depth=4, seed=100 + k).cpu().numpy().astype(np.float64) for k in range(K)])
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    scene = render.load_estimated_mesh(t(depth), use_mesh_normal=True)
    scene._set("emitter.data", t(env))
    with torch.no_grad():
        det = {s: render.render_w_brdf(scene, t(a), t(r), t(m), None, s).cpu().numpy().astype(np.float64) for s in (64, 128)}
    inner = (slice(8, H - 8), slice(8, W - 8))       # away from the mesh border (jittered rays off its last half pixel see the sky)
    blk = lambda z: z[..., inner[0], inner[1], :].reshape(*z.shape[:-3], (H - 16) // 8, 8, (W - 16) // 8, 8, 3).mean(axis=(-4, -2))
    path_b = blk(X).mean(0)
    sigma = np.sqrt(blk(X.var(0, ddof=1)[None])[0] / (64 * K))
    det_b, delta = blk(det[128]), np.abs(blk(det[128]) - blk(det[64]))
    z = np.abs(path_b - det_b) / (4 * sigma + delta)
    rel_mean = abs(X.mean(0)[inner].mean() / det[128][inner].mean() - 1)
    _report(f"plane vs deterministic render {H}x{W}: max block |diff| / (4 sigma + delta)", f"{z.max():.3f}")
    _report(f"plane vs deterministic render {H}x{W}: image-mean relative difference", f"{rel_mean:.2e}")
    assert z.max() <= 1.0, (z.max(), np.unravel_index(z.argmax(), z.shape))
    assert rel_mean <= 5e-3


def test_max_depth_semantics(pt, groove):
    g = groove
    args = (g["a"], g["r"], g["m"], g["env"])
    d1 = g["tracer"].render(*args, spp=4, max_depth=1, seed=3).cpu().numpy()
    d2 = g["tracer"].render(*args, spp=4, max_depth=2, seed=3).cpu().numpy()
    d4 = g["tracer"].render(*args, spp=4, max_depth=4, seed=3).cpu().numpy()
    # every pixel of the groove has geometry under all its jittered rays except the outermost half-pixel ring
    assert np.all(d1[1:-1, 1:-1] == 0.0)
    assert np.all(d4 >= d2), np.argwhere(d4 < d2)[:5]
    assert np.all(d2 >= d1)
    assert (d2.sum(-1) > 0).mean() > 0.9          # direct light with shadows reaches most pixels at spp 4


def test_same_bits_for_every_split_and_seed(pt, groove):
    g = groove
    args = (g["a"], g["r"], g["m"], g["env"])
    x8 = g["tracer"].render(*args, spp=64, seed=7, spp_per_launch=8).cpu().numpy()
    x64 = g["tracer"].render(*args, spp=64, seed=7, spp_per_launch=64).cpu().numpy()
    x8b = g["tracer"].render(*args, spp=64, seed=7, spp_per_launch=8).cpu().numpy()
    x5 = g["tracer"].render(*args, spp=64, seed=7, spp_per_launch=5).cpu().numpy()
    other = g["tracer"].render(*args, spp=64, seed=8, spp_per_launch=8).cpu().numpy()
    assert np.array_equal(x8.view(np.uint32), x8b.view(np.uint32))
    assert np.array_equal(x8.view(np.uint32), x64.view(np.uint32))
    assert np.array_equal(x8.view(np.uint32), x5.view(np.uint32))
    assert not np.array_equal(x8, other)


def test_against_mitsuba_on_the_references_final_maps(pt, golden_dir):
    """tests/golden/indoor2.npz: the reference's final maps, MaterialNet's depth, the 16 x 32 envmap and Mitsuba's `path` render of
    them (max_depth 4, spp 64).  The path render and the deterministic render of the same maps, both against it."""
    from materialist_amd import mesh, render

    dev = torch.device("cuda:0")
    z = np.load(os.path.join(golden_dir, "indoor2.npz"))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    a = t(z["ref_albedo_u8"].astype(np.float32) / 255.0)
    r = t(z["ref_roughness_u8"].astype(np.float32)[..., None] / 255.0).clamp(0.07, 1.0)
    m = t(z["ref_metallic_u8"].astype(np.float32)[..., None] / 255.0)
    env = z["ref_envmap_f32"]
    ref = z["ref_render_f16"].astype(np.float64)
    depth = z["depth_pred_f32"]
    depth = 2 * depth.max() - depth                                                  # inverse_img_w_mi.py:722
    H, W = depth.shape
    rm = mesh.reference_mesh(depth, FOV)
    tracer = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV)
    _report("BVH of indoor2 (triangles, nodes, depth, MB, build ms)",
            f"{tracer.stats['n_tris']}, {tracer.stats['n_nodes']}, {tracer.stats['depth']}, {tracer.stats['bytes'] / 2**20:.1f}, "
            f"{tracer.stats['build_s'] * 1e3:.0f}")
    img = tracer.render(a, r, m, env, spp=256, max_depth=4, seed=0).cpu().numpy().astype(np.float64)
    assert np.isfinite(img).all()
    scene = render.load_estimated_mesh(t(depth), use_mesh_normal=True)
    scene._set("emitter.data", t(env))
    with torch.no_grad():
        direct = render.render_w_brdf(scene, a, r, m, None, 64).cpu().numpy().astype(np.float64)
    g = lambda x: np.clip(x, 0, 1) ** (1 / 2.2)
    psnr = lambda x, y: -10 * np.log10(np.mean((g(x) - g(y)) ** 2))
    res = {}
    for name, x in (("path", img), ("direct", direct)):
        res[name] = (psnr(x, ref), psnr(x * (ref.mean() / x.mean()), ref))
        _report(f"{name} render vs Mitsuba (indoor2), dB raw / mean-matched", f"{res[name][0]:.2f} / {res[name][1]:.2f}")
    assert res["path"][0] > 20.5 and res["path"][1] > 24.5, res
    # one 512 x 512 frame at spp 64, max_depth 4: hip events around the enqueued launches, rays counted by the kernel
    for _ in range(2):
        tracer.render(a, r, m, env, spp=64, max_depth=4, seed=1)
    rays = torch.zeros(H, W, dtype=torch.int32, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    tracer.render(a, r, m, env, spp=64, max_depth=4, seed=1, rays=rays)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    n_rays = float(rays.to(torch.float64).sum())
    _report("512x512 spp 64 max_depth 4 frame: ms, Mrays, Mrays/s", f"{ms:.1f}, {n_rays / 1e6:.1f}, {n_rays / 1e3 / ms:.0f}")
    assert ms < 5000.0


def test_render_final_cli_with_the_path_integrator(pt, tmp_path):
    from materialist_amd.imageio_exr import read_exr

    tmp = str(tmp_path)
    tl.synthetic_output(tmp, H=64, W=64)
    cli = [sys.executable, os.path.join(ROOT, "render_final.py"), "--save_name", "case", "--input_path", tmp, "--save_path", tmp,
           "--spp", "8", "--integrator", "path"]
    res = subprocess.run(cli + ["--mode", "real"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    exr = os.path.join(tmp, "case", "mi_case_envmap_.exr")
    assert os.path.exists(exr) and os.path.exists(exr[:-4] + ".png")
    img = read_exr(exr)
    assert img.shape[:2] == (64, 64) and np.isfinite(img).all() and img.mean() > 0
    res = subprocess.run(cli + ["--mode", "rolling", "--frames", "3", "--rotation_step", "90", "--max_depth", "3",
                               "--seed", "4"], capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    anim = os.path.join(tmp, "case", "rolling_envmap_animation")
    assert sorted(os.listdir(anim)) == ["frame_0000.png", "frame_0001.png", "frame_0002.png"]
    for ext in ("gif", "mp4"):
        assert os.path.getsize(os.path.join(tmp, "case", f"rolling_envmap_case_envmap.{ext}")) > 0
    from PIL import Image

    frames = [np.asarray(Image.open(os.path.join(anim, f))) for f in sorted(os.listdir(anim))]
    assert all(np.isfinite(f).all() for f in frames) and not np.array_equal(frames[0], frames[2])
    # without a .ply the scene is meshed from depthPred.exr as the pipeline does: the same mesh, the same image
    os.remove(os.path.join(tmp, "case", "case.ply"))
    res = subprocess.run(cli + ["--mode", "real"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert np.array_equal(read_exr(exr), img)
