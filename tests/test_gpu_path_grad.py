"""The path render's backward pass on the GPU (libmatpbr_path.so matpbr_path_render_bwd): per-path parity of
every gradient with the fp64 restatement (tests/path_fp64.py), the envmap's homogeneity, bit-reproducibility, the autograd face
(pathtrace.PathRenderFn under render.Scene's "path" integrator), what the fit gains in occluded pixels, and the command line."""
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
import path_testlib as tl  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pt():
    return tl.load(gpu=True)


_report = tl.reporter("path grad", "test_gpu_path_grad")


@pytest.fixture(scope="module")
def groove(pt):
    from materialist_amd import mesh

    H = W = 24
    rm = mesh.reference_mesh(pf.groove_scene(H, W), pf.FOV)
    rng = np.random.default_rng(11)
    a, r, m = pf.groove_maps(H, W, rng)
    env = pf.groove_env(rng)
    tracer = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, pf.FOV)
    d_out = np.random.default_rng(5).normal(size=(H, W, 3)).astype(np.float32)
    return {"rm": rm, "a": a, "r": r, "m": m, "env": env, "tracer": tracer, "H": H, "W": W, "d_out": d_out}


def _np(g):
    return {k: v.cpu().numpy().astype(np.float64) for k, v in g.items()}


def test_gradients_match_the_fp64_restatement(pt, groove, oracle64):
    g = groove
    H, W = g["H"], g["W"]
    tab = pt.env_tables(g["env"])
    V = g["rm"]["vertices"].astype(np.float32).astype(np.float64)
    for seed in (0, 1, 2):
        got = _np(g["tracer"].render_bwd(g["a"], g["r"], g["m"], g["env"], g["d_out"], spp=1, max_depth=4, seed=seed))
        _, rec = pf.replay(oracle64, V, g["rm"]["triangles"], g["a"], g["r"], g["m"], g["env"], tab, H, W, 4, seed)
        ref = pf.held_grad(oracle64, rec, g["a"].astype(np.float64), g["r"].astype(np.float64), g["m"].astype(np.float64),
                           g["env"].astype(np.float64), g["d_out"].astype(np.float64))
        for key in ("a", "r", "m", "env"):
            assert np.isfinite(got[key]).all()
            scale = np.abs(ref[key]).mean()
            err = (np.abs(got[key] - ref[key]) / np.maximum(np.abs(ref[key]), scale)).max(-1)
            frac = float((err <= 1e-3).mean())
            _report(f"seed {seed} d_{key}: share of texels within 1e-3", f"{frac:.4f} (max err {err.max():.3e})")
            assert frac >= 0.99, (seed, key, frac, np.argwhere(err > 1e-3)[:10])
            assert np.abs(ref[key]).max() > 0


@pytest.mark.parametrize("max_depth", [2, 4])
def test_envmap_homogeneity(pt, groove, max_depth):
    """With the tables held, the render is linear and homogeneous in the texels: sum d_env . env == sum d_out . out."""
    g = groove
    tabs = g["tracer"].tables(g["env"])
    kw = dict(spp=16, max_depth=max_depth, seed=9, tables=tabs)
    out = g["tracer"].render(g["a"], g["r"], g["m"], g["env"], **kw).cpu().numpy().astype(np.float64)
    d_env = g["tracer"].render_bwd(g["a"], g["r"], g["m"], g["env"], g["d_out"], want=("env",), **kw)["env"].cpu().numpy().astype(np.float64)
    lhs = float((d_env * g["env"]).sum())
    rhs = float((g["d_out"] * out).sum())
    _report(f"homogeneity max_depth {max_depth}: relative difference", f"{abs(lhs - rhs) / abs(rhs):.2e}")
    assert abs(lhs - rhs) <= 1e-5 * abs(rhs), (lhs, rhs)


def test_bits_splits_and_null_outputs(pt, groove):
    g = groove
    args = (g["a"], g["r"], g["m"], g["env"], g["d_out"])
    ref = g["tracer"].render_bwd(*args, spp=64, seed=7, spp_per_launch=8)
    again = g["tracer"].render_bwd(*args, spp=64, seed=7, spp_per_launch=8)
    for k in ref:
        assert torch.equal(ref[k].view(torch.int32), again[k].view(torch.int32)), k
    for spl in (1, 5, 64):
        other = g["tracer"].render_bwd(*args, spp=64, seed=7, spp_per_launch=spl)
        for k in ref:
            assert torch.equal(ref[k].view(torch.int32), other[k].view(torch.int32)), (spl, k)
    # d_out of any scale: the quantum follows max|d_out| (a power of two), so scaling d_out by 2^k scales the gradients exactly
    big = g["tracer"].render_bwd(*args[:4], g["d_out"] * 1024.0, spp=64, seed=7, spp_per_launch=8)
    for k in ref:
        assert torch.equal(big[k], ref[k] * 1024.0), k
    # a null pointer is not computed and its buffer is not touched; the others are ADDED to
    H, W = g["H"], g["W"]
    dev = g["tracer"].device
    sentinel = torch.full((H, W, 1), 3.25, device=dev)
    base_a = torch.full((H, W, 3), 0.5, device=dev)
    got = g["tracer"].render_bwd(*args, spp=64, seed=7, spp_per_launch=8, want=("a",), grads={"a": base_a})
    assert set(got) == {"a"} and got["a"] is base_a
    assert torch.equal(base_a, torch.full_like(base_a, 0.5) + ref["a"])
    assert torch.equal(sentinel, torch.full_like(sentinel, 3.25))
    only_r = g["tracer"].render_bwd(*args, spp=64, seed=7, spp_per_launch=8, want=("r",))
    assert torch.equal(only_r["r"], ref["r"])
    # the forward of the autograd face is PathTracer.render, bit for bit
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    env = t(g["env"]).requires_grad_(True)
    a = t(g["a"]).requires_grad_(True)
    ctx = {"tracer": g["tracer"], "spp": 8, "max_depth": 4, "seed": 3, "spp_per_launch": 8, "tables": pt.PathTables()}
    out = pt.PathRenderFn.apply(a, t(g["r"]), t(g["m"]), env, ctx)
    direct = g["tracer"].render(g["a"], g["r"], g["m"], g["env"], spp=8, max_depth=4, seed=3)
    assert torch.equal(out.detach().view(torch.int32), direct.view(torch.int32))


def test_render_w_brdf_backward_equals_render_bwd(pt, groove):
    from materialist_amd import render

    g = groove
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    scene = render.load_estimated_mesh(t(pf.groove_scene(g["H"], g["W"])), use_mesh_normal=True, max_path=4, integrator="path", seed=21)
    assert scene.integrator == "path"
    env = t(g["env"]).requires_grad_(True)
    a, r, m = (t(x).requires_grad_(True) for x in (g["a"], g["r"], g["m"]))
    render.render_envmap(scene, env, 16)                # sets emitter.data (the render itself is discarded)
    pred = render.render_w_brdf(scene, a, r, m, None, 16)
    seed = scene.last_seed
    (pred * t(g["d_out"])).sum().backward()
    ref = _np(scene.path["tracer"].render_bwd(g["a"], g["r"], g["m"], g["env"], g["d_out"], spp=16, max_depth=4, seed=seed))
    for key, x in (("a", a), ("r", r), ("m", m), ("env", env)):
        assert np.array_equal(x.grad.cpu().numpy(), ref[key].astype(np.float32)), key
    # the seeds come from a seeded sequence: a fresh scene with the same seed draws the same ones
    again = render.load_estimated_mesh(t(pf.groove_scene(g["H"], g["W"])), use_mesh_normal=True, integrator="path", seed=21)
    seq = np.random.default_rng(21)
    assert [again.next_seed() for _ in range(2)] == [int(seq.integers(0, 2 ** 32)) for _ in range(2)]
    # what the path render cannot do is refused
    with pytest.raises(ValueError, match="texels"):
        render.traverse(scene)["emitter.data"] = torch.zeros(25, 3, device=dev)
    with pytest.raises(ValueError, match="normal"):
        render.render_w_brdf(scene, a, r, m, t(np.tile([0.0, 0.0, 1.0], (g["H"], g["W"], 1))), 4)
    with pytest.raises(ValueError, match="use_mesh_normal"):
        render.traverse(scene)["shape.bsdf.use_mesh_normal"] = False


def test_path_fit_beats_sh_in_occluded_pixels(pt):
    """Ground truth from the path tracer with known maps; an 'a' part (loop.BrdfPhase) from the same start under "path" and under "sh".
    Error in the groove's occluded pixels after removing the global scale the loss's exposure ratio leaves free."""
    from materialist_amd import loop, mesh, render

    dev = torch.device("cuda:0")
    H = W = 64
    depth = pf.groove_scene(H, W)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    rng = np.random.default_rng(4)
    a_gt = np.clip(0.55 + 0.2 * rng.uniform(-1, 1, (H, W, 3)), 0, 1).astype(np.float32)
    r_gt = np.full((H, W, 1), 0.6, np.float32)
    m_gt = np.zeros((H, W, 1), np.float32)
    env = np.full((16, 32, 3), 0.3, np.float32)
    env[2:5, 8:12] = 12.0                                 # a bright patch high in the sky: the groove's walls shadow each other
    rm = mesh.reference_mesh(depth, pf.FOV)
    tracer = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, pf.FOV)
    gt = tracer.render(a_gt, r_gt, m_gt, env, spp=1024, max_depth=4, seed=1)
    with torch.no_grad():
        shadowed = tracer.render(np.ones_like(a_gt), r_gt, m_gt, env, spp=256, max_depth=2, seed=2).mean(-1)
        sh_scene = render.load_estimated_mesh(t(depth), use_mesh_normal=True, geometry="mesh")
        sh_scene._set("emitter.data", t(env))
        open_ = render.render_w_brdf(sh_scene, t(np.ones_like(a_gt)), t(r_gt), t(m_gt), None, 128).mean(-1)
    occ = (shadowed < 0.6 * open_).cpu().numpy()
    occ[:2], occ[-2:], occ[:, :2], occ[:, -2:] = False, False, False, False
    lit = (shadowed > 0.9 * open_).cpu().numpy()
    assert occ.sum() >= 50 and lit.sum() >= 200, (occ.sum(), lit.sum())
    errs = {}
    for kind in ("sh", "path"):
        if kind == "path":
            scene = render.load_estimated_mesh(t(depth), use_mesh_normal=True, max_path=4, integrator="path", seed=3)
        else:
            scene = render.load_estimated_mesh(t(depth), use_mesh_normal=True, geometry="mesh")
        render.traverse(scene)["emitter.data"] = t(env)
        start = t(np.full((H, W, 3), 0.5, np.float32))
        ph = loop.BrdfPhase(scene, gt, start, t(r_gt), t(m_gt), None, optimize_part="a", spp=16, lr=0.02, scale_delta=0.0)
        for _ in range(150):
            ph.step()
        a_fit = ph.current_maps()["albedo"].detach().cpu().numpy().astype(np.float64)
        a_fit *= a_gt[lit].mean() / a_fit[lit].mean()
        errs[kind] = float(np.abs(a_fit[occ] - a_gt[occ]).mean())
    _report("albedo error in occluded pixels, sh / path", f"{errs['sh']:.4f} / {errs['path']:.4f} ({int(occ.sum())} pixels)")
    # measured on an MI355X: sh 0.326, path 0.155 (1934 occluded pixels); the threshold leaves room below that margin
    assert errs["path"] < 0.6 * errs["sh"], errs


def _image(tmp, H=32, W=32):
    from PIL import Image

    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    img = np.stack([0.3 + 0.4 * (j / W), 0.5 - 0.2 * (i / H), 0.4 + 0.1 * ((i + j) % 5 == 0)], -1)
    path = os.path.join(tmp, "case.png")
    Image.fromarray((img * 255).astype(np.uint8)).save(path)
    return path


@pytest.mark.parametrize("model", ["none", "pos_mlp"])
def test_inverse_cli_with_the_path_integrator(pt, tmp_path, model):
    tmp = str(tmp_path)
    img = _image(tmp)
    cli = [sys.executable, os.path.join(ROOT, "inverse_img_w_mi.py"), "--img_inverse_path", img, "--save_name", "case", "--opt_src", "arm",
           "--opt_order", "arm", "--save_path", tmp, "--model_name", model, "--size", "32", "--spp", "4", "--num_epochs",
           "3" if model == "none" else "2", "--integrator", "path", "--max_depth", "3", "--seed", "5"]
    res = subprocess.run(cli, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    assert "integrator path" in res.stdout and "under the path-traced render" in res.stdout, res.stdout[-3000:]
    out = os.path.join(tmp, "case")
    for f in ("config.json", "final_envmap.hdr", "gt_image.exr", os.path.join("best_results", "albedo.exr"),
              os.path.join("best_results", "roughness.exr"), os.path.join("best_results", "metallic.exr"), os.path.join("best_results", "envmap.hdr")):
        assert os.path.exists(os.path.join(out, f)), f
    from materialist_amd.imageio_exr import read_exr

    alb = read_exr(os.path.join(out, "best_results", "albedo.exr"))
    assert alb.shape[:2] == (32, 32) and np.isfinite(alb).all()
