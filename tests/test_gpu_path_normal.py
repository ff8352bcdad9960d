"""The path render's shading normals on the GPU (libmatpbr_path.so's `matpbr_path_render_normals` / `matpbr_path_render_bwd_normals`,
DESIGN.md section 1.4, "Shading normals"): every path and every gradient against the fp64 restatement tests/path_normal_fp64.py,
partial tiles, the exact properties of both passes, the other renders' bits, the autograd face, the command lines, and the cost of
one indoor2 frame against the plain render and its backward pass."""
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
import path_normal_fp64 as pnf  # noqa: E402
import path_testlib as tl  # noqa: E402
from path_testlib import bits as _bits, parity as _parity  # noqa: E402

pytestmark = pytest.mark.gpu

FOV = pf.FOV
KEYS = ("a", "r", "m", "env", "n")


@pytest.fixture(scope="module")
def pt():
    return tl.load(gpu=True)


_report = tl.reporter("path normal", "test_gpu_path_normal")


def _scene(pt, H=24, W=24):
    s = pnf.normal_scene(pt, H, W)
    s["tracer"] = pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], H, W, FOV)
    s["maps"] = (s["a"], s["r"], s["m"], s["env"])
    return s


@pytest.fixture(scope="module")
def scene(pt):
    """The groove at 24 x 24 under path_normal_fp64.tilted_normals; a fixed d_out for the backward passes."""
    s = _scene(pt)
    s["d_out"] = np.random.default_rng(5).normal(size=(s["H"], s["W"], 3)).astype(np.float32)
    return s


def _replays(s, oracle64):
    return {(md, seed): pnf.replay_normal(oracle64, s["V"], s["T"], s["a"], s["r"], s["m"], s["env"], s["tab"], s["nrm"], s["H"], s["W"], md, seed)
            for md, seed in pnf.CASES}


@pytest.fixture(scope="module")
def replays(scene, oracle64):
    """The restatement's renders and records of the shared cases, computed once (the backward parity reads the max_depth 4 records)."""
    return _replays(scene, oracle64)


def _forward_parity(s, reps, where):
    for (max_depth, seed), (ref, rec) in reps.items():
        got = s["tracer"].render(*s["maps"], spp=1, max_depth=max_depth, seed=seed, normal=s["nrm"]).cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all()
        frac, err = _parity(got, ref)
        below, nov0 = rec["below"].reshape(s["H"], s["W"]), rec["nov0"].reshape(s["H"], s["W"])
        _report(f"per-path parity {where}, max_depth {max_depth} seed {seed}: share of pixels within 1e-3",
                f"{frac:.4f} ({int((err > 1e-3).sum())} flipped paths, max err {err.max():.3e}; over the {int(below.sum())} pixels with a sample below "
                f"the sheet {err[below].max():.3e}, over the {int(nov0.sum())} with ns . wo <= 0 {err[nov0].max():.3e})")
        assert frac >= 0.99, (where, max_depth, seed, frac, np.argwhere(err > 1e-3)[:10])
        assert below.any() and nov0.any(), (where, max_depth, seed)


def test_every_path_matches_the_fp64_restatement(pt, scene, replays):
    """At least 0.99 of the pixels within 1e-3 of max(|ref|, mean |ref|), everything finite, and every render meets vertices whose
    BSDF sample leaves below the face and vertices whose shading normal looks away from the viewer.  tests/test_path_normal_host.py
    shows the restatement alone, over fp32 and fp64 traversal, within half that cap on these renders."""
    _forward_parity(scene, replays, "24x24")
    # the map matters: the plain render of the same frame is another picture
    plain = scene["tracer"].render(*scene["maps"], spp=1, max_depth=4, seed=0).cpu().numpy().astype(np.float64)
    frac, _ = _parity(plain, replays[(4, 0)][0])
    assert frac < 0.5, frac


@pytest.mark.parametrize("H,W", [(36, 20), (17, 9)])
def test_partial_tiles(pt, oracle64, H, W):
    s = _scene(pt, H, W)
    _forward_parity(s, _replays(s, oracle64), f"{W}x{H}")


def test_gradients_match_the_fp64_restatement(pt, scene, replays, oracle64):
    """test_gpu_path_grad.py's per-texel form, per key: at least 0.99 of the texels within 1e-3 of max(|ref|, mean |ref|)."""
    s = scene
    f64 = lambda x: x.astype(np.float64)
    for seed in (0, 1, 2):
        got = s["tracer"].render_bwd(*s["maps"], s["d_out"], spp=1, max_depth=4, seed=seed, normal=s["nrm"], want=KEYS)
        got = {k: v.cpu().numpy().astype(np.float64) for k, v in got.items()}
        ref = pnf.held_grad_normal(oracle64, replays[(4, seed)][1], f64(s["a"]), f64(s["r"]), f64(s["m"]), f64(s["env"]), f64(s["nrm"]), f64(s["d_out"]))
        for key in KEYS:
            assert np.isfinite(got[key]).all()
            scale = np.abs(ref[key]).mean()
            err = (np.abs(got[key] - ref[key]) / np.maximum(np.abs(ref[key]), scale)).max(-1)
            frac = float((err <= 1e-3).mean())
            _report(f"seed {seed} d_{key}: share of texels within 1e-3", f"{frac:.4f} (max err {err.max():.3e})")
            assert frac >= 0.99, (seed, key, frac, np.argwhere(err > 1e-3)[:10])
            assert np.abs(ref[key]).max() > 0


def test_exact_properties(pt, scene):
    s = scene
    tr, H, W, dev = s["tracer"], s["H"], s["W"], s["tracer"].device
    args = (*s["maps"], s["d_out"])
    # forward: every split, and run to run
    x = tr.render(*s["maps"], spp=64, seed=7, spp_per_launch=8, normal=s["nrm"])
    assert np.array_equal(_bits(x), _bits(tr.render(*s["maps"], spp=64, seed=7, spp_per_launch=8, normal=s["nrm"])))
    for spl in (1, 5, 64):
        assert np.array_equal(_bits(x), _bits(tr.render(*s["maps"], spp=64, seed=7, spp_per_launch=spl, normal=s["nrm"]))), spl
    # backward: every gradient, d_n included
    kw = dict(spp=64, seed=7, normal=s["nrm"], want=KEYS)
    ref = tr.render_bwd(*args, spp_per_launch=8, **kw)
    again = tr.render_bwd(*args, spp_per_launch=8, **kw)
    for k in KEYS:
        assert torch.equal(ref[k].view(torch.int32), again[k].view(torch.int32)), k
        assert float(ref[k].abs().max()) > 0
    for spl in (1, 5, 64):
        other = tr.render_bwd(*args, spp_per_launch=spl, **kw)
        for k in KEYS:
            assert torch.equal(ref[k].view(torch.int32), other[k].view(torch.int32)), (spl, k)
    # d_out . 2^10 scales every gradient exactly
    big = tr.render_bwd(*s["maps"], s["d_out"] * 1024.0, spp_per_launch=8, **kw)
    for k in KEYS:
        assert torch.equal(big[k], ref[k] * 1024.0), k
    # a null d_n is not computed and leaves its buffer alone; the others keep their bits, and the gradients are ADDED
    sentinel = torch.full((H, W, 3), 3.25, device=dev)
    base_n = torch.full((H, W, 3), 0.5, device=dev)
    no_n = tr.render_bwd(*args, spp=64, seed=7, spp_per_launch=8, normal=s["nrm"], want=("a", "r", "m", "env"))
    assert set(no_n) == {"a", "r", "m", "env"}
    for k in no_n:
        assert torch.equal(no_n[k].view(torch.int32), ref[k].view(torch.int32)), k
    assert torch.equal(sentinel, torch.full_like(sentinel, 3.25))
    got = tr.render_bwd(*args, spp=64, seed=7, spp_per_launch=8, normal=s["nrm"], want=("n",), grads={"n": base_n})
    assert set(got) == {"n"} and got["n"] is base_n
    assert torch.equal(base_n, torch.full_like(base_n, 0.5) + ref["n"])
    # the library: nrm == NULL with a d_n is refused, a workspace of the plain size is too small for a map, and nothing is launched
    a, r, m, env, row, col, pdf = tr._inputs(*s["maps"], None)
    lib = pt.load()
    small = int(lib.matpbr_path_render_bwd_workspace_bytes(H, W, 8, 16))
    ws = torch.zeros(int(lib.matpbr_path_render_bwd_normals_workspace_bytes(H, W, 8, 16)), dtype=torch.uint8, device=dev)
    d_out, nrm = torch.from_numpy(s["d_out"]).to(dev), torch.from_numpy(s["nrm"]).to(dev)
    base = (tr.nodes.data_ptr(), tr.tris.data_ptr(), a.data_ptr(), r.data_ptr(), m.data_ptr(), H, W, FOV, env.data_ptr(), row.data_ptr(),
            col.data_ptr(), pdf.data_ptr(), 8, 16, 1, 4, 0, 8, d_out.data_ptr(), None, None, None, None, ws.data_ptr())
    assert lib.matpbr_path_render_bwd_normals(*base, ws.numel(), None, None, None, sentinel.data_ptr()) == -1
    assert lib.matpbr_path_render_bwd_normals(*base, small, None, None, nrm.data_ptr(), sentinel.data_ptr()) == -1
    torch.cuda.synchronize()
    assert torch.equal(sentinel, torch.full_like(sentinel, 3.25))
    # normal=None is the plain render and the plain backward pass, to the bit
    assert np.array_equal(_bits(tr.render(*s["maps"], spp=8, seed=3, normal=None)), _bits(tr.render(*s["maps"], spp=8, seed=3)))
    p0 = tr.render_bwd(*args, spp=8, seed=3)
    p1 = tr.render_bwd(*args, spp=8, seed=3, normal=None)
    for k in p0:
        assert torch.equal(p0[k].view(torch.int32), p1[k].view(torch.int32)), k
    with pytest.raises(ValueError, match="normal"):
        tr.render_bwd(*args, spp=1, want=("n",))


def test_other_renders_keep_their_bits(pt, scene):
    s = scene
    tr, H, W = s["tracer"], s["H"], s["W"]
    empty = pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], H, W, FOV, objects=[])
    mask = np.zeros((H, W), bool)
    mask[6:18, 4:14] = True
    bg = np.random.default_rng(1).uniform(0, 1, (H, W, 3)).astype(np.float32)
    for seed in (0, 7):
        def others():
            out = [tr.render(*s["maps"], spp=8, seed=seed), tr.render_trans(*s["maps"], mask, bg, spp=8, seed=seed),
                   empty.render(*s["maps"], spp=8, seed=seed)]
            g = tr.render_bwd(*s["maps"], s["d_out"], spp=8, seed=seed)
            return [_bits(x) for x in out] + [_bits(g[k]) for k in ("a", "r", "m", "env")]

        before = others()
        tr.render(*s["maps"], spp=8, seed=seed, normal=s["nrm"])
        tr.render_bwd(*s["maps"], s["d_out"], spp=8, seed=seed, normal=s["nrm"], want=KEYS)
        after = others()
        for k, (x, y) in enumerate(zip(before, after)):
            assert np.array_equal(x, y), (seed, k)
        assert np.array_equal(before[0], before[2])


def test_autograd_face(pt, scene):
    from materialist_amd import render

    s = scene
    H, W = s["H"], s["W"]
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    depth = t(pf.groove_scene(H, W))
    sc = render.load_estimated_mesh(depth, use_mesh_normal=False, max_path=4, integrator="path", seed=21, shading_normals="map")
    assert sc.integrator == "path" and sc.shading_normals == "map" and not sc.use_mesh_normal
    env = t(s["env"]).requires_grad_(True)
    a, r, m, n = (t(x).requires_grad_(True) for x in (s["a"], s["r"], s["m"], s["nrm"]))
    render.render_envmap(sc, env, 16)                   # sets emitter.data (the render itself is discarded)
    pred = render.render_w_brdf(sc, a, r, m, n, 16)
    seed = sc.last_seed
    tr = sc.path["tracer"]
    direct = tr.render(*s["maps"], spp=16, max_depth=4, seed=seed, normal=s["nrm"])
    assert np.array_equal(_bits(pred.detach()), _bits(direct))
    (pred * t(s["d_out"])).sum().backward()
    ref = tr.render_bwd(*s["maps"], s["d_out"], spp=16, max_depth=4, seed=seed, normal=s["nrm"], want=KEYS)
    for key, x in (("a", a), ("r", r), ("m", m), ("env", env), ("n", n)):
        assert np.array_equal(_bits(x.grad), _bits(ref[key].reshape(x.shape))), key
    assert float(n.grad.abs().max()) > 0
    # use_mesh_normal=True: the same scene passes no map, and renders the bits of a "face" scene with the same seed
    render.traverse(sc)["shape.bsdf.use_mesh_normal"] = True
    face = render.load_estimated_mesh(depth, use_mesh_normal=True, max_path=4, integrator="path", seed=33)
    both = []
    for scn in (sc, face):
        scn.path["rng"] = np.random.default_rng(33)
        render.traverse(scn)["emitter.data"] = t(s["env"])
        with torch.no_grad():
            both.append(render.render_w_brdf(scn, t(s["a"]), t(s["r"]), t(s["m"]), None, 8))
    assert sc.last_seed == face.last_seed
    assert np.array_equal(_bits(both[0]), _bits(both[1]))
    assert np.array_equal(_bits(both[0]), _bits(tr.render(*s["maps"], spp=8, max_depth=4, seed=sc.last_seed)))
    # a "face" scene refuses what it refused
    with pytest.raises(ValueError, match="normal"):
        render.render_w_brdf(face, t(s["a"]), t(s["r"]), t(s["m"]), t(s["nrm"]), 4)
    with pytest.raises(ValueError, match="use_mesh_normal"):
        render.traverse(face)["shape.bsdf.use_mesh_normal"] = False


def _image(tmp, H=32, W=32):
    from PIL import Image

    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    img = np.stack([0.3 + 0.4 * (j / W), 0.5 - 0.2 * (i / H), 0.4 + 0.1 * ((i + j) % 5 == 0)], -1)
    path = os.path.join(tmp, "case.png")
    Image.fromarray((img * 255).astype(np.uint8)).save(path)
    return path


@pytest.mark.parametrize("model,order", [("none", ["arm", "n"]), ("pos_mlp", ["armn"])])
def test_command_lines(pt, tmp_path, model, order):
    """test_inverse_cli_with_the_path_integrator's run with the normals in --opt_order, then render_final.py on its output.  SaveBest keeps
    a normal map only from an iteration that beats the best loss so far, and every path render draws a fresh seed: under `none` 30
    iterations per part at spp 16 get there (8 at spp 4 leave the initial map, measured), under `pos_mlp` 4 at spp 4 do."""
    from materialist_amd.imageio_exr import read_exr

    tmp = str(tmp_path)
    img = _image(tmp)
    cli = [sys.executable, os.path.join(ROOT, "inverse_img_w_mi.py"), "--img_inverse_path", img, "--save_name", "case", "--opt_src", "arm",
           "--opt_order", *order, "--save_path", tmp, "--model_name", model, "--size", "32", "--spp", "16" if model == "none" else "4", "--num_epochs",
           "30" if model == "none" else "4", "--integrator", "path", "--max_depth", "3", "--seed", "5", "--shading_normals", "map"]
    res = subprocess.run(cli, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-4000:]
    assert "integrator path" in res.stdout and "shading normals 'map'" in res.stdout and "under the path-traced render" in res.stdout, res.stdout[-3000:]
    out = os.path.join(tmp, "case")
    nrm = np.asarray(read_exr(os.path.join(out, "best_results", "normal.exr"))[..., :3], np.float64)
    first = np.asarray(read_exr(os.path.join(out, "normalPred.exr"))[..., :3], np.float64)
    assert nrm.shape == (32, 32, 3) and np.isfinite(nrm).all()
    assert np.abs(np.linalg.norm(nrm, axis=-1) - 1).max() < 1e-3
    assert np.abs(nrm - first).max() > 1e-6
    if model != "none":
        return
    imgs = {}
    for kind in ("face", "map"):
        fin = subprocess.run([sys.executable, os.path.join(ROOT, "render_final.py"), "--save_name", "case", "--input_path", tmp, "--save_path", tmp,
                              "--mode", "real", "--integrator", "path", "--spp", "8", "--shading_normals", kind], capture_output=True, text=True,
                             timeout=600)
        assert fin.returncode == 0, fin.stdout + fin.stderr
        imgs[kind] = np.array(read_exr(os.path.join(out, "mi_case_envmap_.exr"))[..., :3], np.float32)
        assert imgs[kind].shape == (32, 32, 3) and np.isfinite(imgs[kind]).all()
    # the flat prior's mesh is a plane, and the fitted map has moved a little off its face normal (3e-3 at most, measured): the two
    # renders share their seed, so they are the same picture but for the map, and not the same bits
    diff = np.abs(imgs["map"] - imgs["face"])
    _report("render_final.py, map against face: mean |difference| / mean face", f"{diff.mean() / imgs['face'].mean():.3e}")
    assert not np.array_equal(imgs["map"].view(np.uint32), imgs["face"].view(np.uint32))
    assert 0 < diff.mean() < 0.1 * imgs["face"].mean()


def test_indoor2_frame_against_the_plain_render(pt, golden_dir):
    """One 512 x 512 frame of tests/golden/indoor2.npz, spp 64, max_depth 4, with ops.normals_from_depth of its depth as the map:
    best of two timed frames after a warm-up, hip events, one process.  The bound of test_gpu_path_trans.py's frame test, at most 2
    for the render and for the backward pass with d_n, guards against spills; it is not a target.  Times, rays and ratios go to the report."""
    from materialist_amd import mesh, ops

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
    tracer = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV)
    nrm = ops.normals_from_depth(t(depth).contiguous(), FOV).reshape(H, W, 3).contiguous()
    assert float((nrm.norm(dim=-1) - 1).abs().max()) < 1e-4
    d_out = t(np.random.default_rng(0).normal(size=(H, W, 3)))
    tabs = tracer.tables(env)
    kw = dict(spp=64, max_depth=4, seed=1, tables=tabs)
    want_env = int(env.shape[0]) * int(env.shape[1]) <= pt.MAX_BWD_ENV_TEXELS
    keys = ("a", "r", "m") + (("env",) if want_env else ())

    def timed(fn):
        best, rays_sum, out = None, 0.0, None
        fn(None)                                                                     # warm-up
        for _ in range(2):
            rays = torch.zeros(H, W, dtype=torch.int32, device=dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(rays)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1)
            best, rays_sum = (ms if best is None else min(best, ms)), float(rays.to(torch.float64).sum())
        return best, rays_sum, out

    ms_p, rays_p, _ = timed(lambda rays: tracer.render(a, r, m, env, rays=rays, **kw))
    ms_n, rays_n, img = timed(lambda rays: tracer.render(a, r, m, env, rays=rays, normal=nrm, **kw))
    ms_bp, rays_bp, _ = timed(lambda rays: tracer.render_bwd(a, r, m, env, d_out, rays=rays, want=keys, **kw))
    ms_bn, rays_bn, g = timed(lambda rays: tracer.render_bwd(a, r, m, env, d_out, rays=rays, want=keys + ("n",), normal=nrm, **kw))
    assert bool(torch.isfinite(img).all()) and all(bool(torch.isfinite(v).all()) for v in g.values())
    assert float(g["n"].abs().max()) > 0
    _report("512x512 spp 64 max_depth 4 frame: render with the map ms, Mrays, Mrays/s; plain ms, Mrays; ratio",
            f"{ms_n:.1f}, {rays_n / 1e6:.1f}, {rays_n / 1e3 / ms_n:.0f}; {ms_p:.1f}, {rays_p / 1e6:.1f}; {ms_n / ms_p:.3f}")
    _report(f"512x512 spp 64 max_depth 4 frame: render_bwd {keys + ('n',)} with the map ms, Mrays, Mrays/s; plain {keys} ms, Mrays; ratio",
            f"{ms_bn:.1f}, {rays_bn / 1e6:.1f}, {rays_bn / 1e3 / ms_bn:.0f}; {ms_bp:.1f}, {rays_bp / 1e6:.1f}; {ms_bn / ms_bp:.3f}")
    assert ms_n <= 2.0 * ms_p
    assert ms_bn <= 2.0 * ms_bp
