"""Transparency editing on the GPU (libmatpbr_path.so's `matpbr_path_render_trans`, DESIGN.md section 1.4, "Transparency editing"):
every path against the fp64 restatement tests/path_trans_fp64.py, the exact properties of the edit, the other two renders' bits,
partial tiles, the refusals, the `trans_edit.py` command line, and the cost of one indoor2 frame against the plain render."""
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
import path_trans_fp64 as ptf  # noqa: E402
import path_testlib as tl  # noqa: E402
from path_testlib import bits as _bits, parity as _parity  # noqa: E402

pytestmark = pytest.mark.gpu

FOV = pf.FOV


@pytest.fixture(scope="module")
def pt():
    return tl.load(gpu=True)


_report = tl.reporter("path trans", "test_gpu_path_trans")


@pytest.fixture(scope="module")
def scene(pt):
    """The groove at 24 x 20 (path_trans_fp64.trans_scene: the masked maps as trans_edit.py sets them, a random background)."""
    s = ptf.trans_scene(pt)
    s["tracer"] = pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], s["H"], s["W"], FOV)
    s["maps"] = (s["a"], s["r"], s["m"], s["env"])
    return s


@pytest.fixture(scope="module")
def replays(scene, oracle64):
    """The restatement's renders and records of the shared cases, computed once."""
    s = scene
    out = {}
    for max_depth, seed, ior, T in ptf.CASES:
        out[(max_depth, seed, ior, T)] = ptf.replay_trans(oracle64, s["V"], s["T"], s["a"], s["r"], s["m"], s["env"], s["tab"], s["H"], s["W"],
                                                         max_depth, seed, s["mask"], s["bg"], ior, T)
    return out


def test_every_path_matches_an_fp64_restatement(pt, scene, replays):
    """At least 0.99 of the pixels within 1e-3 of max(|ref|, mean |ref|), everything finite.  The rest are paths whose fp32 and fp64
    hit decisions differ: tests/test_path_trans_host.py shows the restatement alone, over the library's fp32 traversal and over the
    fp64 brute force, stays within half that cap on these renders."""
    s = scene
    for (max_depth, seed, ior, T), (ref, rec) in replays.items():
        got = s["tracer"].render_trans(*s["maps"], s["mask"], s["bg"], ior, T, spp=1, max_depth=max_depth, seed=seed).cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all()
        frac, err = _parity(got, ref)
        mv = rec["masked_vertex"].reshape(s["H"], s["W"])
        _report(f"per-path parity, max_depth {max_depth} seed {seed} ior {ior} T {T}: share of pixels within 1e-3",
                f"{frac:.4f} ({int((err > 1e-3).sum())} flipped paths, max err {err.max():.3e}; over pixels with a masked vertex {err[mv].max():.3e}, "
                f"below-surface {err[rec['below'].reshape(s['H'], s['W'])].max() if rec['below'].any() else 0.0:.3e})")
        assert frac >= 0.99, (max_depth, seed, ior, T, frac, np.argwhere(err > 1e-3)[:10])
        assert rec["masked_vertex"].any() and (~rec["masked_vertex"]).any()


def test_exact_properties(pt, scene, oracle64):
    s = scene
    tr, H, W = s["tracer"], s["H"], s["W"]
    edit = (s["mask"], s["bg"])
    # every split of a frame into launches gives the same bits
    x8 = tr.render_trans(*s["maps"], *edit, spp=8, seed=3, spp_per_launch=8)
    for split in (1, 3):
        assert np.array_equal(_bits(x8), _bits(tr.render_trans(*s["maps"], *edit, spp=8, seed=3, spp_per_launch=split))), split
    # a longer path only adds light
    d2, d4 = (tr.render_trans(*s["maps"], *edit, spp=8, max_depth=k, seed=3).cpu().numpy() for k in (2, 4))
    assert np.all(d4 >= d2), np.argwhere(d4 < d2)[:5]
    assert (d4 - d2).mean() > 1e-3 * d4.mean()
    # T = 0: the background does not enter
    other = np.ascontiguousarray(1.0 - s["bg"][::-1])
    t0 = tr.render_trans(*s["maps"], s["mask"], s["bg"], 1.2, 0.0, spp=8, seed=3)
    assert np.array_equal(_bits(t0), _bits(tr.render_trans(*s["maps"], s["mask"], other, 1.2, 0.0, spp=8, seed=3)))
    assert not np.array_equal(_bits(x8), _bits(tr.render_trans(*s["maps"], s["mask"], other, spp=8, seed=3)))
    # pixels none of whose 8 samples meets a masked texel do not know T or the index of refraction
    touched = np.zeros(H * W, bool)
    for sample in range(8):
        _, rec = ptf.replay_trans(oracle64, s["V"], s["T"], s["a"], s["r"], s["m"], s["env"], s["tab"], H, W, 4, 3, s["mask"], s["bg"], sample=sample)
        touched |= rec["masked_vertex"]
    free = ~touched.reshape(H, W)
    assert free.sum() >= 40 and touched.sum() >= H * W // 4
    t9 = tr.render_trans(*s["maps"], *edit, 1.2, 0.9, spp=8, seed=3)
    i15 = tr.render_trans(*s["maps"], *edit, 1.5, 0.4, spp=8, seed=3)
    assert np.array_equal(_bits(x8)[free], _bits(t9)[free]) and np.array_equal(_bits(x8)[free], _bits(i15)[free])
    assert (_bits(x8)[~free] != _bits(t9)[~free]).any() and (_bits(x8)[~free] != _bits(i15)[~free]).any()
    # an all-false mask: MatDiffBSDF's values under TransBSDF's pdf and weight, whatever the index and T
    none = np.zeros_like(s["mask"])
    ref, rec = ptf.replay_trans(oracle64, s["V"], s["T"], s["a"], s["r"], s["m"], s["env"], s["tab"], H, W, 4, 0, none, s["bg"])
    e0 = tr.render_trans(*s["maps"], none, s["bg"], 1.2, 0.4, spp=1, seed=0)
    frac, err = _parity(e0.cpu().numpy().astype(np.float64), ref)
    _report("all-false mask, max_depth 4 seed 0: share of pixels within 1e-3", f"{frac:.4f} (max err {err.max():.3e})")
    assert frac >= 0.99 and not rec["masked_vertex"].any()
    for ior, T in ((1.5, 0.4), (1.2, 0.9), (1.0, 0.0)):
        assert np.array_equal(_bits(e0), _bits(tr.render_trans(*s["maps"], none, other, ior, T, spp=1, seed=0)))


def test_other_renders_keep_their_bits(pt, scene):
    s = scene
    empty = pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], s["H"], s["W"], FOV, objects=[])
    for seed in (0, 7):
        before = s["tracer"].render(*s["maps"], spp=8, seed=seed)
        s["tracer"].render_trans(*s["maps"], s["mask"], s["bg"], spp=8, seed=seed)
        after = s["tracer"].render(*s["maps"], spp=8, seed=seed)
        assert np.array_equal(_bits(before), _bits(after))
        assert np.array_equal(_bits(before), _bits(empty.render(*s["maps"], spp=8, seed=seed)))


@pytest.mark.parametrize("H,W", [(36, 20), (17, 9)])
def test_partial_tiles(pt, oracle64, H, W):
    s = ptf.trans_scene(pt, H, W)
    tr = pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], H, W, FOV)
    ref, rec = ptf.replay_trans(oracle64, s["V"], s["T"], s["a"], s["r"], s["m"], s["env"], s["tab"], H, W, 4, 1, s["mask"], s["bg"])
    got = tr.render_trans(s["a"], s["r"], s["m"], s["env"], s["mask"], s["bg"], spp=1, max_depth=4, seed=1).cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    frac, err = _parity(got, ref)
    _report(f"per-path parity at {W} x {H}: share of pixels within 1e-3", f"{frac:.4f} ({int((err > 1e-3).sum())} flipped paths, max err {err.max():.3e})")
    assert frac >= 0.99 and rec["masked_vertex"].any()


def test_refusals(pt, scene):
    s = scene
    H, W = s["H"], s["W"]
    cube = {"vertices": np.array([[x, y, z] for z in (-1.3, -1.2) for y in (-0.05, 0.05) for x in (-0.05, 0.05)], np.float64),
            "triangles": np.array([[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2],
                                   [1, 3, 7], [1, 7, 5]], np.int32), "bsdf": {"type": "diffuse", "reflectance": (0.8, 0.8, 0.8)}}
    with_objects = pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], H, W, FOV, objects=[cube])
    with pytest.raises(ValueError, match="objects"):
        with_objects.render_trans(*s["maps"], s["mask"], s["bg"], spp=1)
    with pytest.raises(ValueError, match="mask"):
        s["tracer"].render_trans(*s["maps"], s["mask"][:-1], s["bg"], spp=1)
    with pytest.raises(ValueError, match="bg"):
        s["tracer"].render_trans(*s["maps"], s["mask"], s["bg"][:, :-1], spp=1)
    with pytest.raises(ValueError, match="bg"):
        s["tracer"].render_trans(*s["maps"], s["mask"], s["bg"][..., 0], spp=1)
    with pytest.raises(ValueError, match="ior"):
        s["tracer"].render_trans(*s["maps"], s["mask"], s["bg"], ior=0.0, spp=1)
    with pytest.raises(ValueError, match="spec_trans"):
        s["tracer"].render_trans(*s["maps"], s["mask"], s["bg"], spec_trans=1.5, spp=1)
    # the library refuses the same by itself
    import ctypes

    dev = s["tracer"].device
    a, r, m, env, row, col, pdf = s["tracer"]._inputs(*s["maps"], None)
    out = torch.zeros(H, W, 3, device=dev)
    mk = torch.from_numpy(s["mask"].astype(np.uint8)).to(dev)
    bg = torch.from_numpy(s["bg"]).to(dev)
    base = (s["tracer"].nodes.data_ptr(), s["tracer"].tris.data_ptr(), a.data_ptr(), r.data_ptr(), m.data_ptr(), H, W, FOV, env.data_ptr(),
            row.data_ptr(), col.data_ptr(), pdf.data_ptr(), int(env.shape[0]), int(env.shape[1]), 1, 4, 0, 8, out.data_ptr(), None, None)
    lib = pt.load()
    for ed, mp, bp in ((pt.PathTransEdit(0.0, 0.4, 100.0, 0.0), mk.data_ptr(), bg.data_ptr()), (pt.PathTransEdit(1.2, 1.5, 100.0, 0.0), mk.data_ptr(), bg.data_ptr()),
                       (pt.PathTransEdit(1.2, 0.4, -1.0, 0.0), mk.data_ptr(), bg.data_ptr()), (pt.PathTransEdit(1.2, 0.4, float("inf"), 0.0), mk.data_ptr(), bg.data_ptr()),
                       (pt.PathTransEdit(1.2, 0.4, 100.0, 0.0), None, bg.data_ptr()), (pt.PathTransEdit(1.2, 0.4, 100.0, 0.0), mk.data_ptr(), None)):
        assert lib.matpbr_path_render_trans(*base, mp, bp, ctypes.cast(ctypes.byref(ed), ctypes.c_void_p)) == -1
    assert lib.matpbr_path_render_trans(*base, mk.data_ptr(), bg.data_ptr(), None) == -1
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0                               # nothing was launched
    # no backward pass goes through it
    a_req = torch.from_numpy(s["a"]).to(dev).requires_grad_(True)
    img = s["tracer"].render_trans(a_req, s["r"], s["m"], s["env"], s["mask"], s["bg"], spp=1)
    assert not img.requires_grad and img.grad_fn is None


def test_trans_edit_cli(pt, tmp_path):
    from materialist_amd import relight
    from materialist_amd.imageio_exr import read_exr

    tmp = str(tmp_path)
    scene_dir, mask = tl.synthetic_output(tmp, edit=True)
    common = ["--save_name", "case", "--input_path", tmp, "--save_path", tmp]
    cli = [sys.executable, os.path.join(ROOT, "trans_edit.py"), *common, "--spp", "4", "--iters", "2"]
    res = subprocess.run(cli, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    exr = os.path.join(tmp, "case", "mi_trans_1.2_woA_0.4_case_envmap.exr")
    assert os.path.exists(exr) and os.path.exists(exr[:-4] + ".png"), os.listdir(os.path.join(tmp, "case"))
    img = np.ascontiguousarray(read_exr(exr)[..., :3], dtype=np.float32)
    assert img.shape == (32, 32, 3) and np.isfinite(img).all()
    # the same image from PathTracer.render_trans: seeds 0 and 1, averaged as render_trans averages them
    mat = relight.load_estimated_brdf(os.path.join(scene_dir, "best_results"))
    assert np.array_equal(mat["mask"].cpu().numpy(), mask) and tuple(mat["bg"].shape) == (32, 32, 3)
    a, r, m = mat["albedo"].clone(), mat["roughness"].clone(), mat["metallic"].clone()
    a[mat["mask"]], r[mat["mask"]], m[mat["mask"]] = 0.7, 0.3, 0.0
    tracer = relight._path_tracer(scene_dir, "case", mat, "cuda")
    env = relight.load_image(os.path.join(scene_dir, "best_results", "envmap.hdr"))
    acc = torch.zeros_like(a)
    for seed in (0, 1):
        acc += tracer.render_trans(a, r, m, env, mat["mask"], mat["bg"], 1.2, 0.4, 100.0, spp=4, max_depth=4, seed=seed)
    acc /= 2
    assert np.array_equal(acc.cpu().numpy().view(np.uint32), img.view(np.uint32))
    # inside the mask it is another picture than the plain path render, and another again with the albedo kept
    real = subprocess.run([sys.executable, os.path.join(ROOT, "render_final.py"), *common, "--mode", "real", "--integrator", "path", "--spp", "8"],
                          capture_output=True, text=True, timeout=600)
    assert real.returncode == 0, real.stdout + real.stderr
    plain = read_exr(os.path.join(tmp, "case", "mi_case_envmap_.exr"))[..., :3]
    assert np.abs(img - plain)[mask].mean() > 0.02 * plain.mean()
    res = subprocess.run(cli + ["--keep_albedo_color"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    kept = os.path.join(tmp, "case", "mi_trans_1.2_wA_0.4_case_envmap.exr")
    assert os.path.exists(kept) and os.path.exists(kept[:-4] + ".png")
    wa = read_exr(kept)[..., :3]
    assert np.abs(wa - img)[mask].mean() > 0.005 * plain.mean()


def test_indoor2_frame_against_the_plain_render(pt, golden_dir):
    """One 512 x 512 frame of tests/golden/indoor2.npz (set up as test_gpu_path_oi.py's indoor2 test sets it up), a centred disc mask,
    the input photograph as the background, spp 64, max_depth 4: the time, the rays and the ratio to `render` of the same frame (the
    NoObjects instantiation, whose instructions are the parent's) go to the report.  The bound, at most 2, guards against spills or a
    runaway tail of the 1e-6 paths; it is not a target."""
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
    tracer = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV)
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    mask = torch.from_numpy((i - H / 2) ** 2 + (j - W / 2) ** 2 < (0.3 * H) ** 2).to(dev)
    bg = t(z["image_srgb_u8"].astype(np.float32) / 255.0)
    a[mask], r[mask], m[mask] = 0.7, 0.3, 0.0                                        # trans_edit.py:25-28
    tabs = tracer.tables(env)
    kw = dict(spp=64, max_depth=4, seed=1, tables=tabs)

    def timed(fn):
        rays = torch.zeros(H, W, dtype=torch.int32, device=dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        img = fn(rays)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), float(rays.to(torch.float64).sum()), img

    plain = lambda rays=None: tracer.render(a, r, m, env, rays=rays, **kw)
    trans = lambda rays=None: tracer.render_trans(a, r, m, env, mask, bg, rays=rays, **kw)
    plain(), trans()                                                                 # warm both
    ms_p, rays_p, _ = timed(plain)
    ms_t, rays_t, img = timed(trans)
    ms_p2, _, _ = timed(plain)
    ms_t2, _, _ = timed(trans)
    ms_p, ms_t = min(ms_p, ms_p2), min(ms_t, ms_t2)
    assert bool(torch.isfinite(img).all())
    _report("512x512 spp 64 max_depth 4 frame, disc mask: trans ms, Mrays, Mrays/s; plain ms, Mrays; ratio of the times",
            f"{ms_t:.1f}, {rays_t / 1e6:.1f}, {rays_t / 1e3 / ms_t:.0f}; {ms_p:.1f}, {rays_p / 1e6:.1f}; {ms_t / ms_p:.3f}")
    assert ms_t <= 2.0 * ms_p
