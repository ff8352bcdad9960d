"""Host side of transparency editing ("Transparency editing"): the masked-branch BSDF and the refracted texel
lookup the kernel runs (on the CPU) against the fp64 restatement tests/path_trans_fp64.py, the restatement's own sensitivity to fp32
hit decisions on the GPU test's scene, the `bg.png` input and the command line.  No GPU needed."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import path_fp64 as pf  # noqa: E402
import path_trans_fp64 as ptf  # noqa: E402
import path_testlib as tl  # noqa: E402


@pytest.fixture(scope="module")
def path_lib():
    return tl.load()


_report = tl.reporter("path trans", "test_path_trans_host")


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _f32(x):
    """rounded to fp32 as the library receives it, held in fp64 for the restatement"""
    return np.asarray(x, np.float32).astype(np.float64)


# ---- 1. the masked-branch value and pdf ---------------------------------------------------------------------------------------------
def _eval_lanes():
    rng = np.random.default_rng(5)
    N = 4096
    n = _unit(rng.normal(size=(N, 3)))
    wo = _unit(rng.normal(size=(N, 3)))
    wo = np.where(((wo * n).sum(-1) > 0)[:, None], wo, -wo)            # the viewer is above the surface, as at every vertex of a path
    wi = _unit(rng.normal(size=(N, 3)))                               # the light on both sides of it
    a = rng.uniform(0.05, 0.95, (N, 3))
    r = rng.uniform(0.05, 1.0, N)
    m = rng.choice([0.0, 0.3, 1.0], N)
    bg = rng.uniform(0.0, 1.0, (N, 3))
    # named lanes, on the normal z: wi = wo = n; n . wi = 0 exactly; wo . h < 1e-4 (wi all but opposite to wo); bg = 0
    z, x = np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0])
    w45 = np.array([np.sqrt(0.5), 0.0, np.sqrt(0.5)])
    phi = 1e-4                                                         # wo . h = sin(phi / 2) = 5e-5
    opp = -w45 * np.cos(phi) + np.array([0.0, 1.0, 0.0]) * np.sin(phi)
    named = {"wi = wo = n": (z, z, z, 0.3), "n . wi = 0": (z, w45, x, 0.3), "wo . h < 1e-4": (z, w45, opp, 0.5), "bg = 0": (z, w45, _unit(np.array([-0.3, 0.2, 0.9])), 0.4),
             "wi = wo = n, r 0.05": (z, z, z, 0.05)}
    k = len(named)
    n = np.concatenate([n, np.stack([v[0] for v in named.values()])])
    wo = np.concatenate([wo, np.stack([v[1] for v in named.values()])])
    wi = np.concatenate([wi, np.stack([v[2] for v in named.values()])])
    a = np.concatenate([a, np.full((k, 3), 0.7)])
    r = np.concatenate([r, [v[3] for v in named.values()]])
    m = np.concatenate([m, np.zeros(k)])
    bgn = np.full((k, 3), 0.6)
    bgn[list(named).index("bg = 0")] = 0.0
    bg = np.concatenate([bg, bgn])
    return tuple(_f32(v) for v in (n, wo, wi, a, r, m, bg)), list(named), N


def test_trans_eval_host_against_the_restatement(path_lib, oracle64):
    """The project's criterion for eval_brdf: error relative to max(|ref|, mean |ref|) <= 1e-3, for f and for the pdf."""
    (n, wo, wi, a, r, m, bg), names, N = _eval_lanes()
    assert 0.3 < ((n * wi).sum(-1) > 0).mean() < 0.7                  # wi on both sides
    voh = np.maximum((wo * _unit(wi + wo)).sum(-1), 0)
    assert voh[N + names.index("wo . h < 1e-4")] < 1e-4 and (n * wi).sum(-1)[N + names.index("n . wi = 0")] == 0.0
    worst_f = worst_p = 0.0
    for ior in (1.0, 1.2, 1.5):
        for T in (0.0, 0.4, 1.0):
            f, pdf = path_lib.trans_eval_host(n, wo, wi, a, r, m, bg, ior, T)
            rf, rp = ptf.eval_trans(oracle64, wi, wo, n, a, r, m, bg, np.ones(n.shape[0], bool), ior, T)
            assert np.isfinite(f).all() and np.isfinite(pdf).all() and np.isfinite(rf).all() and np.isfinite(rp).all()
            assert (f >= 0).all() and (pdf >= 0).all()
            ef = (np.abs(f - rf) / np.maximum(np.abs(rf), np.abs(rf).mean())).max(-1)
            ep = np.abs(pdf - rp) / np.maximum(np.abs(rp), np.abs(rp).mean())
            worst_f, worst_p = max(worst_f, ef.max()), max(worst_p, ep.max())
            print(f"[path trans] ior {ior} T {T}: f err {ef.max():.3e} (lane {ef.argmax()}), pdf err {ep.max():.3e} (lane {ep.argmax()}); named "
                  + ", ".join(f"{nm}: {ef[N + i]:.1e}/{ep[N + i]:.1e}" for i, nm in enumerate(names)))
            below = ~((n * wi).sum(-1) > 0)
            if T > 0:
                nz = below & (m < 1) & (bg > 0).all(-1)
                assert (rf[nz] > 0).all() and rf[below].max() < 1e-3   # the transmission branch: small, not zero
                assert (f[nz] > 0).all()
    _report("trans_eval_host vs fp64 over 9 (ior, T): max error of f, of pdf, relative to max(|ref|, mean |ref|)", f"{worst_f:.3e}, {worst_p:.3e}")
    assert worst_f <= 1e-3 and worst_p <= 1e-3
    # T = 0: the background does not enter, to the bit
    f0, p0 = path_lib.trans_eval_host(n, wo, wi, a, r, m, bg, 1.2, 0.0)
    f1, p1 = path_lib.trans_eval_host(n, wo, wi, a, r, m, 1.0 - bg[::-1], 1.2, 0.0)
    assert np.array_equal(f0.view(np.uint32), f1.view(np.uint32)) and np.array_equal(p0.view(np.uint32), p1.view(np.uint32))
    f2, _ = path_lib.trans_eval_host(n, wo, wi, a, r, m, 1.0 - bg[::-1], 1.2, 0.4)
    f3, _ = path_lib.trans_eval_host(n, wo, wi, a, r, m, bg, 1.2, 0.4)
    assert not np.array_equal(f2, f3)
    lib = path_lib.load()
    assert lib.matpbr_path_trans_eval_host(None, *[None] * 7, 0, None, None) == -1
    for bad in ({"ior": 0.0}, {"spec_trans": 1.5}, {"spec_trans": -0.1}):
        with pytest.raises(ValueError):
            path_lib.trans_eval_host(n, wo, wi, a, r, m, bg, **bad)


# ---- 2. the refracted texel -----------------------------------------------------------------------------------------------------------
def _lookup_lanes(rng, N, H, W):
    """Front-facing lanes: hit points inside and a little outside the frustum, half seen from the camera (wo = -p / |p|), half from
    anywhere above the surface (a bounce vertex)."""
    th = np.tan(np.radians(pf.FOV) / 2)
    z = -rng.uniform(1.5, 3.0, N)
    p = np.stack([rng.uniform(-1.1, 1.1, N) * th * -z, rng.uniform(-1.1, 1.1, N) * th * H / W * -z, z], -1)
    wo = _unit(rng.normal(size=(N, 3)))
    wo[: N // 2] = _unit(-p[: N // 2])
    n = _unit(rng.normal(size=(N, 3)))
    n = np.where(((n * wo).sum(-1) > 0)[:, None], n, -n)
    return _f32(p), _f32(_unit(_f32(n))), _f32(_unit(_f32(wo)))


def test_trans_lookup_host_against_the_restatement(path_lib, oracle64):
    """Texels equal except on at most 1e-4 of 100 k front-facing lanes (fp32 against fp64 at a texel border): 12.5 k lanes at each of
    (24 x 20, 32 x 32) x (D 1, D 100) x (ior 1.2, 1.5)."""
    rng = np.random.default_rng(9)
    total = wrong = tir = 0
    for H, W in ((20, 24), (32, 32)):
        for D in (1.0, 100.0):
            for ior in (1.2, 1.5):
                p, n, wo = _lookup_lanes(rng, 12500, H, W)
                tp, tq = path_lib.trans_lookup_host(p, n, wo, H, W, ior, D)
                rp = pf.texel(oracle64, p, H, W)
                rq = ptf.refracted_texel(oracle64, p, n, wo, ior, D, H, W)
                assert tq.min() >= 0 and tq.max() < H * W and tp.min() >= 0 and tp.max() < H * W
                bad = int((tp != rp).sum() + (tq != rq).sum())
                c = (wo * n).sum(-1)
                t_lanes = ior * ior * (1 - c * c) >= 1                 # total internal reflection of the first refraction
                assert t_lanes.sum() > 1000
                ty, tx = rq // W, rq % W
                inside = (tx > 0) & (tx < W - 1) & (ty > 0) & (ty < H - 1)
                edges = [int((tx == 0).sum()), int((tx == W - 1).sum()), int((ty == 0).sum()), int((ty == H - 1).sum())]
                assert min(edges) > 50, edges                          # lanes whose refracted texel clamps at each image edge
                if D == 1.0:
                    assert inside.sum() > 1000 and (rq != rp)[inside].mean() > 0.5
                print(f"[path trans] lookup {W}x{H} D {D} ior {ior}: {bad} of {2 * p.shape[0]} texels differ; TIR lanes {int(t_lanes.sum())}, clamped at "
                      f"left/right/top/bottom {edges}, inside {int(inside.sum())}")
                total, wrong, tir = total + p.shape[0], wrong + bad, tir + int(t_lanes.sum())
    _report("trans_lookup_host vs fp64: lanes whose texel or refracted texel differs, of lanes (TIR lanes among them)", f"{wrong} of {total} ({tir})")
    assert total == 100000 and wrong <= 1e-4 * total
    # ior 1: the ray goes straight on, 1.3 D along -wo
    p, n, wo = _lookup_lanes(rng, 2000, 32, 32)
    _, tq = path_lib.trans_lookup_host(p, n, wo, 32, 32, 1.0, 1.0)
    assert (tq != pf.texel(oracle64, p - 1.3 * wo, 32, 32)).sum() <= 1


# ---- 3. the GPU parity test's cap, for the restatement alone ---------------------------------------------------------------------------
def test_mask_of_the_gpu_scene():
    for H, W in ((20, 24), (36, 20), (17, 9)):
        mk = ptf.groove_mask(H, W)
        assert (~mk).mean() >= 1 / 3 and mk.mean() > 0.15
        assert mk[int(0.3 * H):, : int(0.45 * W)].all() and mk[2 * H // 3:].any()  # the left wall, and floor below the step
    mk = ptf.groove_mask(20, 24)
    tile = mk[:8, :16]
    assert tile.any() and not tile.all()                               # its border crosses a 16 x 8 tile


def test_restatement_over_fp32_and_fp64_traversal(path_lib, oracle64):
    """The GPU parity test lets 1 % of the pixels differ by more than 1e-3: paths whose hit decisions differ between fp32 and fp64.
    Here the restatement walks once over the library's fp32 traversal and once over the fp64 brute force; the two may differ by more
    than 1e-3 in at most 0.5 % of the pixels of each render, which leaves the kernel the other half of the cap.
    Every render with max_depth above 2 must show a masked vertex, a BSDF sample that leaves below the surface at one, and a masked
    texel read at a bounce vertex.  A max_depth 2 walk ends before it shades its second hit, so it has no bounce vertex, and only its
    camera vertices sample: about 1 % of them leave below the surface (with every pixel masked: 6, 2 and 5 pixels for seeds 0, 1, 2,
    seed 1's both on the right wall), so those three renders must show one between them, not each."""
    s = ptf.trans_scene(path_lib)
    H, W = s["H"], s["W"]
    bvh = path_lib.build_bvh(s["rm"]["vertices"], s["rm"]["triangles"])

    def closest(o, d):
        t, k = path_lib.trace_host(bvh, o, d)
        return np.where(k >= 0, t.astype(np.float64), np.inf), k.astype(np.int64)

    occluded = lambda o, d: path_lib.trace_host(bvh, o, d)[1] >= 0
    worst, below_depth2 = 0.0, 0
    for max_depth, seed, ior, T in ptf.CASES:
        args = (oracle64, s["V"], s["T"], s["a"], s["r"], s["m"], s["env"], s["tab"], H, W, max_depth, seed, s["mask"], s["bg"], ior, T)
        ref, rec = ptf.replay_trans(*args)
        got, _ = ptf.replay_trans(*args, closest=closest, occluded=occluded)
        assert np.isfinite(ref).all() and np.isfinite(got).all()
        err = (np.abs(got - ref) / np.maximum(np.abs(ref), np.abs(ref).mean())).max(-1)
        frac = float((err > 1e-3).mean())
        worst = max(worst, frac)
        bounce = sum(int(v["masked"].sum()) for v in rec["vertices"] if v["depth"] >= 1)
        moved = sum(int((v["tq"] != v["tp"])[v["masked"]].sum()) for v in rec["vertices"])
        print(f"[path trans] max_depth {max_depth} seed {seed} ior {ior} T {T}: {int((err > 1e-3).sum())} pixels differ; masked_vertex "
              f"{int(rec['masked_vertex'].sum())}, below {int(rec['below'].sum())}, masked bounce vertices {bounce}, refracted texel moved {moved}")
        assert frac <= 0.005, (max_depth, seed, frac)
        assert rec["masked_vertex"].any() and moved > 0, (max_depth, seed)
        if max_depth > 2:                                              # the scene does what it is for, in every one of these renders
            assert rec["below"].any() and bounce > 0, (max_depth, seed)
        else:                                                          # max_depth 2: see the docstring
            assert bounce == 0
            below_depth2 += int(rec["below"].sum())
        assert (~rec["masked_vertex"]).sum() >= H * W // 4
    assert below_depth2 > 0
    _report("restatement over fp32 traversal vs fp64 brute force: largest share of pixels that differ by more than 1e-3 (10 renders)", f"{worst:.4f}")


def test_restatement_with_an_empty_mask_is_the_weights_alone(path_lib, oracle64):
    """An all-false mask leaves MatDiffBSDF's values; only the 1e-4 constants of the pdf and the weight differ from path_fp64.replay."""
    s = ptf.trans_scene(path_lib)
    none = np.zeros_like(s["mask"])
    args = (oracle64, s["V"], s["T"], s["a"], s["r"], s["m"], s["env"], s["tab"], s["H"], s["W"], 4, 0)
    x, rec = ptf.replay_trans(*args, none, s["bg"], 1.2, 0.4)
    y, _ = ptf.replay_trans(*args, none, 1 - s["bg"], 1.5, 0.9)
    assert np.array_equal(x, y) and not rec["masked_vertex"].any() and not rec["below"].any()
    plain, _ = pf.replay(*args)
    rel = np.abs(x - plain).max() / plain.mean()
    assert 0 < rel < 0.05, rel


# ---- 4. inputs and the command line -----------------------------------------------------------------------------------------------------
def _best_results(tmp, H=8, W=8):
    from materialist_amd.imageio_exr import write_exr

    br = os.path.join(tmp, "case", "best_results")
    os.makedirs(br)
    one = np.full((H, W, 3), 0.5, np.float32)
    for name in ("albedo", "roughness", "metallic", "normal"):
        write_exr(os.path.join(br, f"{name}.exr"), one)
    return br


def test_load_estimated_brdf_reads_bg(tmp_path):
    import torch
    from PIL import Image

    from materialist_amd import relight

    br = _best_results(str(tmp_path))
    rng = np.random.default_rng(0)
    assert "bg" not in relight.load_estimated_brdf(br, "cpu")
    rgba = rng.integers(0, 256, (8, 8, 4), dtype=np.uint8)           # RGBA at the maps' size: the first three channels over 255
    Image.fromarray(rgba, "RGBA").save(os.path.join(br, "bg.png"))
    bg = relight.load_estimated_brdf(br, "cpu")["bg"]
    assert bg.dtype == torch.float32 and np.array_equal(bg.numpy(), rgba[..., :3].astype(np.float32) / 255.0)
    big = rng.integers(0, 256, (13, 21, 3), dtype=np.uint8)           # another size: bilinear, align_corners=True
    Image.fromarray(big, "RGB").save(os.path.join(br, "bg.png"))
    bg = relight.load_estimated_brdf(br, "cpu")["bg"].numpy()
    assert bg.shape == (8, 8, 3)
    src = big.astype(np.float64) / 255.0
    ref = np.empty((8, 8, 3))
    for i in range(8):
        for j in range(8):
            y, x = i * 12 / 7, j * 20 / 7
            y0, x0 = min(int(y), 11), min(int(x), 19)
            fy, fx = y - y0, x - x0
            ref[i, j] = (src[y0, x0] * (1 - fx) + src[y0, x0 + 1] * fx) * (1 - fy) + (src[y0 + 1, x0] * (1 - fx) + src[y0 + 1, x0 + 1] * fx) * fy
    np.testing.assert_allclose(bg, ref, atol=2e-6)
    assert np.array_equal(bg[0, 0], big[0, 0].astype(np.float32) / 255.0) and np.allclose(bg[-1, -1], big[-1, -1] / 255.0, atol=1e-6)


def test_render_trans_needs_mask_and_bg(tmp_path):
    from PIL import Image

    from materialist_amd import relight

    br = _best_results(str(tmp_path))
    with pytest.raises(FileNotFoundError, match="mask.png"):
        relight.render_trans("case", input_path=str(tmp_path), save_path=str(tmp_path))
    Image.fromarray(np.full((8, 8), 255, np.uint8)).save(os.path.join(br, "mask.png"))
    with pytest.raises(FileNotFoundError, match="bg.png"):
        relight.render_trans("case", input_path=str(tmp_path), save_path=str(tmp_path))


def test_command_line_parses_the_reference_flags(tmp_path):
    import trans_edit

    a = trans_edit.parse_args(["--save_name", "x"])
    assert (a.ior, a.keep_albedo_color, a.specTrans, a.env_path) == (1.2, False, 0.4, None)
    assert (a.spp, a.iters, a.max_depth, a.seed, a.refract_distance, a.input_path, a.save_path) == (64, 10, 4, 0, 100.0, None, None)
    a = trans_edit.parse_args(["--save_name", "x", "--ior", "1.5", "--keep_albedo_color", "--specTrans", "0.8", "--env_path", "e.hdr"])
    assert (a.ior, a.keep_albedo_color, a.specTrans, a.env_path) == (1.5, True, 0.8, "e.hdr")
    # bad arguments end the command before anything touches a GPU (none is visible here), with argparse's exit code
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    cli = [sys.executable, os.path.join(ROOT, "trans_edit.py"), "--save_name", "x", "--input_path", str(tmp_path), "--save_path", str(tmp_path)]
    for bad in (["--ior", "0"], ["--specTrans", "1.5"], ["--max_depth", "17"], ["--iters", "0"]):
        res = subprocess.run(cli + bad, capture_output=True, text=True, timeout=120, env=env)
        assert res.returncode == 2 and bad[0] in res.stderr, res.stdout + res.stderr
    res = subprocess.run([sys.executable, os.path.join(ROOT, "trans_edit.py")], capture_output=True, text=True, timeout=120, env=env)
    assert res.returncode == 2 and "--save_name" in res.stderr
    assert not (tmp_path / "x").exists()
