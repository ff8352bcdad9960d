"""The path render and its backward pass at their edges, against the fp64 restatement (tests/path_fp64.py):
partial tiles and H != W, materials at the pipeline's clamps, envmaps without emitter tables or with zero-probability rows, the LDS
limit of d_env, sample indices above 0 and the division by spp, max_depth 2 and 16, the fixed-point contract of the gradients, and
the 512 x 512 indoor2 mesh (522 k triangles) against an fp64 brute force that does not use the BVH."""
import os
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

KEYS = ("a", "r", "m", "env")


@pytest.fixture(scope="module")
def pt():
    return tl.load(gpu=True)


_report = tl.reporter("path edges", "test_gpu_path_edges")


# ---- configurations ----------------------------------------------------------------------------------------------------------
def _materials(kind, H, W, rng):
    a, r, m = pf.groove_maps(H, W, rng)
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if kind == "r007":
        r[:] = 0.07
    elif kind == "checker":       # every pairing of roughness {0.07, 1} with metallic {0, 1}
        r[..., 0] = np.where((i + j) % 2 == 0, 0.07, 1.0)
        m[..., 0] = np.where((i // 2 + j // 2) % 2 == 0, 0.0, 1.0)
    elif kind == "albedo01":      # albedo channels at 0 and 1, black metal (a = 0, m = 1: the backward pass's kRemFloor guard)
        pick = rng.integers(0, 3, (H, W, 3))
        a = np.where(pick == 0, 0.0, np.where(pick == 1, 1.0, a)).astype(np.float32)
        black = (i + 2 * j) % 4 == 0
        a[black], m[black] = 0.0, 1.0
        m[(i + 2 * j) % 4 == 2] = 1.0
    return a, r, m


def _envmap(kind, rng, sun):
    if kind == "1x1":
        return np.array([[[0.8, 0.7, 0.6]]], np.float32)
    if kind == "zero":
        return np.zeros((8, 16, 3), np.float32)
    if kind == "indoor":          # the pipeline's 16 x 32
        return np.load(os.path.join(ROOT, "tests", "golden", "envmaps.npz"))["indoor"].astype(np.float32)
    if kind in ("32x32", "32x33"):
        env = rng.gamma(2.0, 0.4, (32, int(kind[3:]), 3)).astype(np.float32)
        env[4, 7] = [30.0, 28.0, 25.0]
        return env
    env = pf.groove_env(rng)
    env[1, 3] *= sun / 30.0
    if kind == "lower_black":     # rows of zero probability
        env[env.shape[0] // 2:] = 0.0
    return env


# name -> (H, W, materials, envmap, sun, spp, spp_per_launch, max_depth)
CONFIGS = {
    "21x35": (21, 35, "groove", "groove", 30, 1, 1, 4),
    "20x36": (20, 36, "groove", "groove", 30, 1, 1, 4),
    "36x20": (36, 20, "groove", "groove", 30, 1, 1, 4),
    "r007-sun30": (24, 24, "r007", "groove", 30, 1, 1, 4),
    "r007-sun1000": (24, 24, "r007", "groove", 1000, 1, 1, 4),
    "checker-sun30": (24, 24, "checker", "groove", 30, 1, 1, 4),
    "checker-sun1000": (24, 24, "checker", "groove", 1000, 1, 1, 4),
    "albedo01-sun30": (24, 24, "albedo01", "groove", 30, 1, 1, 4),
    "albedo01-sun1000": (24, 24, "albedo01", "groove", 1000, 1, 1, 4),
    "env1x1": (24, 24, "groove", "1x1", 30, 1, 1, 4),
    "env-zero": (24, 24, "groove", "zero", 30, 1, 1, 4),
    "env-lower-black": (24, 24, "groove", "lower_black", 30, 1, 1, 4),
    "env-indoor-16x32": (24, 24, "groove", "indoor", 30, 1, 1, 4),
    "env32x32": (24, 24, "groove", "32x32", 30, 1, 1, 4),
    "env32x33": (24, 24, "groove", "32x33", 30, 1, 1, 4),
    "spp3": (24, 24, "groove", "groove", 30, 3, 2, 4),
    "depth2": (24, 24, "groove", "groove", 30, 1, 1, 2),
    "depth16": (24, 24, "groove", "groove", 30, 1, 1, 16),
}
SEED = 4
NO_ENV_GRAD = {"env32x33"}            # over the 1024 texels d_env takes


class Cases:
    """Each configuration's scene, GPU results and fp64 references, built on first use and kept for the module."""

    def __init__(self, pt, o64):
        self.pt, self.o64, self.meshes, self.cases = pt, o64, {}, {}

    def mesh(self, H, W):
        from materialist_amd import mesh

        if (H, W) not in self.meshes:
            rm = mesh.reference_mesh(pf.groove_scene(H, W), pf.FOV)
            self.meshes[(H, W)] = (rm, self.pt.PathTracer(rm["vertices"], rm["triangles"], H, W, pf.FOV))
        return self.meshes[(H, W)]

    def __getitem__(self, name):
        if name not in self.cases:
            H, W, mat, envk, sun, spp, spl, depth = CONFIGS[name]
            rm, tracer = self.mesh(H, W)
            rng = np.random.default_rng(11)
            a, r, m = _materials(mat, H, W, rng)
            env = _envmap(envk, rng, sun)
            tab = self.pt.env_tables(env)
            V = rm["vertices"].astype(np.float32).astype(np.float64)
            L, recs = pf.replay_spp(self.o64, V, rm["triangles"], a, r, m, env, tab, H, W, depth, SEED, spp)
            d_out = np.random.default_rng(5).normal(size=(H, W, 3)).astype(np.float32)
            c = {"H": H, "W": W, "a": a, "r": r, "m": m, "env": env, "tab": tab, "spp": spp, "spl": spl, "max_depth": depth,
                 "tracer": tracer, "L": L, "recs": recs, "d_out": d_out, "name": name}
            c["ref"] = self.grad_ref(c, d_out)
            kw = dict(spp=spp, max_depth=depth, seed=SEED, spp_per_launch=spl)
            c["out"] = tracer.render(a, r, m, env, **kw).cpu().numpy().astype(np.float64)
            self.cases[name] = c
        return self.cases[name]

    def grad_ref(self, c, d_out):
        return pf.held_grad(self.o64, c["recs"], *(c[k].astype(np.float64) for k in KEYS), d_out.astype(np.float64))

    def bwd(self, c, d_out, want=KEYS, grads=None):
        kw = dict(spp=c["spp"], max_depth=c["max_depth"], seed=SEED, spp_per_launch=c["spl"])
        got = c["tracer"].render_bwd(c["a"], c["r"], c["m"], c["env"], d_out, want=want, grads=grads, **kw)
        torch.cuda.synchronize()
        return got


@pytest.fixture(scope="module")
def cases(pt, oracle64):
    return Cases(pt, oracle64)


def _parity(got, ref):
    """path_testlib.parity for any leading shape: the errors come back flat, one per element (an image's pixels or a gradient's
    texels; the worst channel).  -> (share of elements within 1e-3 relative to max(|ref|, mean|ref|), the error per element)."""
    scale = np.abs(ref).mean()
    err = (np.abs(got - ref) / np.maximum(np.abs(ref), scale)).reshape(-1, got.shape[-1]).max(-1)
    return float((err <= 1e-3).mean()), err


def _paths_in_parity(c):
    """Pixels whose every sample's path agrees with fp64 in the forward (a path that leaves parity took another branch somewhere,
    and its gradient goes to texels that the fp64 record does not know)."""
    return _parity(c["out"], c["L"])[1] <= 1e-3


# ---- forward and backward parity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CONFIGS))
def test_forward_matches_fp64(cases, name):
    c = cases[name]
    got, ref = c["out"], c["L"]
    assert np.isfinite(got).all()
    if name == "env-zero":
        assert np.all(got == 0.0) and np.all(ref == 0.0)
        return
    frac, err = _parity(got, ref)
    _report(f"{name}: forward, share of pixels within 1e-3", f"{frac:.4f} (max err {err.max():.3e})")
    assert np.abs(ref).max() > 0
    assert frac >= 0.99, (name, frac, np.argwhere(err.reshape(c["H"], c["W"]) > 1e-3)[:10])


@pytest.mark.parametrize("name", list(CONFIGS))
def test_backward_matches_fp64(pt, cases, name):
    c = cases[name]
    want = ("a", "r", "m") if name in NO_ENV_GRAD else KEYS
    got = {k: v.cpu().numpy().astype(np.float64) for k, v in cases.bwd(c, c["d_out"], want=want).items()}
    for key in want:
        assert np.isfinite(got[key]).all(), key
        ref = c["ref"][key]
        if name == "env-zero" and key != "env":   # no light: nothing reaches a material, and not even rounding may
            assert np.all(got[key] == 0.0) and np.all(ref == 0.0), key
            continue
        frac, err = _parity(got[key], ref)
        _report(f"{name}: d_{key}, share of texels within 1e-3", f"{frac:.4f} (max err {err.max():.3e})")
        assert np.abs(ref).max() > 0, key
        assert frac >= 0.99, (name, key, frac, np.argwhere(err > 1e-3)[:10])
    if name == "env-zero":    # d_env from the escaped rays alone: the camera rays that miss and the BSDF rays that escape
        assert all(not v["em"].any() for rec in c["recs"] for v in rec["vertices"])
    if name in NO_ENV_GRAD:
        H, W = c["H"], c["W"]
        He, We = c["env"].shape[:2]
        assert He * We > pt.MAX_BWD_ENV_TEXELS
        with pytest.raises(ValueError, match=r"He \* We <= 1024"):
            cases.bwd(c, c["d_out"])
        # the C entry refuses it too, before any work
        lib = pt.load()
        dev = c["tracer"].device
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
        a, r, m, env = t(c["a"]), t(c["r"]), t(c["m"]), t(c["env"])
        tab = {k: t(c["tab"][k]) for k in ("row_cdf", "col_cdf", "pdf")}
        d_out, d_env, d_a = t(c["d_out"]), torch.full((He, We, 3), 7.0, device=dev), torch.full((H, W, 3), 7.0, device=dev)
        nbytes = int(lib.matpbr_path_render_bwd_workspace_bytes(H, W, He, We))
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        code = lib.matpbr_path_render_bwd(c["tracer"].nodes.data_ptr(), c["tracer"].tris.data_ptr(), a.data_ptr(), r.data_ptr(), m.data_ptr(),
                                          H, W, pf.FOV, env.data_ptr(), tab["row_cdf"].data_ptr(), tab["col_cdf"].data_ptr(),
                                          tab["pdf"].data_ptr(), He, We, 1, 4, SEED, 1, d_out.data_ptr(), d_a.data_ptr(), None, None,
                                          d_env.data_ptr(), ws.data_ptr(), nbytes, None, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
        assert code == -1, code                                  # MATPBR_PATH_ERR_INVALID_ARG
        assert bool((d_env == 7.0).all()) and bool((d_a == 7.0).all())


@pytest.mark.parametrize("name", [n for n in CONFIGS if n not in NO_ENV_GRAD and n != "env-zero"])
def test_envmap_homogeneity(cases, name):
    """With the tables held the render is linear and homogeneous in the texels: sum d_env . env == sum d_out . out (spp 16), a
    global identity that the 1 % allowance of the parity checks cannot hide."""
    c = cases[name]
    tabs = c["tracer"].tables(c["env"])
    kw = dict(spp=16, max_depth=c["max_depth"], seed=9, spp_per_launch=c["spl"], tables=tabs)
    out = c["tracer"].render(c["a"], c["r"], c["m"], c["env"], **kw).cpu().numpy().astype(np.float64)
    d_env = c["tracer"].render_bwd(c["a"], c["r"], c["m"], c["env"], c["d_out"], want=("env",), **kw)["env"].cpu().numpy()
    lhs = float((d_env.astype(np.float64) * c["env"]).sum())
    rhs = float((c["d_out"].astype(np.float64) * out).sum())
    _report(f"{name}: homogeneity, relative difference", f"{abs(lhs - rhs) / abs(rhs):.2e}")
    assert abs(lhs - rhs) <= 1e-5 * abs(rhs), (lhs, rhs)


# ---- the fixed-point contract ("Determinism") ---------------------------------------------------------
FIX_CASE = "albedo01-sun1000"


def _quantum(d_out):
    """q = 2^(e - 24) with max|d_out| < 2^e, as path_bwd_scale_kernel forms it."""
    return 2.0 ** (np.frexp(np.float32(np.abs(d_out).max()))[1] - 24)


def _check_rounding_bound(cases, c, d_out, what):
    """|got - ref| <= n q / (2 spp) + 1e-3 max(|ref|, mean|ref|) for every element, n = the contributions the fp64 record counts.
    d_out is set to 0 on the paths that leave fp64 parity (their terms would go to texels of another path)."""
    d_out = np.where(_paths_in_parity(c).reshape(c["H"], c["W"], 1), d_out, np.float32(0.0)).astype(np.float32)
    got = {k: v.cpu().numpy().astype(np.float64) for k, v in cases.bwd(c, d_out).items()}
    ref = cases.grad_ref(c, d_out)
    q = _quantum(d_out)
    n = pf.contributions(c["recs"])
    worst = {}
    for key in KEYS:
        assert np.isfinite(got[key]).all(), key
        cnt = n["env"] if key == "env" else n["maps"]
        bound = cnt * q / (2 * c["spp"]) + 1e-3 * np.maximum(np.abs(ref[key]), np.abs(ref[key]).mean())
        dev = np.abs(got[key] - ref[key])
        bad = np.argwhere(dev > bound)[:6]
        assert np.all(dev <= bound), (what, key, [(tuple(b), got[key][tuple(b)], ref[key][tuple(b)], bound[tuple(b)], cnt[tuple(b[:-1])])
                                                  for b in bad])
        worst[key] = float((dev / bound).max())
    _report(f"{FIX_CASE} {what}: max |got - ref| / (n q/(2 spp) + 1e-3 scale) for a, r, m, env",
            " / ".join(f"{worst[k]:.3f}" for k in KEYS) + f" (q = 2^{int(np.log2(q))})")
    return q


def test_fixed_point_rounding_bound(cases):
    """d_out with one pixel 2^12 times the rest: the quantum follows the outlier, the other pixels' terms are rounded coarsely; and
    3 x that d_out, whose quantum is not the same power of two times the first."""
    c = cases[FIX_CASE]
    ok = _paths_in_parity(c)
    d_out = c["d_out"].copy()
    lit = np.nonzero(ok & (c["out"].reshape(-1, 3).max(-1) > 0))[0]
    d_out.reshape(-1, 3)[lit[lit.size // 2]] = 4096.0 * np.abs(d_out).max()
    q1 = _check_rounding_bound(cases, c, d_out, "d_out with a 2^12 outlier")
    assert q1 >= 2.0 ** 11 * _quantum(c["d_out"])
    q3 = _check_rounding_bound(cases, c, d_out * np.float32(3.0), "3 x that d_out")
    assert q3 in (2 * q1, 4 * q1)


def test_fixed_point_scaling_and_zero(cases):
    c = cases[FIX_CASE]
    dev = c["tracer"].device
    ref = cases.bwd(c, c["d_out"])
    assert all(bool((ref[k] != 0).any()) for k in KEYS)
    # d_out 2^k: the quantum moves with it, the integer sums do not; every gradient scales exactly
    for k in (-30, -10, 10, 30):
        got = cases.bwd(c, c["d_out"] * np.float32(2.0 ** k))
        for key in KEYS:
            assert torch.equal(got[key], ref[key] * 2.0 ** k), (k, key)
    # d_out = 0: buffers that are added to keep their bits
    base = {k: torch.randn(v.shape, device=dev, generator=torch.Generator(dev).manual_seed(1)) for k, v in ref.items()}
    keep = {k: v.clone() for k, v in base.items()}
    got = cases.bwd(c, np.zeros_like(c["d_out"]), grads=base)
    for key in KEYS:
        assert got[key] is base[key] and torch.equal(got[key].view(torch.int32), keep[key].view(torch.int32)), key


# ---- real size: indoor2 ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def indoor2(pt, golden_dir):
    from materialist_amd import mesh

    z = np.load(os.path.join(golden_dir, "indoor2.npz"))
    a = z["ref_albedo_u8"].astype(np.float32) / 255.0
    r = np.clip(z["ref_roughness_u8"].astype(np.float32)[..., None] / 255.0, 0.07, 1.0)
    m = z["ref_metallic_u8"].astype(np.float32)[..., None] / 255.0
    env = z["ref_envmap_f32"].astype(np.float32)
    depth = z["depth_pred_f32"]
    depth = 2 * depth.max() - depth                                                  # inverse_img_w_mi.py:722
    H, W = depth.shape
    rm = mesh.reference_mesh(depth, pf.FOV)
    tracer = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, pf.FOV)
    # 512 pixels: half at random, half where |grad depth| is largest (creases and silhouettes: the gap-closing triangles)
    gy, gx = np.gradient(depth.astype(np.float64))
    steep = np.argsort(-np.hypot(gx, gy).ravel(), kind="stable")[:256]
    rng = np.random.default_rng(0)
    rest = np.setdiff1d(np.arange(H * W), steep)
    pix = np.concatenate([steep, rng.choice(rest, 256, replace=False)])
    V = rm["vertices"].astype(np.float32).astype(np.float64)
    brute = pf.TorchBrute(V[rm["triangles"]], device=tracer.device)
    return {"a": a, "r": r, "m": m, "env": env, "H": H, "W": W, "tracer": tracer, "pix": pix, "V": V, "T": rm["triangles"],
            "brute": brute, "tab": pt.env_tables(env)}


def test_indoor2_paths_and_gradients_match_fp64(indoor2, oracle64):
    g = indoor2
    H, W, pix = g["H"], g["W"], g["pix"]
    tr = g["tracer"]
    _report("indoor2 BVH (triangles, nodes, depth)", f"{tr.stats['n_tris']}, {tr.stats['n_nodes']}, {tr.stats['depth']}")
    assert tr.stats["depth"] <= 40
    a64, r64, m64, e64 = (g[k].astype(np.float64) for k in ("a", "r", "m", "env"))
    d_out = np.zeros((H, W, 3), np.float32)
    d_out.reshape(-1, 3)[pix] = np.random.default_rng(6).normal(size=(pix.size, 3))
    for seed in (0, 1):
        got = tr.render(g["a"], g["r"], g["m"], g["env"], spp=1, max_depth=4, seed=seed).cpu().numpy().astype(np.float64)
        L, rec = pf.replay(oracle64, g["V"], g["T"], g["a"], g["r"], g["m"], g["env"], g["tab"], H, W, 4, seed, pixels=pix,
                           closest=g["brute"].closest, occluded=g["brute"].occluded)
        frac, err = _parity(got.reshape(-1, 3)[pix], L)
        _report(f"indoor2 seed {seed}: forward, share of the 512 paths within 1e-3", f"{frac:.4f} (max err {err.max():.3e})")
        assert np.isfinite(got).all() and np.abs(L).max() > 0
        assert frac >= 0.99, (seed, frac, pix[err > 1e-3][:10])
        # backward with d_out on those pixels only
        bwd = {k: v.cpu().numpy().astype(np.float64) for k, v in
               tr.render_bwd(g["a"], g["r"], g["m"], g["env"], d_out, spp=1, max_depth=4, seed=seed).items()}
        ref = pf.held_grad(oracle64, rec, a64, r64, m64, e64, d_out.astype(np.float64))
        maps, _ = pf.touched(rec)
        reached = np.array(sorted(set().union(*maps)))
        # every other texel stays exactly 0, except those that only paths leaving parity reach: the kernel's own walk of a flipped
        # path reads texels the fp64 record does not know, so that check runs with d_out on the paths that keep parity
        ok = err <= 1e-3
        d_ok = np.zeros_like(d_out)
        d_ok.reshape(-1, 3)[pix[ok]] = d_out.reshape(-1, 3)[pix[ok]]
        bwd_ok = tr.render_bwd(g["a"], g["r"], g["m"], g["env"], d_ok, spp=1, max_depth=4, seed=seed, want=("a", "r", "m"))
        outside = np.ones(H * W, bool)
        outside[list(set().union(*(maps[q] for q in np.nonzero(ok)[0])))] = False
        for key in ("a", "r", "m"):
            gk, rk = bwd[key].reshape(H * W, -1), ref[key].reshape(H * W, -1)
            assert np.isfinite(gk).all()
            f, e = _parity(gk[reached], rk[reached])
            _report(f"indoor2 seed {seed}: d_{key}, share of the {reached.size} texels reached within 1e-3", f"{f:.4f} (max err {e.max():.3e})")
            assert f >= 0.99, (seed, key, f)
            stray = outside & (bwd_ok[key].cpu().numpy().reshape(H * W, -1) != 0).any(-1)
            assert not stray.any(), (seed, key, np.nonzero(stray)[0][:10])
        f, e = _parity(bwd["env"], ref["env"])
        _report(f"indoor2 seed {seed}: d_env, share of the 512 texels within 1e-3", f"{f:.4f} (max err {e.max():.3e})")
        assert np.isfinite(bwd["env"]).all() and f >= 0.99, (seed, f)
