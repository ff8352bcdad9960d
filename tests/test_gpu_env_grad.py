"""The envmap MLP's gradients and the small-tile kernels under them against fp64 (hot loop A with the reference's light network,
`envhead.EnvMlpPhase`; its sibling `envhead.EnvTexelPhase`).

Adam's first updates are lr * m / sqrt(v): nearly independent of the gradient's magnitude, so the phase tests of tests/test_gpu_parity.py
(weights after a few steps) cannot see a gradient that is off by a factor, a bias gradient that drops a row tile or a weight gradient that
loses a quarter of its rows.  Here every gradient is read directly: `matpbr_mlp_small_bwd_step` launch by launch, the small-tile forms of
`matpbr_mlp_layer_fwd / _bwd_input / _bwd_weight`, `matpbr_env_project[_bwd]`, and the phases' own `gflat`, `d_light`, `g_out`, `g` after
their first iteration.  The references are the plain fp64 torch helpers of tests/env_fp64.py (pinned to autograd on the CPU by
tests/test_env_fp64_host.py).

Bounds.  Every comparison is max |got - ref64| / max |ref64| of a tensor.  Beside the kernel's error e_kernel each
test measures e_torch32: the error of the fp32 torch composition of the same operation (addmm / matmul / autograd on the GPU) against the
same fp64 reference, and asserts
    e_kernel <= max(4 e_torch32, floor),  floor = 4e-6.
The 4 covers the different summation orders (four k-quarters and four m-quarters folded in fixed order here, BLAS's tiling there); the floor
is four times the worst error of the fp32 torch composition of the envmap network's full backward pass against fp64 on a CPU (8.6e-7,
9.1e-7, 9.3e-7, 5.4e-7 of each tensor's maximum at 512, 900, 32 points and the narrow network at 128).  For sin / cos outputs the floor is
the header's contract instead: 1.5 ulp of the result plus the rounding of the pre-activation, |pre| 2^-23.  No bound is taken from the
kernel under test.  Sentinels, zero padding columns, `env == y` above softplus's threshold and refusal codes are exact."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import env_fp64 as ef  # noqa: E402

FLOOR = 4e-6
SENTINEL = 1234.5
INVALID_ARG = -1          # MATPBR_ERR_INVALID_ARG


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.manual_seed(20250629)   # every test draws its random tensors from a fixed stream
    return torch.device("cuda:0")


def _report(what, measured, bound, floor=False):
    """MATPBR_TOLERANCE_REPORT=<file>: one line per comparison -- the test that made it, what was compared, the measured value beside its
    bound and whether it held (the line format of tests/test_gpu_parity.py; how the bounds were set: DESIGN.md section 5)."""
    path = os.environ.get("MATPBR_TOLERANCE_REPORT")
    if path:
        test = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0].split("::", 1)[-1]
        ok = float(measured) >= float(bound) if floor else float(measured) <= float(bound)
        with open(path, "a") as f:
            f.write(f"{test}\t{what}\t{float(measured):.3e}\t{'>=' if floor else '<='}\t{float(bound):.1e}\t{'ok' if ok else 'EXCEEDED'}\n")


def _rel(got, ref):
    return (got.double() - ref).abs().max().item() / (ref.abs().max().item() + 1e-300)


class _Tally:
    """Every comparison of a test is measured, printed and reported before the test asserts on all of them."""

    def __init__(self):
        self.bad = []

    def bounded(self, what, got, ref64, t32, floor=FLOOR):
        assert got.shape == ref64.shape == t32.shape, (what, got.shape, ref64.shape, t32.shape)
        finite = bool(torch.isfinite(got).all())
        e_k, e_t = _rel(got, ref64) if finite else float("inf"), _rel(t32, ref64)
        bound = max(4.0 * e_t, floor)
        print(f"{what}: e_kernel {e_k:.3e}  e_torch32 {e_t:.3e}  bound {bound:.3e}")
        _report(what, e_k, bound)
        _report(what + " [fp32 torch composition]", e_t, float("inf"))
        if not finite:
            self.bad.append(f"{what}: non-finite values")
        elif not e_k <= bound:
            self.bad.append(f"{what}: e_kernel {e_k:.3e} > max(4 x e_torch32 {e_t:.3e}, {floor:.1e})")

    def exact(self, what, cond):
        if not bool(cond):
            self.bad.append(what)

    def done(self):
        assert not self.bad, "\n".join(self.bad)


_al4 = lambda n: (n + 3) // 4 * 4


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _lib():
    from materialist_amd import _lib as L

    return L.load()


def _sent(dev, *shape):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device=dev)


def _kept(buf, written):
    """Every element outside `written` (a bool mask of buf's shape) still holds the sentinel, bit for bit."""
    bits = buf.view(torch.int32)[~written]
    return bool((bits == torch.tensor(SENTINEL, dtype=torch.float32).view(torch.int32).item()).all())


def _mask2(buf, rows, cols):
    m = torch.zeros(buf.shape, dtype=torch.bool, device=buf.device)
    m[:rows, :cols] = True
    return m


# ----------------------------------------------------------------------------------------------------------------------------------
# matpbr_mlp_small_bwd_step launch by launch, and the same shapes through the ordinary entry points
# ----------------------------------------------------------------------------------------------------------------------------------
def _spread(values, n, rng):
    """n draws in which every value occurs (a seeded permutation of the cycled list)."""
    out = [values[i % len(values)] for i in range(n)]
    return [out[i] for i in rng.permutation(n)]


def _step_cases():
    c = []
    # the workload's five launches (13 -> 243 -> 256 -> 243 -> 256 -> 3 on 512 texels), top layer first
    c.append(("workload-out", 512, 3, 256, 256, dict(ldg=4, bias="g")))                         # bias from g itself: 512 groups, tree fold
    c.append(("workload-l3", 512, 256, 256, 243, dict(ldg=256, bias="ws")))
    c.append(("workload-l2", 512, 243, 256, 256, dict(ldg=256, bias="ws")))
    c.append(("workload-l1-tight", 512, 256, 256, 243, dict(ldg=256, bias="ws", tight=True)))  # every stride as envhead's buffers have it
    c.append(("workload-l0", 512, 243, 13, 0, dict(ldg=256, ldx=16, bias="ws")))               # w = NULL
    # ragged rows: 900 -> 29 column-sum groups (8 x 3 + 5: the serial fold's remainder loop), 1024 -> two 128-row batches per wave
    for M in (1, 31, 33, 64, 65, 900, 1000, 1024):
        c.append((f"rows-{M}", M, 256, 256, 256, dict(bias="ws")))
    # the two bias folds: the tree when n_red <= 4 and groups_in > 64, the serial fold otherwise
    c.append(("fold-64x3-serial", 64, 3, 32, 32, dict(ldg=4, bias="g")))
    c.append(("fold-65x3-tree", 65, 3, 32, 32, dict(ldg=4, bias="g")))
    c.append(("fold-200x4-tree", 200, 4, 32, 32, dict(ldg=4, bias="g")))
    c.append(("fold-200x5-serial", 200, 5, 32, 32, dict(ldg=8, bias="g")))
    # ragged reductions and widths: a dozen combinations, every listed value at least once
    rng = np.random.default_rng(20250718)
    Ms = _spread([1, 31, 33, 65, 257, 900], 12, rng)
    Ks = _spread([1, 4, 13, 33, 252, 255, 256], 12, rng)
    nrs = _spread([1, 3, 32, 33, 243], 12, rng)
    nps = _spread([1, 19, 32, 33, 243], 12, rng)
    for i in range(12):
        c.append((f"ragged-{Ms[i]}x{nrs[i]}x{Ks[i]}x{nps[i]}", Ms[i], nrs[i], Ks[i], nps[i], dict(bias="g" if i % 2 else "ws", ldx=_al4(Ks[i]))))
    return c


_STEP_CASES = _step_cases()


def _step_inputs(dev, M, n_red, K, n_prev, opt, seed):
    """Inputs of one backward step with every padding region NaN: g (order 1e-3, one all-zero row tile where there are two or more tiles),
    x (sine-like, one column of magnitude ~30: the positional code's raw coordinates), the forward weight w and c_prev in [-1, 1]."""
    gen = torch.Generator().manual_seed(seed)
    nan = float("nan")
    tight = opt.get("tight", False)
    ldg = opt.get("ldg", _al4(n_red) + 4)
    ldx = opt.get("ldx", _al4(K) if tight else _al4(K) + 4)
    d = dict(M=M, n_red=n_red, K=K, n_prev=n_prev, ldg=ldg, ldx=ldx)
    g = torch.full((M, ldg), nan)
    g[:, :n_red] = 1e-3 * torch.randn(M, n_red, generator=gen)
    if M >= 64:
        g[32:64, :n_red] = 0.0
    x = torch.full((M, ldx), nan)
    x[:, :K] = torch.sin(3.0 * torch.randn(M, K, generator=gen))
    x[:, 0] = 30.0 * (torch.rand(M, generator=gen) * 2 - 1)
    d["g"], d["x"] = g.to(dev), x.to(dev)
    if n_prev:
        ld = d["ld"] = _al4(n_prev) if tight else _al4(n_prev) + 4
        w = torch.full((n_red, ld), nan)
        w[:, :n_prev] = (torch.rand(n_red, n_prev, generator=gen) * 2 - 1) / n_red ** 0.5
        c = torch.full((M, ld), nan)
        c[:, :n_prev] = torch.rand(M, n_prev, generator=gen) * 2 - 1
        d["w"], d["c"] = w.to(dev), c.to(dev)
    groups = (M + 31) // 32
    if opt["bias"] == "ws":      # what the launch before left: per-tile column sums of g in a [groups, 256] workspace (fp32 roundings of the fp64 sums)
        ws = torch.full((groups, 256), nan)
        g64 = g[:, :n_red].double()
        ws[:, :n_red] = torch.stack([g64[r:r + 32].sum(0) for r in range(0, M, 32)]).float()
        d["bias_src"], d["bias_stride"], d["bias_groups"] = ws.to(dev), 256, groups
    else:
        d["bias_src"], d["bias_stride"], d["bias_groups"] = d["g"], ldg, M
    return d


def _call_step(dev, g, ldg, w, ldw, c, gp, ldo, cs_out, n_prev, x, ldx, dw, ldw_out, K, cs_in, cs_stride, groups_in, d_bias, M, n_red):
    with torch.cuda.device(dev):
        return _lib().matpbr_mlp_small_bwd_step(_P(g), ldg, _P(w), ldw, _P(c), _P(gp), ldo, _P(cs_out), n_prev, _P(x), ldx, _P(dw), ldw_out, K,
                                                _P(cs_in), cs_stride, groups_in, _P(d_bias), M, n_red, _stream(dev))


@pytest.mark.parametrize("case", _STEP_CASES, ids=[c[0] for c in _STEP_CASES])
def test_small_bwd_step_matches_fp64(case):
    """One launch of `matpbr_mlp_small_bwd_step` against `bwd_step64`: d_w, g_prev, the per-row-tile column sums and d_bias, with NaN in
    every padding column of the inputs and sentinels in output buffers that are larger than the outputs (extra rows, wider strides): the
    outputs are finite and within the bound, and nothing outside the documented outputs is written."""
    name, M, n_red, K, n_prev, opt = case
    dev = _cuda()
    d = _step_inputs(dev, M, n_red, K, n_prev, opt, seed=1000 + _STEP_CASES.index(case))
    tight = opt.get("tight", False)
    tiles = (M + 31) // 32
    ldw_out = _al4(K) if tight else _al4(K) + 4
    dw = _sent(dev, n_red + 2, ldw_out)
    d_bias = _sent(dev, n_red + 5)
    gp = cs = None
    if n_prev:
        gp, cs = _sent(dev, M + 3, d["ld"]), _sent(dev, tiles + 2, 256)
    code = _call_step(dev, d["g"], d["ldg"], d.get("w"), d.get("ld", 0), d.get("c"), gp, d.get("ld", 0), cs, n_prev, d["x"], d["ldx"], dw, ldw_out, K,
                      d["bias_src"], d["bias_stride"], d["bias_groups"], d_bias, M, n_red)
    torch.cuda.synchronize()
    assert code == 0, code
    g32, x32 = d["g"][:, :n_red].contiguous(), d["x"][:, :K].contiguous()
    w32 = d["w"][:, :n_prev].contiguous() if n_prev else None
    c32 = d["c"][:, :n_prev].contiguous() if n_prev else None
    r_dw, r_gp, r_cs, _ = ef.bwd_step64(g32.double(), w32.double() if n_prev else None, c32.double() if n_prev else None, x32.double())
    t_dw, t_gp, t_cs, _ = ef.bwd_step64(g32, w32, c32, x32)                                    # the same composition in fp32 (BLAS)
    src = d["bias_src"][:d["bias_groups"], :n_red]
    ta = _Tally()
    ta.bounded(f"{name} d_w", dw[:n_red, :K], r_dw, t_dw)
    ta.bounded(f"{name} d_bias", d_bias[:n_red], src.double().sum(0), src.sum(0))
    ta.exact(f"{name}: d_w wrote outside [n_red, K]", _kept(dw, _mask2(dw, n_red, K)))
    ta.exact(f"{name}: d_bias wrote beyond n_red", _kept(d_bias, torch.arange(n_red + 5, device=dev) < n_red))
    if n_prev:
        ta.bounded(f"{name} g_prev", gp[:M, :n_prev], r_gp, t_gp)
        ta.bounded(f"{name} colsum_out", cs[:tiles, :n_prev], r_cs, t_cs)
        ta.exact(f"{name}: g_prev wrote outside [M, n_prev]", _kept(gp, _mask2(gp, M, n_prev)))
        ta.exact(f"{name}: colsum_out wrote outside [tiles, n_prev]", _kept(cs, _mask2(cs, tiles, n_prev)))
    ta.done()


@pytest.mark.parametrize("case", _STEP_CASES, ids=[c[0] for c in _STEP_CASES])
def test_small_tile_entry_points_match_fp64(case):
    """The same shapes once through `ops.mlp_layer_fwd` (sin / cos and the `c_out = None` bias form), `ops.mlp_layer_bwd_input` (with its
    d_bias) and `ops.mlp_layer_bwd_weight` at M <= 1024, NaN in every padding column.  sin / cos are compared with sin / cos of the fp64
    pre-activation (|pre| stays below ~100)."""
    from materialist_amd import ops

    name, M, n_red, K, n_prev, opt = case
    dev = _cuda()
    d = _step_inputs(dev, M, n_red, K, n_prev, opt, seed=1000 + _STEP_CASES.index(case))
    g32, x32 = d["g"][:, :n_red].contiguous(), d["x"][:, :K].contiguous()
    ta = _Tally()
    # weight gradient
    dw = ops.mlp_layer_bwd_weight(d["g"], d["x"], n_red, K)
    ta.bounded(f"{name} bwd_weight d_w", dw, g32.double().t() @ x32.double(), g32.t() @ x32)
    # input gradient with the bias gradient of the layer below: wt = w^T [n_prev, n_red], padded with NaN
    if n_prev:
        w32, c32 = d["w"][:, :n_prev].contiguous(), d["c"][:, :n_prev].contiguous()
        wt = torch.full((n_prev, _al4(n_red) + 4), float("nan"), device=dev)
        wt[:, :n_red] = w32.t()
        gp, db = _sent(dev, M, d["ld"]), _sent(dev, n_prev)
        ops.mlp_layer_bwd_input(d["g"], wt, d["c"], gp, n_prev, n_red, db)
        r_gp, t_gp = (g32.double() @ w32.double()) * c32.double(), (g32 @ w32) * c32
        ta.bounded(f"{name} bwd_input g_prev", gp[:, :n_prev], r_gp, t_gp)
        ta.bounded(f"{name} bwd_input d_bias_prev", db, r_gp.sum(0), t_gp.sum(0))
    # forward: a layer x[M, K] -> N = n_red outputs
    gen = torch.Generator().manual_seed(77 + _STEP_CASES.index(case))
    wf = torch.full((n_red, d["ldx"]), float("nan"))
    wf[:, :K] = (torch.rand(n_red, K, generator=gen) * 2 - 1) / K ** 0.5
    wf, b = wf.to(dev), (torch.rand(n_red, generator=gen) * 2 - 1).to(dev)
    ldo = _al4(n_red) + 4
    s, c, lin = _sent(dev, M, ldo), _sent(dev, M, ldo), _sent(dev, M, ldo)
    ops.mlp_layer_fwd(d["x"], wf, b, s, c, K)
    ops.mlp_layer_fwd(d["x"], wf, b, lin, None, K)
    torch.cuda.synchronize()
    pre64 = x32.double() @ wf[:, :K].double().t() + b.double()
    pre32 = torch.addmm(b, x32, wf[:, :K].t())
    pmax = pre64.abs().max().item()
    assert pmax < 100.0, pmax
    fl_s = (1.5 * 2.0 ** -24 + pmax * 2.0 ** -23) / (torch.sin(pre64).abs().max().item() + 1e-300)
    fl_c = (1.5 * 2.0 ** -24 + pmax * 2.0 ** -23) / (torch.cos(pre64).abs().max().item() + 1e-300)
    ta.bounded(f"{name} fwd sin", s[:, :n_red], torch.sin(pre64), torch.sin(pre32), floor=fl_s)
    ta.bounded(f"{name} fwd cos", c[:, :n_red], torch.cos(pre64), torch.cos(pre32), floor=fl_c)
    ta.bounded(f"{name} fwd bias form", lin[:, :n_red], pre64, pre32)
    ta.done()


def test_small_bwd_step_refuses_bad_arguments_and_launches_nothing():
    dev = _cuda()
    M, n_red, K, n_prev = 64, 8, 16, 12
    d = _step_inputs(dev, M, n_red, K, n_prev, dict(bias="g"), seed=5)
    big = _step_inputs(dev, 1025, n_red, K, n_prev, dict(bias="g"), seed=6)
    dw, db, gp, cs = _sent(dev, n_red, 32), _sent(dev, n_red), _sent(dev, 1025, d["ld"]), _sent(dev, 40, 256)

    def call(dd=d, **kw):
        a = dict(g=dd["g"], ldg=dd["ldg"], w=dd["w"], ldw=dd["ld"], c=dd["c"], gp=gp, ldo=dd["ld"], cs_out=cs, n_prev=n_prev, x=dd["x"], ldx=dd["ldx"], dw=dw,
                 ldw_out=32, K=K, cs_in=dd["bias_src"], cs_stride=dd["bias_stride"], groups_in=dd["bias_groups"], d_bias=db, M=dd["M"], n_red=n_red)
        a.update(kw)
        return _call_step(dev, *[a[k] for k in ("g", "ldg", "w", "ldw", "c", "gp", "ldo", "cs_out", "n_prev", "x", "ldx", "dw", "ldw_out", "K", "cs_in",
                                                "cs_stride", "groups_in", "d_bias", "M", "n_red")])

    refused = {
        "M = 1025": call(dd=big),
        "ldg not a multiple of 4": call(ldg=d["ldg"] + 1),
        "ldx < ceil4(K)": call(K=14, ldx=12),
        "ldw_out < K": call(ldw_out=K - 1),
        "d_bias without colsum_in": call(cs_in=None),
        "w without g_prev": call(gp=None),
    }
    torch.cuda.synchronize()
    assert refused == {k: INVALID_ARG for k in refused}, refused
    for buf in (dw, db, gp, cs):
        assert _kept(buf, torch.zeros(buf.shape, dtype=torch.bool, device=dev))
    assert call() == 0                                        # the same arguments without a fault are accepted
    torch.cuda.synchronize()
    assert not _kept(dw, torch.zeros(dw.shape, dtype=torch.bool, device=dev))


def test_small_bwd_step_column_sums_feed_the_next_launch():
    """Two launches of a two-layer toy chain on alternating workspaces, as `envhead` drives them: the column sums the upper launch leaves are
    the lower launch's `colsum_in`, and the lower layer's bias gradient is the fp64 column sum of its g."""
    dev = _cuda()
    M, n2, n1, n0 = 900, 3, 243, 64
    top = _step_inputs(dev, M, n2, n1, n1, dict(ldg=4, bias="g"), seed=21)           # output layer: x = the sines of layer 1 [M, n1]
    low = _step_inputs(dev, M, n1, n0, n0, dict(ldg=256, bias="g"), seed=22)         # its g is replaced by the upper launch's g_prev
    tiles = (M + 31) // 32
    ws = [_sent(dev, tiles + 1, 256), _sent(dev, tiles + 1, 256)]
    g1 = _sent(dev, M, top["ld"])
    dw2, db2 = _sent(dev, n2, _al4(n1)), _sent(dev, n2)
    assert _call_step(dev, top["g"], 4, top["w"], top["ld"], top["c"], g1, top["ld"], ws[0], n1, top["x"], top["ldx"], dw2, _al4(n1), n1,
                      top["g"], 4, M, db2, M, n2) == 0
    g0 = _sent(dev, M, low["ld"])
    dw1, db1 = _sent(dev, n1, _al4(n0)), _sent(dev, n1 + 3)
    assert _call_step(dev, g1, top["ld"], low["w"], low["ld"], low["c"], g0, low["ld"], ws[1], n0, low["x"], low["ldx"], dw1, _al4(n0), n0,
                      ws[0], 256, tiles, db1, M, n1) == 0
    torch.cuda.synchronize()
    g2_32, w2, c1 = top["g"][:, :n2].contiguous(), top["w"][:, :n1].contiguous(), top["c"][:, :n1].contiguous()
    r_g1 = (g2_32.double() @ w2.double()) * c1.double()
    t_g1 = (g2_32 @ w2) * c1
    ta = _Tally()
    ta.bounded("chain d_bias of the lower layer vs fp64 column sums of its fp64 g", db1[:n1], r_g1.sum(0), t_g1.sum(0))
    ta.bounded("chain d_bias of the lower layer vs fp64 column sums of the g the kernel wrote", db1[:n1], g1[:, :n1].double().sum(0), g1[:, :n1].sum(0))
    ta.bounded("chain d_bias of the output layer", db2, g2_32.double().sum(0), g2_32.sum(0))
    x1 = low["x"][:, :n0].contiguous()
    ta.bounded("chain d_w of the lower layer", dw1[:, :n0], g1[:, :n1].double().t() @ x1.double(), g1[:, :n1].contiguous().t() @ x1)
    ta.exact("chain: d_bias wrote beyond n1", _kept(db1, torch.arange(n1 + 3, device=dev) < n1))
    ta.exact("chain: workspace 0 wrote outside [tiles, n1]", _kept(ws[0], _mask2(ws[0], tiles, n1)))
    ta.exact("chain: workspace 1 wrote outside [tiles, n0]", _kept(ws[1], _mask2(ws[1], tiles, n0)))
    ta.done()


# ----------------------------------------------------------------------------------------------------------------------------------
# matpbr_env_project / matpbr_env_project_bwd
# ----------------------------------------------------------------------------------------------------------------------------------
_PLANTED = (-100.0, -30.0, -1e-3, 0.0, 19.999, 20.0, 20.001, 50.0)


@pytest.mark.parametrize("grid", [(4, 8), (8, 16), (16, 32), (30, 30), (32, 32)], ids=lambda g: f"{g[0]}x{g[1]}")
def test_env_project_and_its_backward_match_fp64(grid):
    """softplus (torch's threshold at 20) + SH projection and their backward: a random body of order 1 with values planted around the
    threshold and far in both tails, NaN in the padding column of y."""
    from materialist_amd import sh

    dev = _cuda()
    lib = _lib()
    T = grid[0] * grid[1]
    proj = torch.from_numpy(sh.envmap_to_sh_matrix(*grid)).to(dev, torch.float32).contiguous()
    y = torch.randn(T, 4, device=dev)
    where = [((3 + 4 * i) % T, i % 3) for i in range(len(_PLANTED))]
    for (t, c), v in zip(where, _PLANTED):
        y[t, c] = v
    y[:, 3] = float("nan")
    d_light = torch.randn(25, 3, device=dev)
    env, light, d_y, d_y1 = _sent(dev, T + 2, 3), _sent(dev, 26, 3), _sent(dev, T + 2, 4), _sent(dev, T + 2, 4)
    y_big = torch.full_like(y, 50.0)                            # derivative 1 in every element: the projection's own sums
    with torch.cuda.device(dev):
        assert lib.matpbr_env_project(_P(y), 4, _P(proj), _P(env), _P(light), T, _stream(dev)) == 0
        assert lib.matpbr_env_project_bwd(_P(y), 4, _P(proj), _P(d_light), _P(d_y), 4, T, _stream(dev)) == 0
        assert lib.matpbr_env_project_bwd(_P(y_big), 4, _P(proj), _P(d_light), _P(d_y1), 4, T, _stream(dev)) == 0
    torch.cuda.synchronize()
    y3 = y[:, :3].contiguous()
    r_env, r_light = ef.project64(y3.double(), proj.double())
    t_env, t_light = ef.project64(y3, proj)
    r_dy, t_dy = ef.project_bwd64(y3.double(), proj.double(), d_light.double()), ef.project_bwd64(y3, proj, d_light)
    ta = _Tally()
    ta.bounded(f"project {T} env", env[:T], r_env, t_env)
    ta.bounded(f"project {T} light", light[:25], r_light, t_light)
    ta.bounded(f"project {T} d_y", d_y[:T, :3], r_dy, t_dy)
    above = y3 > 20
    assert int(above.sum()) == 2
    ta.exact("d_y's padding column is not exactly zero", (d_y[:T, 3] == 0).all())
    ta.exact("the derivative above the threshold is not exactly 1", torch.equal(d_y[:T, :3][above], d_y1[:T, :3][above]))
    ta.exact("below the threshold the derivative is not below 1", (d_y[:T, :3][~above].abs() <= d_y1[:T, :3][~above].abs()).all())
    ta.exact("env != y above the threshold", torch.equal(env[:T][above], y3[above]))
    ta.exact("env negative or non-finite", (torch.isfinite(env[:T]) & (env[:T] >= 0)).all())
    ta.exact("env wrote beyond T rows", _kept(env, _mask2(env, T, 3)))
    ta.exact("light wrote beyond 25 rows", _kept(light, _mask2(light, 25, 3)))
    ta.exact("d_y wrote beyond T rows", _kept(d_y, _mask2(d_y, T, 4)))
    ta.done()


# ----------------------------------------------------------------------------------------------------------------------------------
# the phases' own gradients after their first iteration
# ----------------------------------------------------------------------------------------------------------------------------------
_H = _W = 48
_SPP = 8
_scene_cache = {}


def _scene(dev):
    """make_scene() and the target image, once per session."""
    if "s" not in _scene_cache:
        from materialist_amd import render, synthetic

        sc = synthetic.make_scene(8, _H, _W)
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)

        def make():
            s = render.load_estimated_mesh(t(sc.depth), use_mesh_normal=True)
            p = render.traverse(s)
            p["shape.bsdf.a"], p["shape.bsdf.r"], p["shape.bsdf.m"] = t(sc.albedo), t(sc.roughness), t(sc.metallic)
            return s

        with torch.no_grad():
            gt = render.render_envmap(make(), t(sc.light), _SPP).clone()
        _scene_cache["s"] = (make, gt)
    return _scene_cache["s"]


def _dense_transfer(T, dev):
    """The radiance transfer as a dense fp32 map light[25, 3] -> image: `ops.relight` under the unit lights (one per coefficient and channel,
    so nothing is assumed about how the channels couple).  relight is linear in the light (tests/test_gpu_parity.py)."""
    from materialist_amd import ops

    eye = torch.eye(75, device=dev).reshape(75, 25, 3).contiguous()
    return ops.relight(T, eye, _H, _W).reshape(25, 3, _H, _W, 3).clone()


def _render_loss(D, light, gt):
    from materialist_amd import loss

    pred = torch.einsum("kchwd,kc->hwd", D, light)
    return loss.env_loss(pred, gt)


_PHASE_CFGS = [("16x32", (16, 32), {}), ("30x30", (30, 30), {}), ("4x8", (4, 8), {}), ("8x16-narrow", (8, 16), dict(hidden=(64, 128, 64), skip=(2,)))]
_phase_cache = {}


def _phase(dev, cfg):
    """One first iteration of `EnvMlpPhase` (no graph) and the fp64 / fp32 torch references of everything it leaves, computed once."""
    name, grid, kw = cfg
    if name in _phase_cache:
        return _phase_cache[name]
    from materialist_amd import ops, posmlp
    from materialist_amd.envhead import EnvMlpPhase

    make, gt = _scene(dev)
    M = grid[0] * grid[1]
    torch.manual_seed(3)
    net = posmlp.envmap_net(**kw).to(dev)
    getattr(net, f"lin{net.n_layers - 1}").weight.data.normal_(0, 0.05)      # the reference zero-initialises the last layer
    net0 = copy.deepcopy(net)                                                # the module as it is before the step
    start = torch.ones(M, 3, device=dev)
    ph = EnvMlpPhase(make(), gt, net, start, spp=_SPP, lr=1e-3, use_graph=False, env_size=grid)
    ph.step()
    torch.cuda.synchronize()
    r = dict(ph=ph, skip=net0.skip)
    # the gradient buffer through the views EnvMlpPhase builds: (weight [n, al4(k)], bias [al4(n)]) per layer
    lins = ef.layers_of(net0)
    r["names"] = [n for n, _ in lins]
    gviews, off = [], 0
    for wp, bp in ph.views:
        gw = ph.gflat[off:off + wp.numel()].view_as(wp)
        off += wp.numel()
        gb = ph.gflat[off:off + _al4(bp.numel())]
        off += _al4(bp.numel())
        gviews.append((gw, gb))
    assert off == ph.gflat.numel()
    r["gviews"] = gviews
    D32 = _dense_transfer(ph.T, dev)
    x0 = net0._points(start)
    refs = {}
    for dt in (torch.float64, torch.float32):
        ws = [lin.weight.detach().to(dt).clone().requires_grad_(True) for _, lin in lins]
        bs = [lin.bias.detach().to(dt).clone().requires_grad_(True) for _, lin in lins]
        proj, D, g_t = ph.proj.to(dt), D32.to(dt), ph.gt.to(dt)
        o = {}
        # a. the network chain in isolation: the kernel's own d_light as the upstream
        y, _, _ = ef.forward64(ws, bs, net0.skip, x0.to(dt))
        y.retain_grad()
        (ef.project64(y, proj)[1] * ph.d_light.to(dt)).sum().backward()
        o["a_dy"] = y.grad.clone()
        o["a"] = [(w.grad.clone(), b.grad.clone()) for w, b in zip(ws, bs)]
        o["y"] = y.detach()
        for t in ws + bs:
            t.grad = None
        # b. the light gradient: the kernel's own light through the dense transfer and env_loss
        light = ph.light.to(dt).clone().requires_grad_(True)
        total, mse, _ = _render_loss(D, light, g_t)
        total.backward()
        o["b_dlight"], o["b_mse"], o["b_loss"] = light.grad.clone(), mse.detach().reshape(1), total.detach().reshape(1)
        # c. end to end: module -> softplus -> projection -> dense transfer -> env_loss
        y, _, _ = ef.forward64(ws, bs, net0.skip, x0.to(dt))
        total, _, _ = _render_loss(D, ef.project64(y, proj)[1], g_t)
        total.backward()
        o["c"] = [(w.grad.clone(), b.grad.clone()) for w, b in zip(ws, bs)]
        refs[dt] = o
    # chain64 itself (what the CPU test pins) agrees with the autograd reference used above
    net64 = copy.deepcopy(net0).double()
    c64 = ef.chain64(net64, x0.double(), ef.project_bwd64(refs[torch.float64]["y"], ph.proj.double(), ph.d_light.double()))
    for n, (gw, gb) in zip(r["names"], refs[torch.float64]["a"]):
        assert (c64[n + ".weight"] - gw).abs().max().item() <= 1e-10 * gw.abs().max().item()
        assert (c64[n + ".bias"] - gb).abs().max().item() <= 1e-10 * gb.abs().max().item()
    r["r64"], r["r32"] = refs[torch.float64], refs[torch.float32]
    _phase_cache[name] = r
    return r


def _compare_gflat(ta, tag, r, key):
    for l, (name, (gw, gb)) in enumerate(zip(r["names"], r["gviews"])):
        (w64, b64), (w32, b32) = r["r64"][key][l], r["r32"][key][l]
        n, k = w64.shape
        ta.bounded(f"{tag} {name}.weight", gw[:, :k], w64, w32)
        ta.bounded(f"{tag} {name}.bias", gb[:n], b64, b32)
        ta.exact(f"{tag} {name}.weight: padding columns of gflat are not exactly zero", (gw[:, k:] == 0).all())
        ta.exact(f"{tag} {name}.bias: padding entries of gflat are not exactly zero", (gb[n:] == 0).all())


@pytest.mark.parametrize("cfg", _PHASE_CFGS, ids=[c[0] for c in _PHASE_CFGS])
def test_env_mlp_phase_network_chain_matches_fp64(cfg):
    """a. From the kernel's own `d_light`: `g_out` against `project_bwd64` and every parameter's slice of `gflat` against `chain64` on the
    fp64 copy of the module as it was before the step; padding entries exactly zero."""
    dev = _cuda()
    r = _phase(dev, cfg)
    ph, ta = r["ph"], _Tally()
    ta.bounded(f"{cfg[0]} chain g_out", ph.g_out[:, :3], r["r64"]["a_dy"], r["r32"]["a_dy"])
    ta.exact("g_out's padding column is not exactly zero", (ph.g_out[:, 3] == 0).all())
    _compare_gflat(ta, f"{cfg[0]} chain", r, "a")
    ta.done()


@pytest.mark.parametrize("cfg", _PHASE_CFGS, ids=[c[0] for c in _PHASE_CFGS])
def test_env_mlp_phase_light_gradient_matches_fp64(cfg):
    """b. `d_light` and the loss statistics against fp64 autograd of `env_loss` over the dense transfer, from the kernel's own light."""
    from materialist_amd import ops

    dev = _cuda()
    r = _phase(dev, cfg)
    ph, ta = r["ph"], _Tally()
    ta.bounded(f"{cfg[0]} d_light", ph.d_light, r["r64"]["b_dlight"], r["r32"]["b_dlight"])
    ta.bounded(f"{cfg[0]} stats mse", ph.stats[0, ops.STAT_MSE].reshape(1), r["r64"]["b_mse"], r["r32"]["b_mse"])
    ta.bounded(f"{cfg[0]} stats loss", ph.stats[0, ops.STAT_LOSS].reshape(1), r["r64"]["b_loss"], r["r32"]["b_loss"])
    ta.done()


@pytest.mark.parametrize("cfg", _PHASE_CFGS, ids=[c[0] for c in _PHASE_CFGS])
def test_env_mlp_phase_gradients_match_fp64_end_to_end(cfg):
    """c. `gflat` against fp64 autograd of the whole composition: module -> softplus -> projection -> dense transfer -> env_loss."""
    dev = _cuda()
    r = _phase(dev, cfg)
    ta = _Tally()
    _compare_gflat(ta, f"{cfg[0]} end to end", r, "c")
    ta.done()


def test_env_texel_phase_gradient_matches_fp64():
    """d. `EnvTexelPhase.g` after the first iteration (same scene, 16 x 32 texels): the unfused tail against `project_bwd64` of the fp64 light
    gradient, padding column exactly zero, and the fused tail the same bits."""
    from materialist_amd.envhead import EnvTexelPhase

    dev = _cuda()
    make, gt = _scene(dev)
    torch.manual_seed(2)
    raw0 = torch.randn(16, 32, 3, device=dev) * 0.3
    g, ph = {}, None
    for fused in (False, True):
        EnvTexelPhase.FUSED_TAIL = fused
        try:
            ph = EnvTexelPhase(make(), gt, raw0.clone().requires_grad_(True), spp=_SPP, lr=1e-2, use_graph=False)
        finally:
            EnvTexelPhase.FUSED_TAIL = True
        assert ph.fused_tail == fused
        ph.step()
        torch.cuda.synchronize()
        g[fused] = ph.g.clone()
    D32 = _dense_transfer(ph.T, dev)
    ref = {}
    for dt in (torch.float64, torch.float32):
        y = raw0.reshape(-1, 3).to(dt).clone().requires_grad_(True)
        proj = ph.proj.to(dt)
        light = ef.project64(y, proj)[1].detach().requires_grad_(True)
        _render_loss(D32.to(dt), light, ph.gt.to(dt))[0].backward()
        ref[dt] = ef.project_bwd64(y.detach(), proj, light.grad)
    ta = _Tally()
    ta.bounded("texel phase g (unfused tail)", g[False][:, :3], ref[torch.float64], ref[torch.float32])
    ta.exact("g's padding column is not exactly zero", (g[False][:, 3] == 0).all())
    ta.exact("the fused tail's g differs from the unfused tail's", torch.equal(g[True], g[False]))
    ta.done()
