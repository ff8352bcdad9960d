"""The cache plan of the f16 backward pass (`ops.mlp_set_cache_plan`) changes where bytes live, never a value.

The backward sequence of `ArmMlpPhase.backward` -- output layer, three weight gradients, two input gradients, the first-layer form and the one
fold launch -- on M = 2048 rows (16 tiles; 8 weight-gradient workgroups of 2 tiles) runs once with the plan off and once per budget with it on:
a few KB (every stream takes the streaming policy), 5 MiB (every threshold falls inside the 16 tiles: the last 8 tiles of the input gradients'
stores, the first 4 / 6 tiles of the loads at their last use keep the default policy, the partial sums stream -- both instruction forms in one
launch) and 1 TiB (nothing streams).
Every output is the same bits as with the plan off.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

M = 2048
CASES = {"wide": [256, 256, 256, 256], "ragged": [241, 256, 241, 256]}     # columns of the four sine layers (241: a skip layer, x0 in its tail)
BUDGETS = {"all_streamed": 4096, "threshold_inside": 5 << 20, "nothing_streamed": 1 << 40}
_inputs, _reference = {}, {}


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _make_inputs(case):
    """Made once per case on the CPU from a fixed seed and left unchanged.  d_x: the loss gradient of the five outputs, 1e-6 with tile magnitudes
    spread over 1e4 and one all-zero tile (the recipe of test_block_scaled_f16_backward_products); sines that carry the sign of their cosine in
    their last mantissa bit (`pack_cos_sign`), the tail of a 241-column layer holding coordinates."""
    if case not in _inputs:
        ns = CASES[case]
        rng = np.random.default_rng(4000 + sum(ns))
        T = M // 128
        mag = np.clip(np.exp(rng.standard_normal(T) * 2.0), 1e-2, 1e2).astype(np.float32)
        d_x = np.zeros((M, 8), dtype=np.float32)
        d_x[:, :5] = rng.standard_normal((M, 5), dtype=np.float32) * np.float32(1e-6) * np.repeat(mag, 128)[:, None]
        d_x[128 * 5:128 * 6] = 0.0
        x0 = np.zeros((M, 16), dtype=np.float32)
        x0[:, :15] = rng.standard_normal((M, 15), dtype=np.float32)
        x0[:, 0] = rng.integers(0, 512, M).astype(np.float32)
        sines = []
        for n in ns:
            pre = rng.standard_normal((M, 256)) * 3.0
            s = np.sin(pre).astype(np.float32)
            bits = s.view(np.uint32)
            bits &= np.uint32(0xFFFFFFFE)
            bits |= (np.cos(pre) < 0).astype(np.uint32)
            if n < 256:
                s[:, n:] = x0[:, :256 - n]
            sines.append(s)
        weights = [((rng.random((256, 256), dtype=np.float32) * 2 - 1) / 16).astype(np.float32) for _ in ns]
        w_out = ((rng.random((5, 256), dtype=np.float32) * 2 - 1) / 16).astype(np.float32)
        _inputs[case] = {"d_x": torch.from_numpy(d_x), "x0": torch.from_numpy(x0), "sines": [torch.from_numpy(s) for s in sines],
                         "weights": [torch.from_numpy(w) for w in weights], "w_out": torch.from_numpy(w_out)}
    return _inputs[case]


def _backward(case, dev):
    """One backward pass under the current plan: every gradient matrix, the tile maxima and every folded parameter gradient."""
    from materialist_amd import _lib, ops

    ns = CASES[case]
    L = len(ns)
    inp = _make_inputs(case)
    d_x, x0, w_out = inp["d_x"].to(dev), inp["x0"].to(dev), inp["w_out"].to(dev)
    s = [t.to(dev) for t in inp["sines"]]
    # wt[l]: the transposed operand of the forward weight of sine layer l, [ns[l], ns[l - 1]]
    wt = [None] + [ops.mlp_split_weights(inp["weights"][l].to(dev), ns[l - 1], ns[l], transposed=True, f16=True) for l in range(1, L)]
    g = [None] + [torch.full((M, 256), 7.0, device=dev) for _ in range(1, L)]          # g[l] = dL/d pre of sine layer l
    tmax = [None] + [ops.mlp_tile_max(M, dev) for _ in range(1, L)]
    out = {"d_w_out": torch.zeros(5, 256, device=dev), "d_b_out": torch.zeros(5, device=dev), "d_w0": torch.zeros(ns[0], 16, device=dev)}
    for l in range(L):
        out[f"d_b{l}"] = torch.zeros(ns[l], device=dev)
    for l in range(1, L):
        out[f"d_w{l}"] = torch.zeros(ns[l], 256, device=dev)
    jobs, nj = (_lib.ReduceJob * 16)(), 0
    slot = lambda k: (ctypes.cast(ctypes.byref(jobs, k * ctypes.sizeof(_lib.ReduceJob)), ctypes.c_void_p), f"_plan{k}")
    ops.mlp_out_layer_bwd_tmax(d_x, s[L - 1], w_out, g[L - 1], tmax[L - 1], out["d_w_out"], out["d_b_out"], out[f"d_b{L - 1}"], 5, ns[L - 1],
                               defer=slot(nj))
    nj += 1
    for l in range(L - 1, 0, -1):
        ops.mlp_layer_bwd_weight_blk(g[l], tmax[l], s[l - 1], ns[l], 256, out=out[f"d_w{l}"], defer=slot(nj))
        nj += 1
        if l == 1:
            ops.mlp_first_layer_bwd_blk(g[l], tmax[l], wt[l], s[0], x0, out["d_w0"], 15, ns[0], ns[l], out["d_b0"], defer=slot(nj))
            nj += 2
        else:
            ops.mlp_layer_bwd_input_blk(g[l], tmax[l], wt[l], s[l - 1], g[l - 1], ns[l - 1], ns[l], out[f"d_b{l - 1}"], tmax[l - 1], defer=slot(nj))
            nj += 1
    ops.mlp_reduce_jobs(jobs, nj, d_x)
    torch.cuda.synchronize()
    for l in range(1, L):
        out[f"g{l}"] = g[l][:, :ns[l]].contiguous()          # (columns at and beyond ns[l] are scratch for every consumer)
        out[f"tmax{l}"] = tmax[l]
    return out


def _reference_run(case, dev):
    from materialist_amd import ops

    if case not in _reference:
        was = ops.mlp_set_cache_plan(0, 0)
        try:
            _reference[case] = _backward(case, dev)
        finally:
            ops.mlp_set_cache_plan(was, 0)
        assert was == 1                                        # the plan is the default
    return _reference[case]


@pytest.mark.parametrize("budget", list(BUDGETS))
@pytest.mark.parametrize("case", list(CASES))
def test_cache_plan_keeps_every_bit_of_the_backward_pass(case, budget):
    from materialist_amd import ops

    dev = _cuda()
    want = _reference_run(case, dev)
    was = ops.mlp_set_cache_plan(1, BUDGETS[budget])
    try:
        got = _backward(case, dev)
    finally:
        ops.mlp_set_cache_plan(was, 0)
    assert set(got) == set(want)
    for name in sorted(want):
        a, b = got[name], want[name]
        assert a.shape == b.shape, name
        if a.dtype == torch.float32:
            assert torch.isfinite(b).all(), name
        assert torch.equal(a, b), (name, int((a != b).sum()))
    L = len(CASES[case])
    for l in range(1, L):                                      # the pass did something: gradients and their exponents are not all zero
        assert float(want[f"g{l}"].abs().max()) > 0.0 and int(want[f"tmax{l}"].max()) > 0
        assert float(want[f"g{l}"][128 * 5:128 * 6].abs().max()) == 0.0      # the zero tile stays zero
        assert float(want[f"d_w{l}"].abs().max()) > 0.0
    assert float(want["d_w0"].abs().max()) > 0.0 and float(want["d_w_out"].abs().max()) > 0.0
