"""The pos_mlp backward kernels whose instruction schedule changed keep their bits:

* `mlp_wgrad_hx` (rows by LDS-DMA, the two waves of a SIMD half a step apart) against the register-staged `mlp_wgrad_bx<3>` behind the same
  entry point (`ops.mlp_set_wgrad_kernel`): the folded `dW` and the raw workspace of partial sums, `torch.equal`;
* the first-layer form `mlp_nt_gx<mul cos, 3, W0>` against digests recorded from the library BEFORE its registers were re-arranged
  (tests/golden/posmlp_w0_bits.json: digests and shapes only).  `python tests/test_gpu_wgrad_stagger.py` prints that file's contents for the
  library `MATPBR_LIB` names; the test never regenerates it.
"""
import hashlib
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "posmlp_w0_bits.json")
ROWS = [128, 128 * 5, 8192, 128 * 520]            # one tile (8 steps) · workgroups of 2 / 2 / 1 tiles · 32 x 2 tiles · 245 workgroups of 3 or 2 tiles
W0_ROWS = [8192, 128 * 520]
_inputs = {}


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _make_inputs(M):
    """The inputs of test_block_scaled_f16_backward_products, made on the CPU from a fixed numpy seed: gradients of 1e-6 with tile magnitudes spread
    over 1e4, one all-zero tile, every seventh column 1e-3 below its tile; x sign-carrying sines (the last mantissa bit is the cosine's sign)
    with one coordinate column of hundreds.  Made once per row count and left unchanged."""
    if M not in _inputs:
        rng = np.random.default_rng(1000 + M)
        T = M // 128
        mag = np.clip(np.exp(rng.standard_normal(T) * 2.0), 1e-2, 1e2).astype(np.float32)
        g = rng.standard_normal((M, 256), dtype=np.float32) * np.float32(1e-6) * np.repeat(mag, 128)[:, None]
        g[:, ::7] *= np.float32(1e-3)
        if T > 1:                                          # (a single tile stays as it is: all zeros would test nothing)
            zt = min(5, T - 1)
            g[128 * zt:128 * (zt + 1)] = 0.0
        pre = rng.standard_normal((M, 256)) * 3.0
        x = np.sin(pre).astype(np.float32)
        bits = x.view(np.uint32)
        bits &= np.uint32(0xFFFFFFFE)
        bits |= (np.cos(pre) < 0).astype(np.uint32)
        x[:, 255] = rng.integers(0, 512, M).astype(np.float32)
        x0 = np.zeros((M, 16), dtype=np.float32)
        x0[:, :15] = rng.standard_normal((M, 15), dtype=np.float32)
        x0[:, 0] = rng.integers(0, 512, M).astype(np.float32)
        w = ((rng.random((256, 256), dtype=np.float32) * 2 - 1) / 16).astype(np.float32)
        _inputs[M] = tuple(torch.from_numpy(a) for a in (g, x, x0, w))
    return _inputs[M]


def _grads(M, n_red, dev, scratch):
    g, x, x0, w = (t.to(dev) for t in _make_inputs(M))
    T = M // 128
    tmax = g[:, :n_red].abs().view(T, 128, n_red).amax((1, 2)).contiguous().view(torch.int32)
    g = g.clone()
    g[:, n_red:] = scratch
    return g, tmax, x, x0, w


@pytest.mark.parametrize("n_red", [256, 241])
@pytest.mark.parametrize("M", ROWS)
def test_staggered_weight_gradient_is_the_register_staged_one_bit_for_bit(M, n_red):
    """`ops.mlp_layer_bwd_weight_blk` on `mlp_wgrad_hx` against the same call on `mlp_wgrad_bx<3>`: the folded dW AND every slab of partial sums
    are the same bits.  M = 128: the stagger's prologue and epilogue are the whole run; 128 x 5: fewer steps than the rings are deep plus one in
    the last workgroup; 128 x 520: more tiles than workgroups.  The scratch columns at and beyond n_red hold inf."""
    from materialist_amd import _lib, ops

    dev = _cuda()
    lib = _lib.load()
    g, tmax, x, _, _ = _grads(M, n_red, dev, float("inf"))
    ws = ops._mlp_workspace("bwd_weight", M, dev, lib.matpbr_mlp_bwd_weight_workspace_bytes(M))
    got = {}
    was = ops.mlp_set_wgrad_kernel(1)
    try:
        for kernel in (1, 0):
            assert ops.mlp_set_wgrad_kernel(kernel) in (0, 1)
            ws.fill_(float("nan"))
            dw = ops.mlp_layer_bwd_weight_blk(g, tmax, x, n_red, 256)
            torch.cuda.synchronize()
            got[kernel] = (dw.clone(), ws.clone())
    finally:
        ops.mlp_set_wgrad_kernel(was)
    assert was == 1                                            # the default is the new kernel
    assert torch.isfinite(got[1][0]).all() and float(got[1][0].abs().max()) > 0.0
    assert torch.equal(got[1][0], got[0][0])
    assert torch.equal(got[1][1].view(torch.int32), got[0][1].view(torch.int32))     # (as integers: untouched slabs stay NaN in both)


def w0_bits(M, dev):
    """SHA-256 of d_w0 and d_bias of `ops.mlp_first_layer_bwd_blk` (n_prev = 241, d0 = 15) on the inputs above."""
    from materialist_amd import ops

    n_prev, n_red, d0 = 241, 256, 15
    g, tmax, s_prev, x0, w = _grads(M, n_red, dev, 0.0)
    wt = ops.mlp_split_weights(w, n_prev, n_red, transposed=True, f16=True)
    d_w0 = torch.zeros(n_prev, 16, device=dev)
    d_b = torch.zeros(n_prev, device=dev)
    ops.mlp_first_layer_bwd_blk(g, tmax, wt, s_prev, x0, d_w0, d0, n_prev, n_red, d_b)
    torch.cuda.synchronize()
    assert torch.isfinite(d_w0).all() and torch.isfinite(d_b).all() and float(d_w0.abs().max()) > 0.0
    return {"d_w0": hashlib.sha256(d_w0.cpu().numpy().tobytes()).hexdigest(), "d_w0_shape": list(d_w0.shape),
            "d_bias": hashlib.sha256(d_b.cpu().numpy().tobytes()).hexdigest(), "d_bias_shape": list(d_b.shape)}


@pytest.mark.parametrize("M", W0_ROWS)
def test_first_layer_form_keeps_its_bits(M):
    """The W0 form of the input gradient (dW0 chains in registers across a workgroup's tiles, csum4 column sums) against the digests recorded
    from the library before its epilogue was brought under 256 registers without scratch."""
    dev = _cuda()
    if not os.path.exists(GOLDEN):
        pytest.skip("tests/golden/posmlp_w0_bits.json is missing: record it with the PREVIOUS library (python tests/test_gpu_wgrad_stagger.py)")
    want = json.load(open(GOLDEN))[str(M)]
    assert w0_bits(M, dev) == want


if __name__ == "__main__":
    print(json.dumps({str(M): w0_bits(M, torch.device("cuda:0")) for M in W0_ROWS}, indent=1, sort_keys=True))
