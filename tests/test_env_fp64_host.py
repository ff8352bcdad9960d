"""The fp64 helpers of tests/env_fp64.py against torch autograd on the fp64 module, without a GPU: what tests/test_gpu_env_grad.py holds
the envmap MLP's kernels to is itself pinned here."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import env_fp64  # noqa: E402


@pytest.mark.parametrize("grid,kw", [((16, 32), {}), ((30, 30), {}), ((4, 8), {}), ((8, 16), dict(hidden=(64, 128, 64), skip=(2,)))],
                         ids=["512", "900", "32", "128-narrow"])
def test_chain64_and_project_bwd64_equal_autograd_on_the_fp64_module(grid, kw):
    """module -> softplus -> SH projection -> a linear functional of the light: every parameter's gradient from `project_bwd64` + `chain64`
    equals torch autograd on the fp64 module at rtol 1e-10 (of each tensor's maximum).  Some of the output pre-activations are pushed
    beyond softplus's threshold of 20 by the last layer's bias, so the derivative's `exactly 1` branch is part of the comparison."""
    from materialist_amd import posmlp, sh

    torch.manual_seed(3)
    M = grid[0] * grid[1]
    net = posmlp.envmap_net(**kw).double()
    last = getattr(net, f"lin{net.n_layers - 1}")
    last.weight.data.normal_(0, 0.05)                         # the reference zero-initialises the last layer
    last.bias.data = torch.tensor([0.3, 21.0, -2.0], dtype=torch.float64)
    start = torch.rand(M, 3, dtype=torch.float64)
    proj = torch.from_numpy(sh.envmap_to_sh_matrix(*grid)).double()
    d_light = torch.randn(25, 3, dtype=torch.float64)

    env = net(start)
    ((proj @ env) * d_light).sum().backward()

    x0 = net._points(start)
    lins = env_fp64.layers_of(net)
    y, _, _ = env_fp64.forward64([l.weight.detach() for _, l in lins], [l.bias.detach() for _, l in lins], net.skip, x0)
    assert (y > 20).any() and (y < 20).any()
    env64, light64 = env_fp64.project64(y, proj)
    assert torch.allclose(env64, env.detach(), rtol=1e-12, atol=0) and torch.allclose(light64, proj @ env.detach(), rtol=1e-12, atol=1e-300)
    grads = env_fp64.chain64(net, x0, env_fp64.project_bwd64(y, proj, d_light))
    names = [k for k, _ in net.named_parameters()]
    assert sorted(grads) == sorted(names)
    for k, p in net.named_parameters():
        scale = p.grad.abs().max().item()
        assert scale > 0, k
        assert (grads[k] - p.grad).abs().max().item() <= 1e-10 * scale, k


def test_bwd_step64_tiles_and_shapes():
    """The per-tile column sums add up to the column sums, the last tile is ragged, and a step without a weight returns no input gradient."""
    torch.manual_seed(5)
    M, n_red, K, n_prev = 70, 5, 7, 9
    g, w = torch.randn(M, n_red, dtype=torch.float64), torch.randn(n_red, n_prev, dtype=torch.float64)
    c, x = torch.rand(M, n_prev, dtype=torch.float64) * 2 - 1, torch.randn(M, K, dtype=torch.float64)
    d_w, g_prev, colsum, d_b = env_fp64.bwd_step64(g, w, c, x)
    assert d_w.shape == (n_red, K) and g_prev.shape == (M, n_prev) and colsum.shape == (3, n_prev) and d_b.shape == (n_red,)
    assert torch.allclose(colsum.sum(0), g_prev.sum(0), rtol=1e-12) and torch.allclose(colsum[2], g_prev[64:].sum(0), rtol=1e-12)
    assert torch.allclose(d_w, torch.einsum("mn,mk->nk", g, x), rtol=1e-12) and torch.allclose(d_b, g.sum(0), rtol=1e-12)
    assert env_fp64.bwd_step64(g, None, None, x)[1:3] == (None, None)


def test_softplus_derivative_at_the_threshold():
    y = torch.tensor([-100.0, -30.0, -1e-3, 0.0, 19.999, 20.0, 20.001, 50.0], dtype=torch.float64, requires_grad=True)
    torch.nn.functional.softplus(y).sum().backward()
    d = env_fp64.softplus_grad64(y.detach())
    assert torch.allclose(d, y.grad, rtol=1e-14, atol=0)          # (autograd forms the sigmoid as z / (z + 1): the last bit may differ)
    assert d[5] < 1.0 and d[6] == 1.0 and d[7] == 1.0 and y.grad[5] < 1.0 and y.grad[6] == 1.0
