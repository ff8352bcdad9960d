"""ArmMlpPhase in the comparison configuration of `bench.py --mlp-products 0`: forward sine layers and backward products on the three bf16
pieces of `_PosMlpHipFn.PRODUCTS`, layer by layer (`FWD_PRODUCTS = 0`, `FWD_CHAIN = False`, `BWD_F16 = False`).  The other tests run the phase
with the f16 backward; this one runs `matpbr_mlp_out_layer_bwd`, `matpbr_mlp_layer_bwd_weight_bx`, `matpbr_mlp_layer_bwd_input_bx` and
`matpbr_mlp_first_layer_bwd_bx` as a phase.  96 x 96 = 9216 points: the smallest square image of whole 128-row tiles with at least MIN_ROWS rows."""
import copy
import contextlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

H = W = 96
SPP = 8


@contextlib.contextmanager
def _bf16_switches():
    from materialist_amd.armhead import ArmMlpPhase

    was = ArmMlpPhase.FWD_PRODUCTS, ArmMlpPhase.FWD_CHAIN, ArmMlpPhase.BWD_F16
    ArmMlpPhase.FWD_PRODUCTS, ArmMlpPhase.FWD_CHAIN, ArmMlpPhase.BWD_F16 = 0, False, False
    try:
        yield ArmMlpPhase
    finally:
        ArmMlpPhase.FWD_PRODUCTS, ArmMlpPhase.FWD_CHAIN, ArmMlpPhase.BWD_F16 = was


def _setup():
    from materialist_amd import posmlp, render, synthetic

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.manual_seed(20250629)
    dev = torch.device("cuda:0")
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    sc = synthetic.make_scene(5, H, W)
    scene = render.load_estimated_mesh(t(sc.depth), use_mesh_normal=True)
    scene._set("emitter.data", t(sc.light))
    gt = torch.rand(H, W, 3, device=dev)
    a0, r0, m0 = t(sc.init_albedo), t(sc.init_roughness), t(sc.init_metallic)
    start_arm = torch.cat([a0.reshape(-1, 3), r0.reshape(-1, 1), m0.reshape(-1, 1)], -1).clamp(0, 1)
    torch.manual_seed(4)
    net = posmlp.brdf_net("arm").to(dev)
    net.lin4.weight.data.normal_(0, 0.05)                  # a non-zero output layer: every layer below it receives a gradient
    net.lin4.bias.data.normal_(0, 0.05)
    return scene, gt, net, start_arm, {"albedo": a0, "roughness": r0, "metallic": m0}


def test_arm_mlp_phase_bf16_network_gradients_match_autograd():
    """`test_arm_mlp_phase_network_gradients_match_autograd` (tests/test_gpu_parity.py) at the bf16 configuration, with its bounds: forward()
    against the reference module's maps, backward() fed with given map gradients against torch autograd through the reference network."""
    from materialist_amd import posmlp

    scene, gt, net_a, start_arm, fixed = _setup()
    net_b = copy.deepcopy(net_a)
    with _bf16_switches() as ArmMlpPhase:
        ph = ArmMlpPhase(scene, gt, net_b, start_arm, fixed, optimize_part="arm", spp=SPP)
    assert ph.chain is False and ph.bwd_f16 is False
    maps = ph.forward()
    posmlp._PosMlpHipFn.MIN_ROWS = 1 << 30             # the reference side on the torch/BLAS composition of the network
    try:
        arm = net_a(start_arm)
        ref = {"albedo": arm[:, 0:3].reshape(H, W, 3), "roughness": (arm[:, 3:4] * 0.93 + 0.07).reshape(H, W, 1), "metallic": arm[:, 4:5].reshape(H, W, 1)}
        for k in ref:                                      # one ulp of the straight-through clamp's (c + x) - x on top of the network's rounding
            err = (maps[k] - ref[k].detach()).abs().max().item()
            print(f"map {k}: max abs err {err:.3e} (bound 3e-6)")
            assert err <= 3e-6, k
        g = {k: torch.randn_like(v) for k, v in ref.items()}
        torch.autograd.backward([ref[k] for k in ref], [g[k] for k in ref])
    finally:
        posmlp._PosMlpHipFn.MIN_ROWS = 8192
    for k in g:
        ph.g[k].copy_(g[k])
    ph.backward()
    g_ref = [p.grad for p in net_a.parameters()]
    for l, (gw, gb) in enumerate(ph.gviews):
        rw, rb = g_ref[2 * l], g_ref[2 * l + 1]
        e_max = (gw[:, :rw.shape[1]] - rw).abs().max().item() / rw.abs().max().item()
        e_w = (gw[:, :rw.shape[1]] - rw).norm().item() / rw.norm().item()
        e_b = (gb[:rb.shape[0]] - rb).norm().item() / rb.norm().item()
        print(f"layer {l}: weight max {e_max:.3e} (bound 3e-4), weight norm {e_w:.3e} (2e-5), bias norm {e_b:.3e} (2e-5)")
        assert e_max <= 3e-4, l
        assert e_w <= 2e-5, l
        assert (gw.shape[1] > rw.shape[1]) == (l == 0)      # 15 inputs in rows of 16 floats: only the first layer has a padding column
        assert (gw[:, rw.shape[1]:] == 0).all()            # the padding column of the first layer never receives a gradient
        assert e_b <= 2e-5, l


def test_arm_mlp_phase_bf16_steps_are_bit_reproducible():
    """Three whole iterations at the bf16 configuration, twice from the same network: the same bits in the parameters, the gradients and the
    statistics row (no atomics and no launch-order dependence anywhere on this path)."""
    scene, gt, net, start_arm, fixed = _setup()
    runs = []
    for _ in range(2):
        with _bf16_switches() as ArmMlpPhase:
            ph = ArmMlpPhase(scene, gt, copy.deepcopy(net), start_arm, fixed, optimize_part="arm", spp=SPP)
        assert ph.chain is False and ph.bwd_f16 is False
        for _ in range(3):
            ph.step()
        torch.cuda.synchronize()
        runs.append((ph.flat.clone(), ph.gflat.clone(), ph.stats.clone()))
    for a, b, what in zip(runs[0], runs[1], ("flat", "gflat", "stats")):
        assert torch.equal(a, b), what
    assert torch.isfinite(runs[0][0]).all() and float(runs[0][1].abs().max()) > 0.0
