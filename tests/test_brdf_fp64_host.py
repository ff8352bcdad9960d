"""The fp64 helpers of tests/brdf_fp64.py against torch autograd on `loss.brdf_loss` (the torch composition, `FUSED = False`) in double,
without a GPU, on the inputs tests/test_gpu_brdf_grad.py feeds the kernels; the conditions those inputs are meant to meet (DESIGN.md
section 5.2); and the error of the fp32 composition on a CPU, from which that section's floor is taken."""
import os
import sys

import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import brdf_fp64 as bf  # noqa: E402

F64 = torch.float64
SD = 0.1
_IDS = ["x".join(map(str, s)) for s in bf.SHAPES]
_KEY = {"a": "albedo", "r": "roughness", "m": "metallic"}


@pytest.fixture(scope="module")
def inputs():
    return {s: bf.make_inputs(*s) for s in bf.SHAPES}


@pytest.fixture()
def torch_loss():
    from materialist_amd import loss

    keep, loss.FUSED = loss.FUSED, False
    yield loss
    loss.FUSED = keep


def _surrogate(c, jac, pred, dtype):
    """A render whose value is `pred` and whose derivatives in the clamped maps are the jac planes' closed forms."""
    P, S, JR = bf.planes(jac, dtype)
    out = c["a"] * (1.0 - c["m"]) * P + (c["m"] * c["a"] + 0.04 * (1.0 - c["m"])) * S + JR * c["r"]
    return out + (pred.to(dtype) - out.detach())


def _autograd(loss, inp, part, pred, dtype=F64):
    raw = {k: inp["maps"][k].to(dtype).requires_grad_() for k in bf.KEYS}
    c = {k: raw[k].clamp(*bf.LIMS[k]) for k in bf.KEYS}
    out = _surrogate(c, inp["jac"], pred, dtype)
    out.retain_grad()
    live = bf.maps_in(part)
    total, mse, _, ratio = loss.brdf_loss(out, inp["gt"].to(dtype), {_KEY[k]: c[k] for k in live}, {_KEY[k]: inp["anchors"][k].to(dtype) for k in live},
                                          float(torch.tensor(SD, dtype=torch.float32)), gt_srgb=inp["gt_srgb"].to(dtype))
    total.backward()
    return {k: raw[k].grad for k in bf.KEYS}, out.grad, mse.detach().reshape(-1), ratio.detach().reshape(-1), total.detach()


@pytest.mark.parametrize("shape", bf.SHAPES, ids=_IDS)
def test_stats_dpred_and_fused_grads_equal_autograd_on_the_torch_composition(shape, inputs, torch_loss):
    inp = inputs[shape]
    for pred in (inp["pred"], inp["pred_z"]):
        for part in bf.PARTS:
            grads, d_pred, mse, ratio, total = _autograd(torch_loss, inp, part, pred)
            s = bf.stats64(pred, inp["gt"], inp["maps"], inp["anchors"], part, SD, inp["gt_srgb"])
            assert torch.allclose(s["mse"], mse, rtol=1e-12, atol=0) and torch.allclose(s["ratio"], ratio, rtol=1e-12, atol=0)
            assert abs(float(s["loss"].sum()) - float(total)) <= 1e-12 * abs(float(total))
            dp = bf.dpred64(pred, inp["gt_srgb"], s["ratio"], s["sr"])
            assert (dp - d_pred).abs().max().item() <= 1e-10 * d_pred.abs().max().item()
            assert bool((dp[inp["zeros"]] == 0).all()) or pred is inp["pred"]
            got = bf.fused_grads64(inp["maps"], inp["anchors"], pred, inp["gt_srgb"], s["ratio"], s["sr"], inp["jac"], part, SD)
            for k in bf.KEYS:
                assert (got[k] - grads[k]).abs().max().item() <= 1e-10 * grads[k].abs().max().item(), (part, k)
    # the regulariser's share is there: a part changes the gradient of its own maps only
    s = bf.stats64(inp["pred"], inp["gt"], inp["maps"], inp["anchors"], "arm", SD, inp["gt_srgb"])
    g_arm = bf.fused_grads64(inp["maps"], inp["anchors"], inp["pred"], inp["gt_srgb"], s["ratio"], s["sr"], inp["jac"], "arm", SD)
    g_a = bf.fused_grads64(inp["maps"], inp["anchors"], inp["pred"], inp["gt_srgb"], s["ratio"], s["sr"], inp["jac"], "a", SD)
    assert torch.equal(g_arm["a"], g_a["a"])
    if shape != (1, 1, 1):
        assert not torch.equal(g_arm["r"], g_a["r"]) and not torch.equal(g_arm["m"], g_a["m"])


def test_part_semantics_of_the_statistics():
    assert bf.maps_in("") == ["a", "r", "m"] and bf.maps_in("arm") == ["a", "r", "m"] and bf.maps_in("rm") == ["r", "m"]
    assert bf.maps_in("n") == [] and bf.maps_in("rn") == ["r"] and bf.maps_in("armn") == ["a", "r", "m"]
    inp = bf.make_inputs(1, 5, 7)
    s = bf.stats64(inp["pred"], inp["gt"], inp["maps"], inp["anchors"], "rn", SD, inp["gt_srgb"])
    assert float(s["la"]) == 0.0 and float(s["lm"]) == 0.0 and float(s["lr"]) > 0.0
    assert float(s["loss"]) == pytest.approx(float(3 * s["sr"] * s["mse"] + s["l1"] + float(torch.tensor(SD, dtype=torch.float32)) * s["lr"]), rel=1e-14)


@pytest.mark.parametrize("shape", [(1, 5, 7), (1, 1, 257), (3, 33, 37)], ids=["1x5x7", "1x1x257", "3x33x37"])
@pytest.mark.parametrize("part", ["n", "rn", "armn"])
def test_normal_step_grads_equal_autograd_through_clamp_and_normalize(shape, part, inputs):
    inp = inputs[shape]
    sd = float(torch.tensor(SD, dtype=torch.float32))
    raw = {k: inp["maps"][k].double().requires_grad_() for k in bf.KEYS}
    pn = inp["pn"].double().requires_grad_()
    c = {k: raw[k].clamp(*bf.LIMS[k]) for k in bf.KEYS}
    nh = torch.nn.functional.normalize(pn, p=2, dim=-1)
    mean = lambda x: x.reshape(x.shape[0], -1).mean(dim=1).sum()
    total = (inp["d"]["n"].double() * nh).sum() + sd * mean((nh - inp["n0"].double()).abs())
    for k in bf.KEYS:
        total = total + (inp["d"][k].double() * c[k]).sum()
        if k in part:
            total = total + sd * mean((c[k] - inp["anchors"][k].double()).abs())
    total.backward()
    got = bf.normal_step_grads64(inp["maps"], inp["anchors"], inp["d"], inp["pn"], inp["n0"], part, SD)
    assert sorted(got) == sorted(part)
    P = shape[1] * shape[2]
    zero = torch.zeros(shape[0], P, dtype=torch.bool)
    for b, z in enumerate(inp["zero_pix"]):
        zero[b, z] = True
    zero = zero.reshape(shape[0], shape[1], shape[2], 1).expand_as(pn)
    assert int(zero.sum()) == 3 * shape[0]
    for sel in (zero, ~zero):           # the all-zero vectors' gradients are g / 1e-12: compared on their own scale
        a, b = got["n"][sel], pn.grad[sel]
        assert bool(torch.isfinite(a).all()) and (a - b).abs().max().item() <= 1e-10 * b.abs().max().item()
    assert got["n"][zero].abs().min().item() > 1e3
    for k in bf.KEYS:
        if k in part:
            assert (got[k] - raw[k].grad).abs().max().item() <= 1e-10 * raw[k].grad.abs().max().item(), k


def test_adam64_is_torch_adam_over_two_steps():
    gen = torch.Generator().manual_seed(7)
    p0 = torch.rand(50, generator=gen, dtype=F64)
    gs = [torch.randn(50, generator=gen, dtype=F64) * 1e-4, torch.randn(50, generator=gen, dtype=F64) * 3e-4]
    gs[0][:3] = 0.0
    p = p0.clone().requires_grad_()
    opt = torch.optim.Adam([p], lr=3e-4)
    q, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for t, g in enumerate(gs, 1):
        p.grad = g.clone()
        opt.step()
        q, m, v = bf.adam64(q, g, m, v, 3e-4, t)
        assert (q - p.detach()).abs().max().item() <= 1e-12 * 3e-4, t
        assert torch.allclose(m, opt.state[p]["exp_avg"], rtol=1e-14, atol=0) and torch.allclose(v, opt.state[p]["exp_avg_sq"], rtol=1e-14, atol=0)
    assert torch.equal(bf.adam64(p0, gs[0], m * 0, v * 0, 3e-4, 1)[0][:3], p0[:3])          # zero gradient, zero moments: the parameter rests
    assert bool((q[:3] != p0[:3]).all())                                                     # ... and moves with the second step's gradient


@pytest.mark.parametrize("shape", bf.SHAPES, ids=_IDS)
def test_input_conditions(shape, inputs):
    """What section 5.2 promises of the inputs: no element is left out of a gradient comparison (no |d| below 1e-5, no fp32 / fp64 sign
    disagreement), every class of raw value occurs, regulariser signs are decided by fp32 inputs alone, the planes span 1e-3 ... 10."""
    inp = inputs[shape]
    B, H, W = shape
    for pred in (inp["pred"], inp["pred_z"]):
        mask, dmin, flips = bf.sign_exclusions(pred, inp["gt"], inp["gt_srgb"], inp["maps"], inp["anchors"])
        assert int(mask.sum()) == 0 and flips == 0 and dmin > 1e-2, (dmin, flips)
    assert float(inp["gt"].min()) >= 0.05 and float(inp["gt"].max()) <= 0.85
    f = inp["pred"] / inp["gt"]
    assert bool((((f > 0.549) & (f < 0.851)) | ((f > 1.149) & (f < 1.451))).all())
    assert int(inp["zeros"].sum()) == B * min(5, H * W * 3 // 24) and bool((inp["pred_z"][inp["zeros"]] == 0).all())
    a = inp["jac"].abs()
    assert float(a.min()) >= 1e-3 * 0.999 and float(a.max()) <= 10.001
    for k in bf.KEYS:
        raw, p0, (lo, hi) = inp["maps"][k].double(), inp["anchors"][k].double(), bf.LIMS[k]
        diff = raw.clamp(lo, hi) - p0
        assert bool(((diff == 0) | (diff.abs() >= 1e-3)).all()), k
        if raw.numel() >= 40:
            assert bool((raw < lo).any()) and bool((raw > hi).any()) and bool((diff == 0).any()), k
            for val in (0.0, 1.0, float(torch.tensor(0.07, dtype=torch.float32))):
                assert bool((raw == val).any()), (k, val)
            assert bool(((diff == 0) & (raw < lo)).any()) and bool(((diff == 0) & (raw > hi)).any()) and bool(((diff == 0) & (raw > lo) & (raw < hi)).any()), k
    nh, ln = bf.normalize64(inp["pn"])
    dn = nh - inp["n0"].double()
    assert bool(((dn == 0) | (dn.abs() >= 1e-3)).all())
    if H * W >= 3:
        assert int((dn == 0).sum()) >= 2 * B and int((ln == 0).sum()) == B
        assert float(ln[ln > 0].min()) >= 0.29 and float(ln.max()) <= 3.01


def _rel(x, ref):
    return (x.double() - ref).abs().max().item() / (ref.abs().max().item() + 1e-300)


def test_fp32_composition_on_the_cpu_sets_the_floor(inputs, torch_loss, capsys):
    """The worst error of the fp32 torch composition (loss.brdf_loss + autograd; the closed forms of the streaming backward and the normal
    step in fp32) against the fp64 helpers over the GPU file's inputs, of each tensor's maximum.  DESIGN.md section 5.2's floor is four
    times this figure (6.4e-7, the fused d_r; section 5.2 lists every family); a CPU with another vector width sums in another order, hence the
    margin of the assertion."""
    worst = {}

    def note(fam, e):
        worst[fam] = max(worst.get(fam, 0.0), e)

    for shape in bf.SHAPES:
        inp = inputs[shape]
        for pred in (inp["pred"], inp["pred_z"]):
            s = bf.stats64(pred, inp["gt"], inp["maps"], inp["anchors"], "arm", SD, inp["gt_srgb"])
            s32 = bf.stats64(pred, inp["gt"], inp["maps"], inp["anchors"], "arm", SD, inp["gt_srgb"], dtype=torch.float32)
            for k in bf.SLOTS:
                note("stats", _rel(s32[k], s[k]))
            grads, d_pred, mse, ratio, _, _ = bf.torch_composition(torch_loss, inp["maps"], inp["anchors"], pred, inp["gt"], inp["gt_srgb"], inp["jac"], "arm", SD,
                                                                   torch.float32)
            note("stats", _rel(mse, s["mse"]))
            note("d_pred", _rel(d_pred, bf.dpred64(pred, inp["gt_srgb"], s["ratio"], s["sr"])))
            ref = bf.fused_grads64(inp["maps"], inp["anchors"], pred, inp["gt_srgb"], s["ratio"], s["sr"], inp["jac"], "arm", SD)
            for k in bf.KEYS:
                note("fused d_" + k, _rel(grads[k], ref[k]))
        c = bf.clamped(inp["maps"])
        ref = bf.jac_grads64(c["a"], c["r"], c["m"], *bf.planes(inp["jac"]), inp["go"])
        c32 = bf.clamped(inp["maps"], torch.float32)
        got = bf.jac_grads64(c32["a"], c32["r"], c32["m"], *bf.planes(inp["jac"], torch.float32), inp["go"], dtype=torch.float32)
        for k in bf.KEYS:
            note("jac d_" + k, _rel(got[k], ref[k]))
        ref = bf.normal_step_grads64(inp["maps"], inp["anchors"], inp["d"], inp["pn"], inp["n0"], "armn", SD)
        got = bf.normal_step_grads64(inp["maps"], inp["anchors"], inp["d"], inp["pn"], inp["n0"], "armn", SD, dtype=torch.float32)
        live = (bf.normalize64(inp["pn"])[1] > 0).expand_as(ref["n"])
        note("normal step d_n", _rel(got["n"][live], ref["n"][live]))
        for k in bf.KEYS:
            note("normal step d_" + k, _rel(got[k], ref[k]))
    with capsys.disabled():
        for fam, e in worst.items():
            print(f"\n  fp32 composition on the CPU, {fam}: {e:.2e}", end="")
        print()
    assert max(worst.values()) <= 1.5 * FLOOR / 4.0, worst


FLOOR = 2.6e-6      # tests/test_gpu_brdf_grad.py FLOOR
