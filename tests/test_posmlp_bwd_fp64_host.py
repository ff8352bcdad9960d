"""The fp64 restatements of the pos_mlp f16 backward pass and their error model (tests/posmlp_bwd_fp64.py), proved on the CPU:
the restatements chained reproduce torch autograd of the 'arm' network in fp64; the emulation of the documented arithmetic stays within the derived
bound for every recipe and shape that tests/test_gpu_posmlp_bwd_fp64.py uses; every deliberate mutation of that arithmetic breaks the bound by a
factor of four or more on some output -- so the GPU file would notice a kernel that made the same mistake."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import posmlp_bwd_fp64 as R    # noqa: E402  (tests/ is on the path: the helper is a sibling module)

# reduction depths at which a dropped cross product (2^-12 of the sum on `coherent`) stands four times above the worst-case bound, whose
# accumulation term is 3 K 2^-23: K = 64 columns for the input gradient and the first layer, 128 rows for the weight gradient, 256 rows (two
# tiles, so that there is a neighbouring exponent) for the first layer's sums over rows (the GPU file's piece probe runs the same depths beside the full ones)
PROBE_N_RED, PROBE_M, PROBE_M_FIRST = 64, 128, 256


def test_restatements_reproduce_autograd_of_the_arm_network():
    """Proves the reference, not a kernel: out_layer -> weight_grad / input_grad -> first_layer, fed with fp64 sines that carry the sign of their
    cosine in their last mantissa bit, against autograd through plain torch operations on the parameters of posmlp.PosMLP('arm').double()
    (whose own forward is checked to be the same function) at 512 points -- the network takes h x 2h grids, so 16 x 32 is its smallest point set
    of whole 128-row tiles beyond one; 256 points are not a grid it accepts: every parameter gradient to 1e-12 of its largest."""
    from materialist_amd import posmlp

    torch.manual_seed(5)
    net = posmlp.brdf_net("arm").double()
    with torch.no_grad():
        net.lin4.weight.copy_(torch.randn(5, 256, dtype=torch.float64) / 16)
        net.lin4.bias.copy_(torch.randn(5, dtype=torch.float64) / 16)
    P = 512
    img = torch.rand(P, 5, dtype=torch.float64)
    x0 = net._points(img)
    assert x0.shape == (P, 15)
    lins = [net.lin0.linear, net.lin1.linear, net.lin2.linear, net.lin3.linear, net.lin4]
    ns = [lin.weight.shape[0] for lin in lins[:4]]
    assert ns == R.SHAPES["ragged"]
    pres, bufs, inp = [], [], x0
    for l in range(4):
        pre = inp @ lins[l].weight.t() + lins[l].bias
        pres.append(pre)
        inp = torch.cat([torch.sin(pre), x0], 1) if ns[l] < 256 else torch.sin(pre)
        bufs.append(inp)
    x = inp @ lins[4].weight.t() + lins[4].bias
    x.retain_grad()
    y = 1.3 * torch.tanh(x) + img
    out = y.clamp(0, 1).detach() + y - y.detach()
    assert torch.allclose(out, net(img), rtol=0, atol=1e-13)
    (out * torch.randn(P, 5, dtype=torch.float64)).sum().backward()

    d_x = torch.zeros(P, 8, dtype=torch.float64)
    d_x[:, :5] = x.grad
    x0p = torch.zeros(P, 16, dtype=torch.float64)
    x0p[:, :15] = x0
    s = []
    for l in range(4):
        b = bufs[l].detach().clone()
        b[:, :ns[l]] = torch.from_numpy(R.pack_sines(pres[l].detach().numpy(), np.float64))
        s.append(b)
    W = [lin.weight.detach() for lin in lins]
    got = {}
    r, _ = R.out_layer(d_x, s[3], W[4], 5, ns[3])
    got["lin4.weight"], got["lin4.bias"], got["lin3.linear.bias"] = r["d_w"], r["d_b"], r["d_b_prev"]
    assert torch.equal(r["tmax"], R.tile_max_bits(r["g"].float(), ns[3]))
    g = r["g"]
    for l in (3, 2, 1):
        tm = R.tile_max_bits(g.float(), ns[l])
        got[f"lin{l}.linear.weight"] = R.weight_grad(g, s[l - 1], ns[l])
        if l > 1:
            r, _ = R.input_grad(g, tm, W[l], s[l - 1], ns[l - 1], ns[l])
            g, got[f"lin{l - 1}.linear.bias"] = r["g"], r["d_b"]
        else:
            r, _ = R.first_layer(g, tm, W[1], s[0], x0p, 15, ns[0], ns[1])
            got["lin0.linear.weight"], got["lin0.linear.bias"] = r["d_w0"][:, :15], r["d_b0"]
    names = dict(net.named_parameters())
    assert set(got) == set(names)
    for name, p in names.items():
        err = float((got[name] - p.grad).abs().max() / p.grad.abs().max())
        assert err <= 1e-12, (name, err)


@pytest.mark.parametrize("M", [128, 2048])
def test_tile_maxima_of_the_restatement_are_the_brute_force_maxima(M):
    inp = R.to_torch(R.make_inputs("random", "ragged", M))
    ref, _ = R.out_layer(inp["d_x"], inp["sines"][3], inp["w_out"], 5, 256)
    g32 = ref["g"].float().numpy()
    want = np.array([np.abs(g32[t * 128:(t + 1) * 128]).max() for t in range(M // 128)], dtype=np.float32)
    assert np.array_equal(ref["tmax"].numpy().view(np.float32), want)
    r2, _ = R.input_grad(ref["g"].float(), ref["tmax"], inp["weights"][3], inp["sines"][2], 241, 256)
    g32 = r2["g"].float().numpy()
    want = np.array([np.abs(g32[t * 128:(t + 1) * 128, :241]).max() for t in range(M // 128)], dtype=np.float32)
    assert np.array_equal(r2["tmax"].numpy().view(np.float32), want)
    if M > 128:
        assert want[5] == 0.0


# (the GPU file's fourth row count, 128 x 520, is about workgroups that walk several tiles: the emulation has no workgroups, and its fp64 bound
# takes 13 s on a CPU -- the sequence is the same code at 9216 rows)
SEQUENCES = [(c, M) for c in R.SHAPES for M in (128, 2048, 9216)]


@pytest.mark.parametrize("case,M", SEQUENCES)
def test_emulated_sequence_stays_within_the_bound(case, M):
    zt = 5
    inp = R.make_inputs("random", case, M, zero_tile=zt)
    res, _ = R.check_sequence(R.to_torch(inp), R.emulate_sequence(inp, case), case, zt)
    print(f"emulation {case} M={M}: " + " ".join(f"{k}={v:.3f}" for k, v in res.items()))
    assert all(v <= 1.0 for v in res.values()), res


def _single(kernel, p, n_prev, n_red, mutation=None):
    """One kernel's emulation against its restatement: {output: max err / bound}."""
    t = R.to_torch(p)
    if kernel == "dgrad":
        g, db, tm = R.emulate_input_grad(p["g"], p["tmax"], p["w"], p["s_prev"], n_prev, n_red, mutation)
        ref, bnd = R.input_grad(t["g"], t["tmax"], t["w"], t["s_prev"], n_prev, n_red)
        return {"g": R.ratio(torch.from_numpy(g), ref["g"], bnd["g"]), "d_b": R.ratio(torch.from_numpy(db), ref["d_b"], bnd["d_b"]),
                "tmax": R.tmax_ratio(torch.from_numpy(tm), ref["g"], bnd["g"], n_prev)}
    if kernel == "first":
        dw, db = R.emulate_first_layer(p["g"], p["tmax"], p["w"], p["s_prev"], p["x0"], 15, n_prev, n_red, mutation)
        ref, bnd = R.first_layer(t["g"], t["tmax"], t["w"], t["s_prev"], t["x0"], 15, n_prev, n_red)
        return {"d_w0": R.ratio(torch.from_numpy(dw), ref["d_w0"], bnd["d_w0"]), "d_b0": R.ratio(torch.from_numpy(db), ref["d_b0"], bnd["d_b0"])}
    assert kernel == "wgrad"
    dw = R.emulate_weight_grad(p["g"], p["tmax"], p["s_prev"], n_red, mutation)
    return {"d_w": R.ratio(torch.from_numpy(dw), R.weight_grad(t["g"], t["s_prev"], n_red), R.weight_grad_bound(t["g"], t["tmax"], t["s_prev"], n_red))}


# kernel, recipe, M, n_prev, n_red: the single-kernel runs of the GPU file (piece probe, magnitude edges)
SINGLES = [("dgrad", "coherent", 2048, 256, 256), ("dgrad", "coherent", 2048, 241, PROBE_N_RED), ("first", "coherent", 2048, 241, 256),
           ("first", "coherent", PROBE_M_FIRST, 241, PROBE_N_RED), ("wgrad", "coherent", 256, 256, 256), ("wgrad", "coherent", PROBE_M, 256, 241),
           ("dgrad", "range", 2048, 241, 256), ("dgrad", "range", 2048, 256, 241), ("first", "range", 2048, 241, 256), ("wgrad", "range", 256, 256, 241)]


@pytest.mark.parametrize("kernel,recipe,M,n_prev,n_red", SINGLES)
def test_emulated_kernel_stays_within_the_bound(kernel, recipe, M, n_prev, n_red):
    zt = 5 if M > 640 else 99
    res = _single(kernel, R.make_single(recipe, M, n_prev, n_red, zero_tile=zt), n_prev, n_red)
    print(f"emulation {kernel} {recipe} M={M} n_prev={n_prev} n_red={n_red}: " + " ".join(f"{k}={v:.3f}" for k, v in res.items()))
    assert all(v <= 1.0 for v in res.values()), res


def _out_layer(recipe, M, mutation=None):
    inp = R.make_inputs(recipe, "wide", M)
    t = R.to_torch(inp)
    g, tm = R.emulate_out_layer(inp["d_x"], inp["sines"][3], inp["w_out"], 5, 256, mutation)
    ref, bnd = R.out_layer(t["d_x"], t["sines"][3], t["w_out"], 5, 256)
    return {"g": R.ratio(torch.from_numpy(g), ref["g"], bnd["g"]), "tmax": R.tmax_ratio(torch.from_numpy(tm), ref["g"], bnd["g"], 256)}


# what each kernel's arithmetic can get wrong: the output layer forms no f16 pieces, the weight gradient decodes no cosine and has one exponent
APPLICABLE = {"dgrad": R.MUTATIONS, "first": R.MUTATIONS, "wgrad": ("drop_p1q2", "drop_p2q1"), "out": ("neighbour_row_cos", "skip_sign")}
PROBES = {"dgrad": (2048, 241, PROBE_N_RED), "first": (PROBE_M_FIRST, 241, PROBE_N_RED), "wgrad": (PROBE_M, 256, 256)}


@pytest.mark.parametrize("kernel,mutation", [(k, m) for k, ms in APPLICABLE.items() for m in ms])
def test_mutation_breaks_the_bound_on_coherent(kernel, mutation):
    """`coherent`: every second piece is as large as it can be and positive, so a lost cross product is a bias of 2^-12 of the sum -- at the probe
    depths that is more than four times the bound (at K = 256 the worst-case accumulation term alone, 768 x 2^-23, is 0.4 of it).  The neighbouring
    tile's exponent overflows f16 where that tile is 2^8 times smaller; every cosine is negative, so the sign is missed everywhere."""
    if kernel == "out":
        clean, res = _out_layer("coherent", 2048), _out_layer("coherent", 2048, mutation)
    else:
        M, n_prev, n_red = PROBES[kernel]
        p = R.make_single("coherent", M, n_prev, n_red, zero_tile=5 if M > 640 else 99)
        clean, res = _single(kernel, p, n_prev, n_red), _single(kernel, p, n_prev, n_red, mutation)
    print(f"mutation {kernel} coherent {mutation}: factor {max(res.values()):.1f} (unmutated {max(clean.values()):.3f})")
    assert max(clean.values()) <= 1.0 and max(res.values()) >= 4.0, (clean, res)


@pytest.mark.parametrize("kernel,mutation", [(k, m) for k in ("dgrad", "first", "out") for m in ("neighbour_exponent", "neighbour_row_cos") if m in APPLICABLE[k]])
def test_mutation_breaks_the_bound_on_random(kernel, mutation):
    """At the full depth, on the recipe of the sequence: a wrong exponent (tile magnitudes spread over 1e4) and a wrong row's cosine."""
    if kernel == "out":
        res = _out_layer("random", 2048, mutation)
    else:
        res = _single(kernel, R.make_single("random", 2048, 241, 256), 241, 256, mutation)
    print(f"mutation {kernel} random {mutation}: factor {max(res.values()):.1f}")
    assert max(res.values()) >= 4.0, res


K_INVARIANCE = 60


@pytest.mark.parametrize("case", list(R.SHAPES))
def test_scaling_by_two_to_the_k_keeps_every_value_a_normal_float(case):
    """The GPU file multiplies d_x by 2^-60 and 2^60 and expects the same bits with another exponent.  That can only hold while no value that
    is stored leaves the normal f32 range: the smallest non-zero and the largest magnitude of every matrix of the reference sequence, with 2^6 to spare for
    the kernels' own error."""
    inp = R.to_torch(R.make_inputs("random", case, 2048))
    ns = R.SHAPES[case]
    ref, _ = R.out_layer(inp["d_x"], inp["sines"][3], inp["w_out"], 5, ns[3])
    mats = [inp["d_x"].double(), ref["g"], ref["d_w"], ref["d_b"], ref["d_b_prev"]]
    g = ref["g"].float()
    for l in (3, 2, 1):
        tm = R.tile_max_bits(g, ns[l])
        mats.append(R.weight_grad(g, inp["sines"][l - 1], ns[l]))
        if l > 1:
            r, _ = R.input_grad(g, tm, inp["weights"][l], inp["sines"][l - 1], ns[l - 1], ns[l])
            mats += [r["g"], r["d_b"]]
            g = r["g"].float()
        else:
            r, _ = R.first_layer(g, tm, inp["weights"][1], inp["sines"][0], inp["x0"], 15, ns[0], ns[1])
            mats += [r["d_w0"], r["d_b0"]]
    lo = min(float(m.abs()[m != 0].min()) for m in mats)
    hi = max(float(m.abs().max()) for m in mats)
    print(f"{case}: smallest non-zero {lo:.3e}, largest {hi:.3e}")
    assert lo * 2.0 ** -K_INVARIANCE >= 2.0 ** -120 and hi * 2.0 ** K_INVARIANCE <= 2.0 ** 120
