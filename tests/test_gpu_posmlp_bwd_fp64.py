"""The kernels of the pos_mlp f16 backward pass -- `matpbr_mlp_out_layer_bwd_tmax`, `matpbr_mlp_layer_bwd_weight_blk`, `matpbr_mlp_layer_bwd_input_blk`,
`matpbr_mlp_first_layer_bwd_blk` and the one `matpbr_mlp_reduce_jobs` behind them -- each against an fp64 restatement of its own operation, evaluated
on the inputs the kernel actually received, under the error bound that tests/posmlp_bwd_fp64.py derives (no constant here or there is a reading
from a GPU; tests/test_posmlp_bwd_fp64_host.py shows on the CPU that the bound holds for the documented arithmetic and that a lost cross
product, a wrong exponent, a wrong row's cosine and a missed sign bit all break it).  Every test prints max(err / bound) per kernel and output."""
import ctypes

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import posmlp_bwd_fp64 as R    # noqa: E402

_cache = {}


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _inputs(recipe, case, M, zero_tile, dev):
    key = (recipe, case, M, zero_tile)
    if key not in _cache:
        _cache[key] = R.to_torch(R.make_inputs(recipe, case, M, zero_tile=zero_tile), dev)
    return _cache[key]


def _sequence(inp, case, dev, d_x=None):
    """The backward sequence as `MlpEngine.backward_raw` drives it with bwd_f16: every fold deferred, one `mlp_reduce_jobs` at the end.  The gradient
    matrices start as NaN: what a kernel does not write, and must not read as data, stays NaN.  Returns every output, the g matrices whole."""
    from materialist_amd import _lib, ops

    ns, L = R.SHAPES[case], 4
    d_x = inp["d_x"] if d_x is None else d_x
    M = d_x.shape[0]
    s, x0, w_out = inp["sines"], inp["x0"], inp["w_out"]
    wt = [None] + [ops.mlp_split_weights(inp["weights"][l], ns[l - 1], ns[l], transposed=True, f16=True) for l in range(1, L)]
    g = [None] + [torch.full((M, 256), float("nan"), device=dev) for _ in range(1, L)]
    tmax = [None] + [ops.mlp_tile_max(M, dev) for _ in range(1, L)]
    out = {"d_w_out": torch.zeros(5, 256, device=dev), "d_b_out": torch.zeros(5, device=dev), "d_w0": torch.zeros(ns[0], 16, device=dev)}
    for l in range(L):
        out[f"d_b{l}"] = torch.zeros(ns[l], device=dev)
    for l in range(1, L):
        out[f"d_w{l}"] = torch.zeros(ns[l], 256, device=dev)
    jobs, nj = (_lib.ReduceJob * 16)(), 0
    slot = lambda k: (ctypes.cast(ctypes.byref(jobs, k * ctypes.sizeof(_lib.ReduceJob)), ctypes.c_void_p), f"_fp64{k}")
    ops.mlp_out_layer_bwd_tmax(d_x, s[L - 1], w_out, g[L - 1], tmax[L - 1], out["d_w_out"], out["d_b_out"], out[f"d_b{L - 1}"], 5, ns[L - 1], defer=slot(nj))
    nj += 1
    for l in range(L - 1, 0, -1):
        ops.mlp_layer_bwd_weight_blk(g[l], tmax[l], s[l - 1], ns[l], 256, out=out[f"d_w{l}"], defer=slot(nj))
        nj += 1
        if l == 1:
            ops.mlp_first_layer_bwd_blk(g[l], tmax[l], wt[l], s[0], x0, out["d_w0"], R.D0, ns[0], ns[l], out["d_b0"], defer=slot(nj))
            nj += 2
        else:
            ops.mlp_layer_bwd_input_blk(g[l], tmax[l], wt[l], s[l - 1], g[l - 1], ns[l - 1], ns[l], out[f"d_b{l - 1}"], tmax[l - 1], defer=slot(nj))
            nj += 1
    ops.mlp_reduce_jobs(jobs, nj, d_x)
    torch.cuda.synchronize()
    for l in range(1, L):
        out[f"g{l}"], out[f"tmax{l}"] = g[l], tmax[l]
    return out


def _report(tag, res):
    print(f"{tag}: " + " ".join(f"{k}={v:.3f}" for k, v in res.items()))


def _check(tag, inp, out, case, zero_tile):
    res, wref = R.check_sequence(inp, out, case, zero_tile)
    _report(tag, res)
    assert all(v <= 1.0 for v in res.values()), {k: v for k, v in res.items() if not v <= 1.0}
    return wref


def _weight_gradients_against_f32(tag, inp, out, wref, case, kernels):
    """Beyond one slab of the weight gradient (M > 256) its worst-case bound is vacuous; there the project's criterion holds instead: against the
    same fp64 reference, at most 1.5 x the error of the exact-f32 kernel (errors as the largest over the matrix, relative to its largest entry)."""
    from materialist_amd import ops

    ns, res = R.SHAPES[case], {}
    for l in (3, 2, 1):
        ref = wref[l][0]
        top = float(ref.abs().max())
        g0 = out[f"g{l}"].clone()
        g0[:, ns[l]:] = 0.0
        e32 = float((ops.mlp_layer_bwd_weight(g0, inp["sines"][l - 1], ns[l], 256).double() - ref).abs().max()) / top
        for k in kernels:
            d_w = out[f"d_w{l}"]
            if k != 1:
                was = ops.mlp_set_wgrad_kernel(k)
                try:
                    d_w = ops.mlp_layer_bwd_weight_blk(out[f"g{l}"], out[f"tmax{l}"], inp["sines"][l - 1], ns[l], 256)
                    torch.cuda.synchronize()
                finally:
                    ops.mlp_set_wgrad_kernel(was)
                assert was == 1                                  # the sequence ran on the default kernel
            e = float((d_w.double() - ref).abs().max()) / top
            res[f"wgrad{l}.kernel{k}"] = e / e32
            assert torch.isfinite(d_w).all() and e <= 1.5 * e32, (l, k, e, e32)
    _report(f"{tag} weight gradients, error / exact-f32 kernel's", res)


@pytest.mark.parametrize("case,M", [(c, M) for c in R.SHAPES for M in (128, 2048, 9216)] + [("wide", 128 * 520)])
def test_teacher_forced_sequence(case, M):
    """M = 128: one tile, one step per workgroup.  2048: 16 tiles, the output layer's slabs (4 rows) never straddle a tile.  9216: 72 tiles, slabs of
    12 rows straddle tile boundaries, so a tile's maximum is put together from two slabs' flushes.  128 x 520 (`wide`): more tiles than workgroups --
    the persistent input-gradient and first-layer kernels change exponent between tiles; another zero tile.  The weight gradient: under the bound at
    M = 128, against the exact-f32 kernel at the larger row counts, both of its kernels."""
    dev = _cuda()
    zt = 7 if M == 128 * 520 else 5
    inp = _inputs("random", case, M, zt, dev)
    out = _sequence(inp, case, dev)
    wref = _check(f"sequence {case} M={M}", inp, out, case, zt)
    if M > 256:
        _weight_gradients_against_f32(f"sequence {case} M={M}", inp, out, wref, case, (1, 0))


def _single(kernel, p, n_prev, n_red, dev):
    """One kernel on operands of its own (no deferral: it folds its partial sums itself): {output: max err / bound}."""
    from materialist_amd import ops

    t = R.to_torch(p, dev)
    M = t["g"].shape[0]
    if kernel == "wgrad":
        dw = ops.mlp_layer_bwd_weight_blk(t["g"], t["tmax"], t["s_prev"], n_red, 256)
        torch.cuda.synchronize()
        return {"d_w": R.ratio(dw, R.weight_grad(t["g"], t["s_prev"], n_red), R.weight_grad_bound(t["g"], t["tmax"], t["s_prev"], n_red))}
    wt = ops.mlp_split_weights(t["w"], n_prev, n_red, transposed=True, f16=True)
    db = torch.zeros(n_prev, device=dev)
    if kernel == "dgrad":
        gp, tm = torch.full((M, 256), float("nan"), device=dev), ops.mlp_tile_max(M, dev)
        ops.mlp_layer_bwd_input_blk(t["g"], t["tmax"], wt, t["s_prev"], gp, n_prev, n_red, db, tm)
        torch.cuda.synchronize()
        ref, bnd = R.input_grad(t["g"], t["tmax"], t["w"], t["s_prev"], n_prev, n_red)
        assert torch.equal(tm, R.tile_max_bits(gp, n_prev))
        return {"g": R.ratio(gp[:, :n_prev], ref["g"], bnd["g"]), "d_b": R.ratio(db, ref["d_b"], bnd["d_b"]), "tmax": R.tmax_ratio(tm, ref["g"], bnd["g"], n_prev)}
    assert kernel == "first"
    dw0 = torch.zeros(n_prev, 16, device=dev)
    ops.mlp_first_layer_bwd_blk(t["g"], t["tmax"], wt, t["s_prev"], t["x0"], dw0, R.D0, n_prev, n_red, db)
    torch.cuda.synchronize()
    ref, bnd = R.first_layer(t["g"], t["tmax"], t["w"], t["s_prev"], t["x0"], R.D0, n_prev, n_red)
    return {"d_w0": R.ratio(dw0, ref["d_w0"], bnd["d_w0"]), "d_b0": R.ratio(db, ref["d_b0"], bnd["d_b0"])}


# kernel, M, n_prev, n_red.  Beside the full depth (K = 256 columns, 2048 or 256 rows), the depths at which tests/test_posmlp_bwd_fp64_host.py shows that a
# lost cross product stands four times above the bound: 64 columns; 128 rows for the weight gradient, 256 for the first layer's sums over rows
PROBES = [("dgrad", 2048, 256, 256), ("dgrad", 2048, 241, 64), ("first", 2048, 241, 256), ("first", 256, 241, 64), ("wgrad", 256, 256, 256),
          ("wgrad", 128, 256, 256)]


@pytest.mark.parametrize("kernel,M,n_prev,n_red", PROBES)
def test_piece_probe(kernel, M, n_prev, n_red):
    """`coherent`: every operand positive with a second f16 piece as large as a remainder can be.  A kept cross product that is lost or misplaced is a
    bias of 2^-12 of the sum here; nothing averages out."""
    dev = _cuda()
    res = _single(kernel, R.make_single("coherent", M, n_prev, n_red, zero_tile=5 if M > 640 else 99), n_prev, n_red, dev)
    _report(f"piece probe {kernel} M={M} n_prev={n_prev} n_red={n_red}", res)
    assert all(v <= 1.0 for v in res.values()), res


def test_piece_probe_output_layer():
    """The output layer forms no f16 pieces (f32 fma chains): `coherent` holds it to J x 2^-24 of the sum of magnitudes, every cosine negative."""
    dev = _cuda()
    inp = _inputs("coherent", "wide", 2048, 5, dev)
    ref, bnd = R.out_layer(inp["d_x"], inp["sines"][3], inp["w_out"], 5, 256)
    out = _sequence(inp, "wide", dev)
    res = {k: R.ratio(out[n], ref[k], bnd[k]) for k, n in (("d_w", "d_w_out"), ("d_b", "d_b_out"), ("d_b_prev", "d_b3"))}
    res["g"] = R.ratio(out["g3"], ref["g"], bnd["g"])
    res["tmax"] = R.tmax_ratio(out["tmax3"], ref["g"], bnd["g"], 256)
    _report("piece probe out M=2048", res)
    assert torch.equal(out["tmax3"], R.tile_max_bits(out["g3"], 256))
    assert all(v <= 1.0 for v in res.values()), res


@pytest.mark.parametrize("kernel,M,n_prev,n_red", [("dgrad", 2048, 241, 256), ("dgrad", 2048, 256, 241), ("first", 2048, 241, 256), ("wgrad", 256, 256, 241)])
def test_magnitude_edges_inside_a_tile(kernel, M, n_prev, n_red):
    """`range`: a tile whose largest element is exactly a power of two, one whose largest is one ulp below a power of two, elements at 2^-15, 2^-17,
    2^-24 and 2^-30 of their tile's largest (the last two live on the absolute floor of the second piece)."""
    dev = _cuda()
    res = _single(kernel, R.make_single("range", M, n_prev, n_red, zero_tile=5 if M > 640 else 99), n_prev, n_red, dev)
    _report(f"range {kernel} M={M} n_prev={n_prev} n_red={n_red}", res)
    assert all(v <= 1.0 for v in res.values()), res


K_INVARIANCE = 60      # tests/test_posmlp_bwd_fp64_host.py: no stored value of the sequence leaves the normal f32 range at 2^-60 or 2^60


@pytest.mark.parametrize("case", list(R.SHAPES))
def test_exponent_invariance(case):
    """Block scaling is by powers of two and all of the arithmetic is linear in g: d_x times 2^k gives every float output times 2^k, bit for bit,
    and every tile maximum with k added to its exponent field."""
    dev = _cuda()
    inp = _inputs("random", case, 2048, 5, dev)
    base = _sequence(inp, case, dev)
    ns = R.SHAPES[case]
    for k in (-K_INVARIANCE, K_INVARIANCE):
        got = _sequence(inp, case, dev, d_x=inp["d_x"] * 2.0 ** k)
        for name in sorted(base):
            a, b = got[name], base[name]
            if name.startswith("tmax"):
                want = torch.where(b != 0, b + (k << 23), b)
                assert torch.equal(a, want), (name, k, int((a != want).sum()))
            else:
                if name.startswith("g"):
                    n = ns[int(name[1:])]
                    a, b = a[:, :n], b[:, :n]
                want = b * 2.0 ** k
                assert torch.isfinite(a).all() and torch.equal(a, want), (name, k, int((a != want).sum()))
    print(f"exponent invariance {case}: every output is the same bits at 2^-{K_INVARIANCE} and 2^{K_INVARIANCE}")


def _edge_d_x(inp, which):
    """d_x rescaled per tile so that its largest element in each tile is `target`: g3 lands within a decade below (|w_out| <= 1/16, five terms)."""
    d_x = inp["d_x"].double()
    T = d_x.shape[0] // 128
    top = d_x.abs().reshape(T, -1).amax(1)
    target = top.clone()
    if which == "huge":
        target[:] = 1e31
    elif which == "tiny_tiles_among_ordinary":
        target[3], target[9] = 1e-35, 1e-39                 # g3 near 1e-36, and subnormal (near 1e-40)
    else:
        target[:] = 1e-35
    scale = torch.where(top > 0, target / top.clamp_min(1e-300), torch.ones_like(top))
    return (d_x * scale.repeat_interleave(128)[:, None]).float()


@pytest.mark.parametrize("which", ["huge", "tiny_tiles_among_ordinary", "every_tile_tiny"])
@pytest.mark.parametrize("case", list(R.SHAPES))
def test_magnitude_edges_of_whole_tiles(case, which):
    """Tile maxima near 1e30; one tile near 1e-36 and one subnormal tile (1e-40) among ordinary ones; every tile near 1e-36.  Everything is finite and
    within the bound, whose floor for tiles below 2^-113 is what include/matpbr_mlp.h guarantees: the scale stops at 2^126, such a tile is carried
    to 2^-151, results round as f32 subnormals do.  (Before the exponent was limited the scale of such a tile was +inf: its elements came out inf, its zeros NaN.)"""
    dev = _cuda()
    inp = _inputs("random", case, 2048, 5, dev)
    d_x = _edge_d_x(inp, which)
    out = _sequence(inp, case, dev, d_x=d_x)
    for name, v in out.items():
        if v.dtype == torch.float32:
            n = R.SHAPES[case][int(name[1:])] if name.startswith("g") else v.shape[-1]
            assert torch.isfinite(v[..., :n]).all(), name
    top = out["tmax3"].view(torch.float32)
    if which == "huge":
        assert 1e28 < float(top[top > 0].min()) and float(top.max()) < 1e32
    elif which == "every_tile_tiny":
        assert 1e-38 < float(top[top > 0].min()) and float(top.max()) < 2.0 ** -114
    else:
        assert 1e-38 < float(top[3]) < 2.0 ** -114 and 0 < float(top[9]) < 2.0 ** -126
    seq = dict(inp)
    seq["d_x"] = d_x
    wref = _check(f"edges {case} {which}", seq, out, case, 5)
    _weight_gradients_against_f32(f"edges {case} {which}", inp, out, wref, case, (1,))
