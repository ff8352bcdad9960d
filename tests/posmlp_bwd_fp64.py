"""fp64 restatements of the four operations of the pos_mlp f16 backward pass, a derived error bound per output element, a numpy emulation of the
documented arithmetic (with switches that break it on purpose) and the input recipes of tests/test_posmlp_bwd_fp64_host.py and
tests/test_gpu_posmlp_bwd_fp64.py.  Plain numpy / torch: nothing here touches the library.

The restatements and bounds are torch functions that run on whatever device their arguments live on (fp64 throughout); each takes exactly what
the kernel takes -- the f32 gradient matrix and the tile maxima it was handed, the f32 weights, the stored sign-carrying sines.

THE COSINE.  A stored sine carries the sign of its cosine in its last mantissa bit (`pack_cos_sign`).  The reference decodes it the way the
kernel does: sign = that bit, magnitude = sqrt(max(0, 1 - s^2)) of the float as stored, bit included.  The kernel forms 1 - s^2 with one fma
(one rounding, 2^-24 relative, halved by the root) and takes a hardware square root (1 ulp, 2^-23), so against this reference
    |cos_kernel - cos_ref| <= (2^-23 + 2^-25) |cos_ref| = U_COS |cos_ref|.
(The 1.2e-7 / |cos| of the kernels' comments is the FORWARD pass's error against the true angle; test_sines_that_carry_the_sign_of_their_cosine
owns that.)

THE BOUND.  Notation: s = 2^(14 - e) the tile's scale (e from frexp of the tile maximum, limited below by -112; 14 for a tile of zeros),
y = g s (exact: a power of two), b = 256 w (exact), K the reduction depth.
 (1) Two round-to-nearest f16 pieces.  f16 keeps 11 significant bits: p1 = rn(y) leaves r = y - p1 with |r| <= 2^-11 |y|, exactly representable
     in f32 (v_fma_mix_f32).  r has at most 12 significant bits above the last place of the f32 number y (24 - 11 - the sign the remainder carries),
     so p2 = rn(r) drops at most ONE bit: |y - p1 - p2| <= 2^-23 |y| (one f32 ulp at the bottom of a binade -- not 2^-24: x = 1 + 2^-12 + 2^-23
     ties to even and loses exactly 2^-23).  Where r is below 2^-14 (always when |y| < 2^-3) p2 is an f16 subnormal with spacing 2^-24:
     |y - p1 - p2| <= 2^-25, absolute.  Both cases: dy = max(2^-23 |y|, 2^-25).  With the tile's largest in [2^13, 2^14) the floor is at most
     2^-38 OF THE LARGEST (include/matpbr_mlp.h said 2^-39: corrected there), and elements down to 2^-16 of the largest are in the relative regime.
     A tile whose exponent hit the limit (largest below 2^-113) has s = 2^126 and is carried to 2^-25 / 2^126 = 2^-151, absolute.
 (2) The low x low product is not formed: |p2| <= lo(y) = max(2^-11 |y|, 2^-24), so |p2 q2| <= lo(y) lo(b) (2^-22 |y b| in the relative regime).
 (3) f32 accumulation.  The f16 products are exact in f32.  3 K terms are summed by the matrix core in an order and a rounding mode that are not
     documented: each of at most 3 K - 1 additions (adding to a zero accumulator is exact) is charged one ulp, U_MM = 2^-23, of the sum of
     magnitudes -- the worst case, linear in the depth.  Sums formed by ordinary f32 instructions (fma chains of the output layer, column sums,
     the folds of partial sums, the exact-f32 matrix instruction of the first layer, which is an fma chain) round to nearest: U_ADD = 2^-24 per
     term, again at most one per term whatever the tree.
 (4) acc 2^(e - 14) 2^-8 is exact unless the result is an f32 subnormal (2^-150, half the spacing, absolute: TINY per rounding).
 (5) v cos: one rounding (2^-24) and the cosine's U_COS.
Summed, for one element of an input gradient (A = |y| |b| summed over k, everything in scaled units and divided by 256 s at the end):
    E_acc = (|y| + dy)(|b| + db) - |y| |b| + lo(y) lo(b) + 3 K U_MM (1 + 2^-9) |y| |b|        (summed over k)
    bound = (1 + 2^-10) (E_acc / (256 s) |cos| + (2^-24 + U_COS) |ref|) + 3 TINY
(1 + 2^-9 covers the magnitudes of the two small products, 1 + 2^-10 every second-order term.)  A column sum over M rows adds the rows' bounds
and M U_ADD times the sum of magnitudes.  The weight gradient is the same with x in the place of b (no 256, no cosine) and K = the rows of the
workgroup's slab; the first layer's dW0 propagates the bound of G0 through |x0| and adds M U_ADD of the sum of magnitudes.  The output layer
is f32 fma chains: J U_ADD of |d_x| |w| summed, then (5).  None of these constants is a reading from a GPU.
"""
import numpy as np
import torch

TILE = 128
U_REP, FLOOR = 2.0 ** -23, 2.0 ** -25        # (1): relative / absolute (scaled units) error of two f16 pieces
LO_REL, LO_ABS = 2.0 ** -11, 2.0 ** -24      # (2): size of the second piece
U_MM, U_ADD = 2.0 ** -23, 2.0 ** -24         # (3)
TINY = 2.0 ** -149                           # (4) (a whole spacing: the f32 result is compared, not its exact value)
U_COS = 2.0 ** -23 + 2.0 ** -25
SLACK = 1.0 + 2.0 ** -10
E_MIN = -112                                 # block_scale's limit: 2^(14 - e) <= 2^126
MUTATIONS = ("drop_p1q2", "drop_p2q1", "neighbour_exponent", "neighbour_row_cos", "skip_sign")


# ---------------------------------------------------------------------------------------------------------------- shared pieces (torch, fp64)
def decode_cos(s):
    """cos from stored sign-carrying sines in fp64, as `cos_from_packed_sin` defines it (f32 as the kernels store them; f64 sines, for the
    proof of the restatements against autograd, carry the sign in THEIR last mantissa bit)."""
    neg = (s.contiguous().view(torch.int32 if s.dtype == torch.float32 else torch.int64) & 1).bool()
    mag = (1.0 - s.double() ** 2).clamp_min(0.0).sqrt()
    return torch.where(neg, -mag, mag)


def tile_exponent(tmax_bits):
    """e per tile from the f32 bit patterns of the tile maxima (int32 tensor), as `block_scale`: frexp, limited below, 14 for zero / not finite."""
    mx = tmax_bits.contiguous().view(torch.float32).double()
    _, e = torch.frexp(mx)
    e = e.clamp_min(E_MIN)
    return torch.where((mx > 0) & (mx < 3.0e38), e, torch.full_like(e, 14)).to(torch.int64)


def tile_max_bits(g, n):
    """Brute force: the f32 bit pattern of the largest |g| over each tile's rows and columns < n."""
    M = g.shape[0]
    return g[:, :n].abs().reshape(M // TILE, TILE * n).amax(1).contiguous().view(torch.int32)


def _rows(per_tile):
    return per_tile.repeat_interleave(TILE)[:, None]


def _piece_err(y):                            # (a zero is carried exactly)
    return torch.where(y > 0, torch.maximum(U_REP * y, torch.full_like(y, FLOOR)), torch.zeros_like(y))


def _piece_lo(y):
    return torch.where(y > 0, torch.maximum(LO_REL * y, torch.full_like(y, LO_ABS)), torch.zeros_like(y))


def _product_bound(ya, ba, depth):
    """E_acc for |y| [M, K] and |b| [K, N] (scaled units)."""
    A = ya @ ba
    return (ya + _piece_err(ya)) @ (ba + _piece_err(ba)) - A + _piece_lo(ya) @ _piece_lo(ba) + 3 * depth * U_MM * (1 + 2.0 ** -9) * A


# ---------------------------------------------------------------------------------------------------------------- the four restatements
def out_layer(d_x, s, w_out, J, n_prev):
    """matpbr_mlp_out_layer_bwd_tmax.  d_x [M, 8], s [M, 256] sign-carrying sines, w_out [J, 256].  Returns fp64 references and bounds."""
    M = d_x.shape[0]
    dx, w, c = d_x[:, :J].double(), w_out[:J, :n_prev].double(), decode_cos(s[:, :n_prev])
    pre = dx @ w
    g = pre * c
    A = dx.abs() @ w.abs()
    b_g = SLACK * (J * U_ADD * A * c.abs() + (U_ADD + U_COS) * g.abs()) + (J + 2) * TINY
    sd = s.double()
    ref = {"g": g, "d_w": dx.t() @ sd, "d_b": dx.sum(0), "d_b_prev": g.sum(0), "tmax": tile_max_bits(g.float(), n_prev)}
    bound = {"g": b_g, "d_w": SLACK * M * U_ADD * (dx.abs().t() @ sd.abs()) + TINY, "d_b": SLACK * M * U_ADD * dx.abs().sum(0) + TINY,
             "d_b_prev": SLACK * (b_g.sum(0) + M * U_ADD * g.abs().sum(0)) + TINY}
    return ref, bound


def input_grad(g, tmax_bits, w, s_prev, n_prev, n_red):
    """matpbr_mlp_layer_bwd_input_blk.  g [M, >= n_red] f32 and the tile maxima the kernel is handed, w [n_red, >= n_prev] the forward weight
    (the kernel's operand is the f16 image of its transpose), s_prev [M, 256].  Returns fp64 references and bounds for g_prev and its column sums."""
    M = g.shape[0]
    gd, wd, c = g[:, :n_red].double(), w[:n_red, :n_prev].double(), decode_cos(s_prev[:, :n_prev])
    scale = torch.ldexp(torch.ones(M // TILE, dtype=torch.float64, device=g.device), 14 - tile_exponent(tmax_bits))
    rs = _rows(scale)
    ref = (gd @ wd) * c
    e_acc = _product_bound(gd.abs() * rs, 256.0 * wd.abs(), n_red) / (256.0 * rs)
    b = SLACK * (e_acc * c.abs() + (U_ADD + U_COS) * ref.abs()) + 3 * TINY
    refs = {"g": ref, "d_b": ref.sum(0), "tmax": tile_max_bits(ref.float(), n_prev)}
    return refs, {"g": b, "d_b": SLACK * (b.sum(0) + M * U_ADD * ref.abs().sum(0)) + TINY}


def first_layer(g, tmax_bits, w, s0, x0, d0, n0, n_red):
    """matpbr_mlp_first_layer_bwd_blk: G0 as in `input_grad` (never stored), d_w0[n, k] = sum_m G0[m, n] x0[m, k] (k < d0, zero beyond), d_b0 its
    column sums."""
    M = g.shape[0]
    r, b = input_grad(g, tmax_bits, w, s0, n0, n_red)
    x = x0[:, :16].double().clone()
    x[:, d0:] = 0.0
    G0 = r["g"]
    refs = {"d_w0": G0.t() @ x, "d_b0": r["d_b"]}
    return refs, {"d_w0": SLACK * (b["g"].t() @ x.abs() + M * U_ADD * (G0.abs().t() @ x.abs())) + TINY, "d_b0": b["d_b"]}


def weight_grad(g, x, N):
    """matpbr_mlp_layer_bwd_weight_blk, reference only: d_w = g[:, :N]^T x over all 256 columns of x (the x0 tail of a 241 layer included)."""
    return g[:, :N].double().t() @ x.double()


def weight_grad_bound(g, tmax_bits, x, N):
    """The bound of one workgroup's slab: M <= 256 rows, ONE exponent (the largest of the tile maxima)."""
    M = g.shape[0]
    assert M <= 256, "beyond one slab the worst-case bound is vacuous: the tests compare with the exact-f32 kernel there"
    e = tile_exponent(tmax_bits.contiguous().view(torch.int32).max().reshape(1))
    scale = torch.ldexp(torch.ones(1, dtype=torch.float64, device=g.device), 14 - e)
    return SLACK * _product_bound((g[:, :N].double().abs() * scale).t().contiguous(), x.double().abs(), M) / scale + TINY


# ---------------------------------------------------------------------------------------------------------------- the emulation (numpy, CPU)
def _np_exponent(tmax_bits):
    mx = np.asarray(tmax_bits).view(np.float32).astype(np.float64)
    _, e = np.frexp(mx)
    return np.where((mx > 0) & (mx < 3.0e38), np.maximum(e, E_MIN), 14).astype(np.int64)


def _np_split(y):
    with np.errstate(over="ignore", invalid="ignore"):
        p1 = y.astype(np.float16)
        p2 = (y - p1.astype(np.float32)).astype(np.float16)
    return p1.astype(np.float32), p2.astype(np.float32)


def _np_three(y, b, mutation):
    """p2 q1 + p1 q2 + p1 q1 with f32 sums; y [M, K], b [K, N] f32."""
    p1, p2 = _np_split(y)
    q1, q2 = _np_split(b)
    with np.errstate(over="ignore", invalid="ignore"):
        acc = p1 @ q1
        if mutation != "drop_p1q2":
            acc = acc + p1 @ q2
        if mutation != "drop_p2q1":
            acc = acc + p2 @ q1
    return acc.astype(np.float32)


def _np_cos(s, mutation):
    s = np.ascontiguousarray(s, dtype=np.float32)
    mag = np.sqrt(np.maximum((1.0 - s.astype(np.float64) ** 2).astype(np.float32), np.float32(0.0)))
    neg = (s.view(np.uint32) & 1).astype(bool)
    c = mag if mutation == "skip_sign" else np.where(neg, -mag, mag)
    return np.roll(c, -1, axis=0) if mutation == "neighbour_row_cos" else c


def emulate_input_grad(g, tmax_bits, w, s_prev, n_prev, n_red, mutation=None):
    """The documented arithmetic of the input gradient: one exponent per tile by frexp, two f16 pieces of g 2^(14 - e) and of 256 w, three
    products, an f32 sum, scaled back, times the decoded cosine.  Returns (g_prev [M, n_prev] f32, column sums f32, outgoing tile maxima as bits)."""
    M = g.shape[0]
    e = _np_exponent(tmax_bits)
    if mutation == "neighbour_exponent":
        e = np.roll(e, -1)
    e = np.repeat(e, TILE)[:, None]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        y = (g[:, :n_red].astype(np.float32) * np.ldexp(np.float32(1.0), (14 - e).astype(np.int32))).astype(np.float32)
        acc = _np_three(y, np.ascontiguousarray(w[:n_red, :n_prev].astype(np.float32) * np.float32(256.0)), mutation)
        v = (acc * np.ldexp(np.float32(1.0), (e - 22).astype(np.int32))).astype(np.float32)
        out = (v * _np_cos(s_prev[:, :n_prev], mutation)).astype(np.float32)
    return out, out.sum(0, dtype=np.float32), np.abs(out).reshape(M // TILE, -1).max(1).view(np.uint32).view(np.int32)


def emulate_first_layer(g, tmax_bits, w, s0, x0, d0, n0, n_red, mutation=None):
    G0, db, _ = emulate_input_grad(g, tmax_bits, w, s0, n0, n_red, mutation)
    x = np.array(x0[:, :16], dtype=np.float32)
    x[:, d0:] = 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        return (G0.T @ x).astype(np.float32), db


def emulate_weight_grad(g, tmax_bits, x, N, mutation=None):
    """One slab (M <= 256): one exponent from the largest tile maximum, x as it is."""
    e = int(_np_exponent(np.asarray(tmax_bits).view(np.uint32).max().reshape(1).view(np.int32))[0])
    y = (g[:, :N].astype(np.float32) * np.ldexp(np.float32(1.0), 14 - e)).astype(np.float32)
    return (_np_three(np.ascontiguousarray(y.T), np.ascontiguousarray(x, dtype=np.float32), mutation) * np.ldexp(np.float32(1.0), e - 14)).astype(np.float32)


def emulate_out_layer(d_x, s, w_out, J, n_prev, mutation=None):
    """f32 throughout (the output layer forms no f16 pieces): the dot product, times the decoded cosine; its tile maxima."""
    pre = (d_x[:, :J].astype(np.float32) @ w_out[:J, :n_prev].astype(np.float32)).astype(np.float32)
    g = (pre * _np_cos(s[:, :n_prev], mutation)).astype(np.float32)
    return g, np.abs(g).reshape(g.shape[0] // TILE, -1).max(1).view(np.uint32).view(np.int32)


# ---------------------------------------------------------------------------------------------------------------- input recipes (seeded numpy)
SHAPES = {"wide": [256, 256, 256, 256], "ragged": [241, 256, 241, 256]}     # columns of the four sine layers (241: a skip layer, x0 in its tail)
D0, J_OUT = 15, 5


def pack_sines(pre, dtype=np.float32):
    """sin(pre) with the sign of cos(pre) in the last mantissa bit."""
    u = np.uint32 if dtype == np.float32 else np.uint64
    s = np.sin(pre).astype(dtype)
    bits = s.view(u)
    bits &= ~u(1)
    bits |= (np.cos(pre) < 0).astype(u)
    return s


def _coherent(rng, shape, exp2=0, odd=False):
    """Positive numbers h (1 + 2^-12 (1 - 2^-6)) 2^exp2 with h in [1, 2) on six significant bits: exactly representable in f32, and the second f16
    piece of each is as large as a remainder can be, always positive.  odd: the last of the six bits is set -- it is then the last mantissa bit of
    the f32 number, so a sine of this form carries a NEGATIVE cosine: one sign throughout, and sums over rows stay coherent as well."""
    h = (32 + (rng.integers(0, 16, shape) * 2 + 1 if odd else rng.integers(0, 32, shape))) / 32.0
    return (h * (1.0 + 2.0 ** -12 * (1.0 - 2.0 ** -6)) * 2.0 ** exp2).astype(np.float32)


def make_inputs(recipe, case, M, zero_tile=5, seed=0):
    """d_x [M, 8], x0 [M, 16], four sine matrices [M, 256], four forward weights [256, 256] (entry 0 unused) and w_out [5, 256]: what the backward
    sequence is driven with.  `random`: the recipe of tests/test_gpu_cache_plan.py::_make_inputs (1e-6 gradients, tile magnitudes spread over 1e4,
    one all-zero tile; the columns 1e-3 below their neighbours are `make_g`'s, d_x has five); `coherent`: see `_coherent`."""
    ns = SHAPES[case]
    T = M // TILE
    rng = np.random.default_rng(4000 + sum(ns) + M + seed)
    d_x, x0 = np.zeros((M, 8), dtype=np.float32), np.zeros((M, 16), dtype=np.float32)
    if recipe == "random":
        mag = np.clip(np.exp(rng.standard_normal(T) * 2.0), 1e-2, 1e2).astype(np.float32)
        d_x[:, :5] = rng.standard_normal((M, 5), dtype=np.float32) * np.float32(1e-6) * np.repeat(mag, TILE)[:, None]
        x0[:, :15] = rng.standard_normal((M, 15), dtype=np.float32)
        x0[:, 0] = rng.integers(0, 512, M).astype(np.float32)
        sines = [pack_sines(rng.standard_normal((M, 256)) * 3.0) for _ in ns]
        weights = [((rng.random((256, 256), dtype=np.float32) * 2 - 1) / 16).astype(np.float32) for _ in ns]
        w_out = ((rng.random((5, 256), dtype=np.float32) * 2 - 1) / 16).astype(np.float32)
    elif recipe == "coherent":
        d_x[:, :5] = _coherent(rng, (M, 5), -20) * np.repeat(2.0 ** ((5 * np.arange(T)) % 13 - 6), TILE)[:, None].astype(np.float32)
        x0[:, :15] = _coherent(rng, (M, 15))
        sines = [_coherent(rng, (M, 256), -1, odd=True) for _ in ns]      # in [0.5, 1), every cosine negative
        weights = [_coherent(rng, (256, 256), -5) for _ in ns]
        w_out = _coherent(rng, (5, 256), -5)
    else:
        raise ValueError(recipe)
    if T > 1:
        d_x[TILE * zero_tile:TILE * (zero_tile + 1)] = 0.0
    for s, n in zip(sines, ns):
        if n < 256:
            s[:, n:] = x0[:, :256 - n]
    return {"d_x": d_x, "x0": x0, "sines": sines, "weights": weights, "w_out": w_out}


def make_g(recipe, M, n, zero_tile=5, seed=0):
    """A gradient matrix [M, 256] for one kernel on its own (columns at and beyond n are NaN: scratch) and the bits of its tile maxima.
    `random`: 1e-6, tile magnitudes spread over 1e4, every seventh column 1e-3 below, one all-zero tile.  `coherent`: `_coherent` times a power of two
    per tile.  `range`: `random`, then tile 0's largest is exactly a power of two, tile 1's is one ulp below one, and tile 2 (tile 0 where there are
    only two) holds elements at 2^-15, 2^-17, 2^-24 and 2^-30 of its largest."""
    T = M // TILE
    rng = np.random.default_rng(7000 + M + n + seed)
    if recipe == "coherent":
        g = _coherent(rng, (M, 256), -20) * np.repeat(2.0 ** ((5 * np.arange(T)) % 13 - 6), TILE)[:, None].astype(np.float32)   # neighbours: 2^5 or 2^-8 apart
    else:
        mag = np.clip(np.exp(rng.standard_normal(T) * 2.0), 1e-2, 1e2).astype(np.float32)
        g = rng.standard_normal((M, 256), dtype=np.float32) * np.float32(1e-6) * np.repeat(mag, TILE)[:, None]
        g[:, ::7] *= np.float32(1e-3)
    if T > 1:
        g[TILE * zero_tile:TILE * (zero_tile + 1)] = 0.0
    if recipe == "range":
        assert T >= 2 and zero_tile > 2
        tops = [np.float32(2.0 ** -18), np.nextafter(np.float32(2.0 ** -21), np.float32(0.0)), np.float32(1.5 * 2.0 ** -19)][:T]
        for t, top in enumerate(tops):
            blk = g[TILE * t:TILE * (t + 1), :n]
            blk *= np.float32(0.4) * top / np.abs(blk).max()
            blk[3, 1] = -top
        ts = len(tops) - 1 if T >= 3 else 0                                   # (two tiles: the small elements share the power-of-two tile)
        for i, k in enumerate((15, 17, 24, 30)):
            g[TILE * ts + 10 + i, 4:n:5] = tops[ts] * np.float32(2.0 ** -k)
    g[:, n:] = np.nan
    return g, np.abs(g[:, :n]).reshape(T, -1).max(1).view(np.uint32).view(np.int32)


def make_single(recipe, M, n_prev, n_red, zero_tile=5, seed=0):
    """One kernel's operands on their own: g [M, 256] and its tile maxima (`make_g`, n = n_red), the forward weight w [256, 256], the stored sines
    of the layer below [M, 256] (x0 in the tail where n_prev < 256) and x0 [M, 16]."""
    rng = np.random.default_rng(9000 + M + n_prev + 3 * n_red + seed)
    g, tmax = make_g(recipe, M, n_red, zero_tile, seed)
    x0 = np.zeros((M, 16), dtype=np.float32)
    if recipe == "coherent":
        x0[:, :15] = _coherent(rng, (M, 15))
        s_prev, w = _coherent(rng, (M, 256), -1, odd=True), _coherent(rng, (256, 256), -5)
    else:
        x0[:, :15] = rng.standard_normal((M, 15), dtype=np.float32)
        x0[:, 0] = rng.integers(0, 512, M).astype(np.float32)
        s_prev = pack_sines(rng.standard_normal((M, 256)) * 3.0)
        w = ((rng.random((256, 256), dtype=np.float32) * 2 - 1) / 16).astype(np.float32)
    if n_prev < 256:
        s_prev[:, n_prev:] = x0[:, :256 - n_prev]
    return {"g": g, "tmax": tmax, "w": w, "s_prev": s_prev, "x0": x0}


# ---------------------------------------------------------------------------------------------------------------- comparisons
def ratio(got, ref, bound):
    """max over all elements of |got - ref| / bound; an element that is not finite counts as infinitely wrong."""
    r = (got.double() - ref).abs() / bound
    return float(torch.where(torch.isfinite(got.double()), r, torch.full_like(r, float("inf"))).max())


def tmax_ratio(got_bits, ref_g, bound_g, n):
    """The tile maxima against the reference's: the largest of a tile moves by at most the largest bound of the tile."""
    T = got_bits.numel()
    got = got_bits.contiguous().view(torch.float32).double()
    ref = ref_g[:, :n].abs().reshape(T, -1).amax(1)
    return ratio(got, ref, bound_g[:, :n].reshape(T, -1).amax(1))


def check_sequence(inp, out, case, zero_tile):
    """Every kernel of one backward sequence judged on its own, from the inputs it actually received (the g and tile maxima the kernel before it
    wrote).  inp: `make_inputs` as torch tensors; out: g1..g3 [M, 256], tmax1..tmax3, d_w_out, d_b_out, d_b0..d_b3, d_w0..d_w3, all on one device.
    Returns ({kernel.output: max err / bound}, {l: (fp64 weight gradient, its bound or None)}); asserts what is exact (tile maxima as bits of what
    was stored, the zero tile)."""
    ns, L = SHAPES[case], 4
    M = inp["d_x"].shape[0]
    s, w = inp["sines"], inp["weights"]
    res, wref = {}, {}
    ref, bnd = out_layer(inp["d_x"], s[L - 1], inp["w_out"], J_OUT, ns[L - 1])
    for got, key in ((out["g3"][:, :ns[3]], "g"), (out["d_w_out"], "d_w"), (out["d_b_out"], "d_b"), (out["d_b3"], "d_b_prev")):
        res["out." + key] = ratio(got, ref[key], bnd[key])
    res["out.tmax"] = tmax_ratio(out["tmax3"], ref["g"], bnd["g"], ns[3])
    for l in range(L - 1, 0, -1):
        g, tm = out[f"g{l}"], out[f"tmax{l}"]
        assert torch.equal(tm, tile_max_bits(g, ns[l])), f"tmax{l} is not the largest |g{l}| the kernel stored"
        if M > TILE:
            assert float(g[TILE * zero_tile:TILE * (zero_tile + 1), :ns[l]].abs().max()) == 0.0 and int(tm[zero_tile]) == 0, f"zero tile of g{l}"
        wref[l] = (weight_grad(g, s[l - 1], ns[l]), weight_grad_bound(g, tm, s[l - 1], ns[l]) if M <= 256 else None)
        if M <= 256:
            res[f"wgrad{l}.d_w"] = ratio(out[f"d_w{l}"], *wref[l])
        if l > 1:
            ref, bnd = input_grad(g, tm, w[l], s[l - 1], ns[l - 1], ns[l])
            res[f"dgrad{l}.g"] = ratio(out[f"g{l - 1}"][:, :ns[l - 1]], ref["g"], bnd["g"])
            res[f"dgrad{l}.d_b"] = ratio(out[f"d_b{l - 1}"], ref["d_b"], bnd["d_b"])
            res[f"dgrad{l}.tmax"] = tmax_ratio(out[f"tmax{l - 1}"], ref["g"], bnd["g"], ns[l - 1])
        else:
            ref, bnd = first_layer(g, tm, w[1], s[0], inp["x0"], D0, ns[0], ns[1])
            res["first.d_w0"] = ratio(out["d_w0"], ref["d_w0"], bnd["d_w0"])
            res["first.d_b0"] = ratio(out["d_b0"], ref["d_b0"], bnd["d_b0"])
    return res, wref


def emulate_sequence(inp, case):
    """The sequence on the CPU by the emulations (numpy in, torch out, the names `check_sequence` reads); weight gradients where one slab holds all rows."""
    ns = SHAPES[case]
    M = inp["d_x"].shape[0]
    s, w = inp["sines"], inp["weights"]
    out = {}
    g, tm = emulate_out_layer(inp["d_x"], s[3], inp["w_out"], J_OUT, ns[3])
    out["d_w_out"] = (inp["d_x"][:, :J_OUT].T @ s[3]).astype(np.float32)
    out["d_b_out"], out["d_b3"] = inp["d_x"][:, :J_OUT].sum(0, dtype=np.float32), g.sum(0, dtype=np.float32)
    for l in range(3, 0, -1):
        full = np.full((M, 256), np.nan, dtype=np.float32)
        full[:, :ns[l]] = g
        out[f"g{l}"], out[f"tmax{l}"] = full, tm
        out[f"d_w{l}"] = emulate_weight_grad(full, tm, s[l - 1], ns[l]) if M <= 256 else np.zeros((ns[l], 256), dtype=np.float32)
        if l > 1:
            g, out[f"d_b{l - 1}"], tm = emulate_input_grad(full, tm, w[l], s[l - 1], ns[l - 1], ns[l])
        else:
            out["d_w0"], out["d_b0"] = emulate_first_layer(full, tm, w[1], s[0], inp["x0"], D0, ns[0], ns[1])
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}


def to_torch(inp, device="cpu"):
    return {k: [torch.from_numpy(a).to(device) for a in v] if isinstance(v, list) else torch.from_numpy(v).to(device) for k, v in inp.items()}
