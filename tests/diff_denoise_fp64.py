"""fp64 restatement of the differential render's denoiser ("Denoiser for the differential render"), written from
its definition: `prepare`, one `level`, `finish`, the `chain` and the `composite`, in vectorised numpy over whole images, plus the inputs
the two test files share (tests/test_diff_denoise_host.py, tests/test_gpu_diff_denoise.py): `denoise_fp64.random_inputs` extended to two
halves of a differential render, the zero-reach field and the synthetic differential image of the gain test.  The restatement uses no
library code; from denoise_fp64 it takes `lum`, the tap weights and the tap indexing.

A, B: (fg [H,W,3], delta [H,W,3], alpha [H,W]) triples, sums over 1 / scale frames; geom [H,W,8]; alb [H,W,3]; cv [H,W,4]; cov [H,W].
Every array is used at the precision it is given in, converted to float64; `scale` is taken as the float32 the library receives."""
import math

import numpy as np

import denoise_fp64 as dn
from denoise_fp64 import H5, _taps, lum

SHAPES = [(17, 9), (36, 20), (40, 72)]
SCALES = [1.0, 1.0 / 3]


def _f64(x):
    return np.asarray(x, np.float64)


def _scale(scale):
    return float(np.float32(scale))


def coverage(A, B, geom, scale):
    """-> (object layer [H,W] bool, abar, kappa): abar = (0.5 (alphaA + alphaB)) scale, kappa = abar on the object layer (id >= 1), else
    max(0, 1 - abar)."""
    obj = _f64(geom)[..., 7] >= 1
    abar = 0.5 * (_f64(A[2]) + _f64(B[2])) * _scale(scale)
    return obj, abar, np.where(obj, abar, np.maximum(0.0, 1.0 - abar))


def _own(T, obj):
    return np.where(obj[..., None], _f64(T[0]), _f64(T[1]))


def prepare(A, B, geom, scale):
    """-> (cv0 [H,W,4], cov [H,W]).  g = scale / kappa where kappa > 0; c0 = (0.5 (X_A + X_B)) g; vraw = ((lum(X_A) - lum(X_B))^2 / 4) g^2;
    v0 = the [1 2 1] x [1 2 1] average of vraw over the taps inside the image with id_q = id_p and kappa_q > 0, normalised by the weights
    used; where kappa = 0, c0 = v0 = 0."""
    obj, _, kappa = coverage(A, B, geom, scale)
    ids = _f64(geom)[..., 7]
    H, W = ids.shape
    XA, XB = _own(A, obj), _own(B, obj)
    has = kappa > 0
    g = np.where(has, _scale(scale) / np.where(has, kappa, 1.0), 0.0)
    c0 = 0.5 * (XA + XB) * g[..., None]
    vraw = (lum(XA) - lum(XB)) ** 2 * 0.25 * g * g
    num, den = np.zeros((H, W)), np.zeros((H, W))
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            ok, qi, qj = _taps(H, W, di, dj)
            w = (2 - abs(di)) * (2 - abs(dj)) * (ok & (ids[qi, qj] == ids) & has[qi, qj])
            num += w * vraw[qi, qj]
            den += w
    v0 = np.where(has, num / np.where(has, den, 1.0), 0.0)
    return np.concatenate([np.where(has[..., None], c0, 0.0), v0[..., None]], -1), kappa


def level(cv, cov, geom, alb, l, levels=None, sigma_n=32.0, sigma_x=1.0, sigma_a=0.1, sigma_c=4.0):
    """Level l (stride 2^l) -> cv [H,W,4]: the denoiser's level with every tap weight, the centre's 9/64 included, multiplied by kappa_q,
    and |lum(c_p)| in the colour term's relative part; a pixel with kappa_p = 0 gives (0, 0, 0, 0)."""
    cv, cov, geom, alb = _f64(cv), _f64(cov), _f64(geom), _f64(alb)
    H, W = cov.shape
    s = 2 ** l
    c, v = cv[..., :3], cv[..., 3]
    x, rho, n, ids = geom[..., :3], geom[..., 3], geom[..., 4:7], geom[..., 7]
    miss = ids == -1
    lc = lum(c)
    den_c = sigma_c * np.sqrt(np.maximum(v, 0.0)) + 1e-3 * np.abs(lc) + 1e-30
    sw, sc, sv = np.zeros((H, W)), np.zeros((H, W, 3)), np.zeros((H, W))
    for di in range(-2, 3):
        for dj in range(-2, 3):
            ok, qi, qj = _taps(H, W, s * di, s * dj)
            if di == 0 and dj == 0:
                w = np.full((H, W), H5[2] * H5[2])
            else:
                with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                    dot = (n * n[qi, qj]).sum(-1)
                    w_n = np.where(miss, 1.0, np.where(dot > 0, np.maximum(dot, 0.0) ** sigma_n, 0.0))
                    dist = np.abs((n * (x[qi, qj] - x)).sum(-1))
                    w_x = np.where(miss, 1.0, np.exp(-dist / (sigma_x * rho * s * math.sqrt(di * di + dj * dj) + 1e-30)))
                    w_a = np.exp(-((alb - alb[qi, qj]) ** 2).sum(-1) / sigma_a ** 2)
                    w_c = np.exp(-np.abs(lc - lc[qi, qj]) / den_c)
                w = H5[di + 2] * H5[dj + 2] * (ok & (ids[qi, qj] == ids)) * w_n * w_x * w_a * w_c
            w = w * cov[qi, qj] * ok
            sw += w
            sc += w[..., None] * c[qi, qj]
            sv += w * w * v[qi, qj]
    has = cov > 0
    sw1 = np.where(has, sw, 1.0)
    return np.where(has[..., None], np.concatenate([sc / sw1[..., None], (sv / sw1 ** 2)[..., None]], -1), 0.0)


def finish(cv, cov, A, B, geom, scale):
    """-> (fg', delta', alpha'): own = kappa c_L goes to the own layer, the other layer is (0.5 (X_A + X_B)) scale, alpha' = abar."""
    obj, abar, _ = coverage(A, B, geom, scale)
    own = _f64(cov)[..., None] * _f64(cv)[..., :3]
    mean = lambda k: 0.5 * (_f64(A[k]) + _f64(B[k])) * _scale(scale)
    return np.where(obj[..., None], own, mean(0)), np.where(obj[..., None], mean(1), own), abar


def chain(A, B, geom, alb, scale, levels=5, **sigmas):
    cv, cov = prepare(A, B, geom, scale)
    for l in range(levels):
        cv = level(cv, cov, geom, alb, l, **sigmas)
    return finish(cv, cov, A, B, geom, scale)


def composite(fg, delta, alpha, photo, scale=1.0):
    """max(0, (fg + delta) scale + (1 - alpha scale) photo)."""
    return np.maximum(0.0, (_f64(fg) + _f64(delta)) * scale + (1.0 - _f64(alpha) * scale)[..., None] * _f64(photo))


def plain(A, B, scale):
    """The means without the filter: ((0.5 (fgA + fgB)) scale, the same of delta, of alpha)."""
    return tuple(0.5 * (_f64(a) + _f64(b)) * _scale(scale) for a, b in zip(A, B))


def reach(levels):
    """R = 2 (2^L - 1) + 1: the levels' strides summed, plus the variance prefilter's tap."""
    return 2 * (2 ** levels - 1) + 1


# ---- shared inputs -----------------------------------------------------------------------------------------------------------------------
def diff_inputs(H, W, scale, seed=0):
    """`denoise_fp64.random_inputs` as two halves of a differential render summed over n = 1 / scale frames: fg halves are its A and B
    times the frames' coverage, delta halves signed (A and B minus 0.6 of their own mean level, so both signs occur in every id), alpha
    sums n a with a in {0, 1} or uniform in [0.05, 1] on object pixels (id >= 1), 0 on most scene pixels and uniform or 1 on about a
    seventh of them (kappa = 0 on either layer occurs), and a tenth of the pixels with equal halves -> {"A", "B" triples, "geom", "alb",
    "scale"}."""
    x = dn.random_inputs(H, W, seed)
    rng = np.random.default_rng(77 * H + W + seed)
    n = round(1.0 / scale)
    ids = x["geom"][..., 7]
    obj = ids >= 1
    pick = rng.uniform(size=(2, H, W))
    both = rng.uniform(size=(H, W))                      # decides for both halves: no coverage at all, or full coverage
    a = np.where(both < 0.12, 0.0, np.where(pick < 0.1, 0.0, np.where(pick < 0.4, 1.0, rng.uniform(0.05, 1.0, size=(2, H, W)))))
    some = rng.uniform(size=(H, W)) < 0.15
    a = np.where(obj, a, np.where(some, np.where(both < 0.4, 1.0, rng.uniform(0.05, 1.0, size=(2, H, W))), 0.0))
    fg = [x[k] * a[i][..., None] * n for i, k in enumerate("AB")]
    level = 0.6 * np.mean([x["A"], x["B"]])
    delta = [(x[k] - level) * n * 0.5 for k in "AB"]
    same = rng.uniform(size=(H, W)) < 0.1
    for t in (fg, delta):
        t[1][same] = t[0][same]
    al = [a[0] * n, np.where(same, a[0], a[1]) * n]
    f32 = lambda y: np.ascontiguousarray(y, dtype=np.float32)
    return {"A": (f32(fg[0]), f32(delta[0]), f32(al[0])), "B": (f32(fg[1]), f32(delta[1]), f32(al[1])), "geom": x["geom"], "alb": x["alb"],
            "scale": scale}


def reduction_inputs(H, W, seed=0):
    """The reduction to the plain denoiser: `random_inputs` with every id > 0 set to 0 (ids 0 and -1 remain), alphas 0, delta halves its
    A and B (>= 0), fg 0."""
    x = dn.random_inputs(H, W, seed)
    geom = x["geom"].copy()
    geom[..., 7] = np.minimum(geom[..., 7], 0.0)
    z3, z1 = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32)
    return {"A": (z3, x["A"], z1), "B": (z3, x["B"], z1), "geom": geom, "alb": x["alb"], "scale": 1.0}


def block_inputs(H=40, W=72, seed=0):
    """Zero reach: `reduction_inputs`' guides, delta halves non-zero in the 4 x 4 block at rows 18..21, columns 34..37 only (signed), fg
    and alpha 0; and a photograph -> (inputs, block mask, photo)."""
    x = reduction_inputs(H, W, seed)
    block = np.zeros((H, W), bool)
    block[18:22, 34:38] = True
    rng = np.random.default_rng(5 + seed)
    dA, dB = (np.where(block[..., None], rng.normal(0.0, 0.5, (H, W, 3)), 0.0).astype(np.float32) for _ in range(2))
    x["A"], x["B"] = (x["A"][0], dA, x["A"][2]), (x["B"][0], dB, x["B"][2])
    return x, block, rng.gamma(2.0, 0.5, (H, W, 3)).astype(np.float32)


def chebyshev_to(mask):
    """Per pixel, the Chebyshev distance to the nearest pixel of `mask`."""
    H, W = mask.shape
    pi, pj = np.nonzero(mask)
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return np.maximum(np.abs(i[..., None] - pi), np.abs(j[..., None] - pj)).min(-1)


def synthetic_diff(H=64, W=80):
    """`denoise_fp64.synthetic()` as a differential image, the disc the inserted object: coverage clip(10.5 - r, 0, 1) around the disc's
    centre, an elliptical Gaussian shadow beside it, a bounce ring of amplitude 0.15 and width 6 at r = 10; D = albedo (-0.6 shadow
    irradiance + 0.8 bounce) is what an uncovered sample sees change, delta = (1 - alpha) D, fg = alpha truth; the photograph is the truth
    times a fine texture -> the guides plus {"alpha", "fg", "delta", "D", "p_touch", "photo", "truth", "composite"}."""
    s = dn.synthetic(H, W)
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    r = np.sqrt((i - 30) ** 2 + (j - 20) ** 2)
    alpha = np.clip(10.5 - r, 0.0, 1.0)
    shadow = np.exp(-((i - 44) / 6.0) ** 2 - ((j - 30) / 12.0) ** 2)
    bounce = 0.15 * np.exp(-((r - 10.0) / 6.0) ** 2)
    alb = s["alb"].astype(np.float64)
    irr = (s["truth"] / alb)[..., :1]
    D = alb * (-0.6 * shadow[..., None] * irr + 0.8 * bounce[..., None])
    photo = s["truth"] * (1.0 + 0.2 * np.sin(1.7 * i) * np.cos(2.3 * j))[..., None]
    s.update(alpha=alpha, fg=alpha[..., None] * s["truth"], delta=(1 - alpha)[..., None] * D, D=D, p_touch=np.clip(shadow + 2 * bounce, 0.0, 1.0),
             photo=np.ascontiguousarray(photo, dtype=np.float32))
    s["composite"] = composite(s["fg"], s["delta"], alpha, s["photo"])
    return s


def noisy_diff_halves(s, spp, rng):
    """Two halves of spp / 2 samples each, built as `noisy_halves` builds them (a mean over the samples): a sample is covered with
    probability alpha and then adds truth times a Gamma(0.5, 2) variate to fg and 1 to alpha; otherwise it is touched with probability
    p_touch and then adds D / p_touch times such a variate to delta (so the mean of delta is (1 - alpha) D) -> (A, B) fp32 triples."""
    def half():
        shp = (spp // 2,) + s["alpha"].shape
        covered = rng.uniform(size=shp) < s["alpha"]
        touched = ~covered & (rng.uniform(size=shp) < s["p_touch"])
        gam = rng.gamma(shape=0.5, scale=2.0, size=shp + (1,))
        fg = (covered[..., None] * s["truth"][None] * gam).mean(0)
        delta = (touched[..., None] * (s["D"] / s["p_touch"][..., None])[None] * gam).mean(0)
        return fg.astype(np.float32), delta.astype(np.float32), covered.mean(0).astype(np.float32)

    return half(), half()


# ---- checks both test files apply: every `lib_*` argument is the library's function of that name, on the CPU or on the device ------------
def u32(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.float32).view(np.uint32)


def check_steps_against_fp64(x, lib_prepare, lib_level, lib_finish, lib_chain, what, report):
    """Prepare, each of five levels (each on the library's own prepare output) and finish against the restatement at every pixel: colours
    within 1e-4 of the largest |c0|, variances within 1e-4 of the largest v0, the existing denoiser's criterion; the chain's three outputs
    to the same criterion; nothing non-finite.  -> the worst colour error."""
    A, B, geom, alb, scale = x["A"], x["B"], x["geom"], x["alb"], x["scale"]
    ref_cv, ref_cov = prepare(A, B, geom, scale)
    cv, cov = (np.asarray(t, np.float64) for t in lib_prepare(A, B, geom, scale))
    c_in, v_in = float(np.abs(ref_cv[..., :3]).max()), float(ref_cv[..., 3].max())
    assert np.array_equal(cov > 0, ref_cov > 0) and float(np.abs(cov - ref_cov).max()) <= 1e-6
    ec, ev = float(np.abs(cv[..., :3] - ref_cv[..., :3]).max()) / c_in, float(np.abs(cv[..., 3] - ref_cv[..., 3]).max()) / v_in
    report(f"{what} prepare: worst colour / variance error relative to the largest c0 / v0", (ec, ev))
    assert ec <= 1e-4 and ev <= 1e-4
    worst = ec
    cv32, cov32 = cv.astype(np.float32), cov.astype(np.float32)
    for l in range(5):
        got = np.asarray(lib_level(cv32, cov32, geom, alb, l), np.float64)
        ref = level(cv32, cov32, geom, alb, l)
        assert np.isfinite(got).all() and not got[cov32 == 0].any()
        ec, ev = float(np.abs(got[..., :3] - ref[..., :3]).max()) / c_in, float(np.abs(got[..., 3] - ref[..., 3]).max()) / v_in
        report(f"{what} level {l}: worst colour / variance error relative to the largest c0 / v0", (ec, ev))
        assert ec <= 1e-4 and ev <= 1e-4, (l, ec, ev)
        worst = max(worst, ec)
        last = got
    last32 = last.astype(np.float32)
    got, ref = lib_finish(last32, cov32, A, B, geom, scale), finish(last32, cov32, A, B, geom, scale)
    ef = max(float(np.abs(np.asarray(g, np.float64) - r).max()) for g, r in zip(got, ref)) / c_in
    report(f"{what} finish: worst error of fg', delta', alpha' relative to the largest c0", ef)
    assert ef <= 1e-4
    got, ref = lib_chain(A, B, alb, geom, scale), chain(A, B, geom, alb, scale)
    assert all(np.isfinite(np.asarray(g)).all() for g in got)
    ech = max(float(np.abs(np.asarray(g, np.float64) - r).max()) for g, r in zip(got, ref)) / c_in
    report(f"{what} chain, L = 5: worst error of fg', delta', alpha' relative to the largest c0", ech)
    assert ech <= 1e-4
    return max(worst, ef, ech)


def check_field(x):
    """The field shows what it is for: ids -1..2, both signs of delta, no coverage on either layer, scene pixels with alpha > 0, partial
    coverage, equal halves."""
    ids = x["geom"][..., 7]
    obj, abar, kappa = coverage(x["A"], x["B"], x["geom"], x["scale"])
    assert set(np.unique(ids)) == {-1.0, 0.0, 1.0, 2.0}
    assert (x["A"][1] < 0).any() and (x["A"][1] > 0).any()
    assert (obj & (kappa == 0)).any() and (~obj & (abar > 0)).any() and ((kappa > 0) & (kappa < 1)).any()
    assert (np.abs(x["A"][1] - x["B"][1]).max(-1) == 0).any()
    return obj, abar, kappa


def check_sign_symmetry(x, lib_chain):
    fg, delta, alpha = (np.asarray(t) for t in lib_chain(x["A"], x["B"], x["alb"], x["geom"], x["scale"]))
    neg = lambda T: (T[0], -T[1], T[2])
    fg2, delta2, alpha2 = (np.asarray(t) for t in lib_chain(neg(x["A"]), neg(x["B"]), x["alb"], x["geom"], x["scale"]))
    assert np.array_equal(u32(fg), u32(fg2)) and np.array_equal(u32(alpha), u32(alpha2))
    assert np.array_equal(delta2, -delta) and (delta != 0).mean() > 0.8
    nz = delta != 0                                                   # a pixel without coverage is +0 either way
    assert np.array_equal(u32(delta2)[nz], u32(-delta)[nz])


def check_scaling(x, lib_chain, k):
    f = np.float32(2.0 ** k)
    one = [np.asarray(t) for t in lib_chain(x["A"], x["B"], x["alb"], x["geom"], x["scale"])]
    mul = lambda T: (T[0] * f, T[1] * f, T[2])
    scaled = [np.asarray(t) for t in lib_chain(mul(x["A"]), mul(x["B"]), x["alb"], x["geom"], x["scale"])]
    assert np.array_equal(u32(one[0] * f), u32(scaled[0])) and np.array_equal(u32(one[1] * f), u32(scaled[1]))
    assert np.array_equal(u32(one[2]), u32(scaled[2]))


def check_pass_through(x, lib_chain):
    """The other layer and alpha: (0.5 (X_A + X_B)) scale in fp32, bit for bit; and they differ from the filtered own layer."""
    fg, delta, alpha = (np.asarray(t) for t in lib_chain(x["A"], x["B"], x["alb"], x["geom"], x["scale"]))
    sc = np.float32(x["scale"])
    mean = lambda k: (np.float32(0.5) * (x["A"][k] + x["B"][k])) * sc
    obj = x["geom"][..., 7] >= 1
    assert np.array_equal(u32(alpha), u32(mean(2)))
    assert np.array_equal(u32(fg)[~obj], u32(mean(0))[~obj]) and np.array_equal(u32(delta)[obj], u32(mean(1))[obj])
    assert (fg[obj] != mean(0)[obj]).any() and (delta[~obj] != mean(1)[~obj]).any()


def check_zero_reach(lib_chain, lib_composite, report, what):
    """40 x 72, L = 2, delta halves non-zero in a 4 x 4 block only: every pixel farther than R = 7 has delta' = +0 and the composite
    returns the photograph's bits there; at least one pixel inside R, outside the block, is non-zero."""
    x, block, photo = block_inputs()
    assert reach(2) == 7
    fg, delta, alpha = (np.asarray(t) for t in lib_chain(x["A"], x["B"], x["alb"], x["geom"], 1.0, levels=2))
    dist = chebyshev_to(block)
    far = dist > 7
    assert far.sum() > 1000 and not u32(delta)[far].any() and not u32(fg).any() and not u32(alpha).any()
    out = np.asarray(lib_composite(fg, delta, alpha, photo, 1.0))
    assert np.array_equal(u32(out)[far], u32(photo)[far])
    spread = (delta != 0).any(-1) & ~block
    assert spread.any() and dist[spread].max() <= 7
    report(f"{what} zero reach, L = 2: pixels beyond R = 7 (all +0); non-zero pixels outside the block; their largest distance",
           (int(far.sum()), int(spread.sum()), int(dist[spread].max())))


def check_convexity(x, lib_chain, report, what):
    """own / kappa stays, per channel, inside the [min, max] of the unpremultiplied mean c0 over the pixels of its own id that have
    coverage and that its footprint reaches (1e-6 of the largest |c0| for rounding)."""
    fg, delta, alpha = (np.asarray(t, np.float64) for t in lib_chain(x["A"], x["B"], x["alb"], x["geom"], x["scale"]))
    c0, kappa = prepare(x["A"], x["B"], x["geom"], x["scale"])
    obj = x["geom"][..., 7] >= 1
    has = kappa > 0
    own = np.where(obj[..., None], fg, delta) / np.where(has, kappa, 1.0)[..., None]
    groups = np.where(has, x["geom"][..., 7], -100.0)                  # pixels without coverage: a group of their own, all zero
    worst = dn.convex_hull_violation(own, c0[..., :3], groups)
    report(f"{what} convex hull of own / kappa per id: worst excess relative to the largest c0", worst)
    assert worst <= 1e-6
    assert float(np.abs(own - c0[..., :3]).max()) > 0.05 * float(np.abs(c0[..., :3]).max())      # and it did filter


def gain_cases():
    """(spp, seed, A, B, the restatement's ratio) for spp 8, 32, 128 x seeds 0..2 on the synthetic differential image: rel_rmse of the plain
    mean's composite over that of the restatement's composite, both against the true composite."""
    s = synthetic_diff()
    out = []
    for spp in (8, 32, 128):
        for seed in range(3):
            A, B = noisy_diff_halves(s, spp, np.random.default_rng(1000 * spp + seed))
            mean = dn.rel_rmse(composite(*plain(A, B, 1.0), s["photo"]), s["composite"])
            den = dn.rel_rmse(composite(*chain(A, B, s["geom"], s["alb"], 1.0), s["photo"]), s["composite"])
            out.append((spp, seed, A, B, mean, mean / den))
    return s, out


def check_gain(lib_chain, report, what):
    """The restatement beats the plain mean by more than 1.5 in every case, and `lib_chain` reaches at least 0.9 of the restatement's ratio."""
    s, cases = gain_cases()
    for spp, seed, A, B, plain, ratio64 in cases:
        got = lib_chain(A, B, s["alb"], s["geom"], 1.0)
        ratio = plain / dn.rel_rmse(composite(*(np.asarray(t, np.float64) for t in got), s["photo"]), s["composite"])
        report(f"{what} synthetic differential 64x80 spp {spp} seed {seed}: rel RMSE plain, ratio of the restatement, ratio of the library",
               (plain, ratio64, ratio))
        assert ratio64 > 1.5, (spp, seed, ratio64)
        assert ratio >= 0.9 * ratio64, (spp, seed, ratio, ratio64)
