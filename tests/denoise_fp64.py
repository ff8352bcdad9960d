"""fp64 restatement of the denoiser ("Denoiser"), written from its definition: `prepare`, one a-trous `level`
and the `chain`, in vectorised numpy over whole images, plus the inputs the denoiser tests share (tests/test_denoise_host.py,
tests/test_gpu_denoise.py): random fields, the synthetic image of the gain test, the two feature scenes and the checks both files
apply.  The restatement itself uses no library code.

Inputs: A, B [H,W,3] two half renders; geom [H,W,8] = (p, rho) and (n, id) per pixel; alb [H,W,3]; cv [H,W,4] = (colour, variance of
its luminance).  Every array is used at the precision it is given in, converted to float64."""
import math

import numpy as np

LUM = np.array([0.2126, 0.7152, 0.0722])
H5 = np.array([1.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 4, 1.0 / 16])
DEFAULTS = {"levels": 5, "sigma_n": 32.0, "sigma_x": 1.0, "sigma_a": 0.1, "sigma_c": 4.0}
FOV = 35.0


def lum(c):
    return np.asarray(c, np.float64) @ LUM


def _taps(H, W, di, dj):
    """Tap (i + di, j + dj) of every pixel: (inside the image [H,W] bool, its row and column clipped to the image)."""
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    qi, qj = i + di, j + dj
    return (qi >= 0) & (qi < H) & (qj >= 0) & (qj < W), np.clip(qi, 0, H - 1), np.clip(qj, 0, W - 1)


def prepare(A, B, geom):
    """c0 = (A + B) / 2; v0 = the [1 2 1] x [1 2 1] average of (lum(A) - lum(B))^2 / 4 over the taps inside the image that carry the
    pixel's id, normalised by the weights used -> cv0 [H,W,4]."""
    A, B, geom = (np.asarray(x, np.float64) for x in (A, B, geom))
    H, W = A.shape[:2]
    ids = geom[..., 7]
    vraw = (lum(A) - lum(B)) ** 2 / 4.0
    num, den = np.zeros((H, W)), np.zeros((H, W))
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            ok, qi, qj = _taps(H, W, di, dj)
            w = (2 - abs(di)) * (2 - abs(dj)) * (ok & (ids[qi, qj] == ids))
            num += w * vraw[qi, qj]
            den += w
    return np.concatenate([(A + B) / 2.0, (num / den)[..., None]], -1)


def level(cv, geom, alb, l, levels=None, sigma_n=32.0, sigma_x=1.0, sigma_a=0.1, sigma_c=4.0):
    """Level l (stride 2^l) -> cv [H,W,4]; `levels` is not used by one level."""
    cv, geom, alb = (np.asarray(x, np.float64) for x in (cv, geom, alb))
    H, W = cv.shape[:2]
    s = 2 ** l
    c, v = cv[..., :3], cv[..., 3]
    x, rho, n, ids = geom[..., :3], geom[..., 3], geom[..., 4:7], geom[..., 7]
    miss = ids == -1
    lc = lum(c)
    den_c = sigma_c * np.sqrt(np.maximum(v, 0.0)) + 1e-3 * lc + 1e-30
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
            sw += w
            sc += w[..., None] * c[qi, qj]
            sv += w * w * v[qi, qj]
    return np.concatenate([sc / sw[..., None], (sv / sw ** 2)[..., None]], -1)


def chain(A, B, geom, alb, levels=5, **sigmas):
    """prepare, then `levels` levels -> the denoised colour [H,W,3]."""
    cv = prepare(A, B, geom)
    for l in range(levels):
        cv = level(cv, geom, alb, l, **sigmas)
    return cv[..., :3]


# ---- shared inputs -----------------------------------------------------------------------------------------------------------------------
SHAPES = [(17, 9), (36, 20), (24, 24), (40, 72)]     # (H, W); at 40 x 72 some pixels have all 25 taps inside the image up to stride 8


def pixel_dirs(H, W, fov=FOV):
    """Unit directions of the rays through the pixel centres, the render's camera: [H,W,3]."""
    f = (W / 2.0) / math.tan(math.radians(fov) / 2.0)
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.stack([(j - (W - 1) / 2.0) / f, -(i - (H - 1) / 2.0) / f, -np.ones_like(i)], -1)
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


def random_inputs(H, W, seed=0):
    """Random fp32 inputs of one step: ids in {-1, 0, 1, 2} in blobs and speckles, random unit normals (each id's own direction,
    perturbed), positions of order 1 (a slab per id along the camera rays, roughened by a few footprints), colours in [0, 1.5],
    variances with exact zeros, a two-level albedo with noise -> {"A", "B", "geom", "alb", "cv"}; cv is what a level takes
    (colours, variances), independent of A and B."""
    rng = np.random.default_rng(1000 * H + W + seed)
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ids = np.zeros((H, W))
    ids[(i - 0.3 * H) ** 2 + (j - 0.6 * W) ** 2 < (0.25 * min(H, W)) ** 2] = 1
    ids[(i > 0.6 * H) & (j < 0.5 * W)] = 2
    ids[i + j < 0.25 * min(H, W)] = -1
    speck = rng.uniform(size=(H, W)) < 0.08
    ids[speck] = rng.integers(-1, 3, size=(H, W))[speck]
    base = np.array([[0.0, 0.0, 1.0], [0.3, 0.1, 0.9], [-0.2, 0.4, 0.8], [0.1, -0.3, 0.9]])[(ids + 1).astype(int)]
    n = base + 0.15 * rng.normal(size=(H, W, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    scale = 2.0 * math.tan(math.radians(FOV) / 2.0) / W
    depth = 1.0 + 0.4 * ids + 0.3 * j / W
    p = pixel_dirs(H, W) * (depth * (1.0 + 1.5 * scale * rng.normal(size=(H, W))))[..., None]
    rho = np.linalg.norm(p, axis=-1) * scale
    miss = ids == -1
    p[miss], n[miss], rho[miss] = 0.0, 0.0, 0.0
    geom = np.concatenate([p, rho[..., None], n, ids[..., None]], -1).astype(np.float32)
    alb = np.where(((i // 5 + j // 7) % 2 == 0)[..., None], [0.8, 0.3, 0.2], [0.2, 0.5, 0.7]) + 0.03 * rng.normal(size=(H, W, 3))
    smooth = 0.5 + 0.3 * np.sin(i / 5.0)[..., None] + 0.2 * np.cos(j / 7.0)[..., None]
    col = np.clip(alb * smooth + 0.08 * rng.normal(size=(H, W, 3)), 0.0, 1.5)
    var = rng.gamma(1.0, 0.01, size=(H, W))
    var[rng.uniform(size=(H, W)) < 0.2] = 0.0
    A = np.clip(col + 0.1 * rng.normal(size=(H, W, 3)), 0.0, None)
    B = np.clip(col + 0.1 * rng.normal(size=(H, W, 3)), 0.0, None)
    same = rng.uniform(size=(H, W)) < 0.1              # pixels where both halves agree: exact zeros of the raw variance
    B[same] = A[same]
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return {"A": f32(A), "B": f32(B), "geom": geom, "alb": f32(alb), "cv": f32(np.concatenate([col, var[..., None]], -1))}


def synthetic(H=64, W=80):
    """The deterministic image of the gain test: a plane tilted in x with a 0.5 depth step at column 40 (id 0), a disc of radius 10 at
    row 30, column 20 (id 1, hemisphere normals, distance 1.5); an 8-pixel two-colour checker, 0.8 on the disc; truth = albedo x (a
    smooth shading of the normals + a slow sinusoid in x) -> {"geom" fp32, "alb" fp32, "truth" fp64}."""
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    fov = math.radians(FOV)
    f = (W / 2) / math.tan(fov / 2)
    dirs = np.stack([(j - (W - 1) / 2) / f, -(i - (H - 1) / 2) / f, -np.ones_like(i, float)], -1)
    z = 2.0 + 0.3 * (j / W) + np.where(j >= 40, 0.5, 0.0)
    pos = dirs * z[..., None]
    nrm = np.zeros((H, W, 3))
    nrm[..., 2], nrm[..., 0] = 1.0, -0.3
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    ids = np.zeros((H, W))
    disc = (i - 30) ** 2 + (j - 20) ** 2 < 100
    ids[disc] = 1
    nd = np.stack([(j - 20) / 12.0, -(i - 30) / 12.0, np.sqrt(np.clip(1 - ((j - 20) ** 2 + (i - 30) ** 2) / 144.0, 0, 1))], -1)
    nrm[disc] = nd[disc] / np.linalg.norm(nd[disc], axis=-1, keepdims=True)
    pos[disc] = dirs[disc] * 1.5
    alb = np.where((((i // 8) + (j // 8)) % 2 == 0)[..., None], np.array([0.8, 0.3, 0.2]), np.array([0.2, 0.5, 0.7]))
    alb[disc] = 0.8
    shade = 0.3 + 0.7 * np.clip(nrm @ np.array([0.3, 0.5, 0.8]), 0, 1) + 0.2 * np.sin(j / 9.0)
    rho = np.linalg.norm(pos, axis=-1) * 2 * math.tan(fov / 2) / W
    geom = np.concatenate([pos, rho[..., None], nrm, ids[..., None]], -1).astype(np.float32)
    return {"geom": np.ascontiguousarray(geom), "alb": np.ascontiguousarray(alb, dtype=np.float32), "truth": alb * shade[..., None]}


def noisy_halves(truth, spp, rng):
    """Two half buffers of spp/2 samples each: every sample is truth times a Gamma(0.5, 2) variate (mean 1) -> (A, B) fp32."""
    half = lambda: (truth[None] * rng.gamma(shape=0.5, scale=2.0, size=(spp // 2,) + truth.shape[:2] + (1,))).mean(0).astype(np.float32)
    return half(), half()


def rel_rmse(x, truth):
    return float(np.sqrt(np.mean((np.asarray(x, np.float64) - truth) ** 2) / np.mean(truth ** 2)))


# ---- checks and scenes both test files use ------------------------------------------------------------------------------------------------
def convex_hull_violation(out, mean, ids, levels=5):
    """How far `out` leaves, per channel, the [min, max] of `mean` over the pixels of its own id that its footprint can reach (the
    sum of the levels' reaches, 2 (2^levels - 1), in both axes), relative to the largest |mean|."""
    H, W = ids.shape
    reach = 2 * (2 ** levels - 1)
    worst = 0.0
    for i in range(H):
        for j in range(W):
            i0, i1, j0, j1 = max(0, i - reach), min(H, i + reach + 1), max(0, j - reach), min(W, j + reach + 1)
            sel = mean[i0:i1, j0:j1][ids[i0:i1, j0:j1] == ids[i, j]]
            worst = max(worst, float((sel.min(0) - out[i, j]).max()), float((out[i, j] - sel.max(0)).max()))
    return worst / float(np.abs(mean).max())


def feature_scenes(pathtrace, H, W):
    """(name, V, T, n_scene, table, corner normals, normal map): the groove under `table_scene`'s objects, and the groove under a
    tilted normal map."""
    from materialist_amd import mesh
    from path_fp64 import groove_scene
    from path_normal_fp64 import tilted_normals
    from path_oi_smooth_fp64 import table_scene

    rm = mesh.reference_mesh(groove_scene(H, W), FOV)
    n_scene = rm["triangles"].shape[0]
    V, T, table, corner = pathtrace.merge_objects(rm["vertices"], rm["triangles"], table_scene(), normals=True)
    yield "table", V, T, n_scene, table, corner, None
    yield "groove+map", rm["vertices"], rm["triangles"], n_scene, [], None, tilted_normals(rm, H, W)[0]


def check_features(got, ref, what, report):
    """id exact in every pixel, p within 1e-5 (1 + |p|), n within 1e-5, rho within 1e-6 relative."""
    got = got.astype(np.float64)
    assert np.array_equal(got[..., 7], ref[..., 7]), what
    ep = float((np.abs(got[..., :3] - ref[..., :3]).max(-1) / (1 + np.linalg.norm(ref[..., :3], axis=-1))).max())
    en = float(np.abs(got[..., 4:7] - ref[..., 4:7]).max())
    er = float((np.abs(got[..., 3] - ref[..., 3]) / np.where(ref[..., 3] > 0, ref[..., 3], 1.0)).max())
    report(f"features {what}: worst p error / (1 + |p|), n error, relative rho error", (ep, en, er))
    assert ep <= 1e-5 and en <= 1e-5 and er <= 1e-6, (what, ep, en, er)
