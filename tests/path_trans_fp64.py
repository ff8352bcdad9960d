"""fp64 restatement of the path render under transparency editing ("Transparency editing"): the reference's
TransBSDF (myutils/mi_plugin.py:1477-1771) written out in numpy from its own lines, and `path_fp64.replay` walking with it.

`refracted_texel` is calculate_refracted_screen_coor (:1494-1519), `eval_trans` is eval_brdf (:1618-1724), `sample_trans` is
sample_brdf (:1567-1616).  `replay_trans` walks one sample of every pixel as `path_fp64.replay` does and records, per pixel, whether
some vertex read a masked texel (`masked_vertex`) and whether a BSDF sample left below the surface at a masked vertex (`below`).

No BVH and no library code; `closest` / `occluded` may be bound to the library's fp32 traversal to tell the paths whose hit
decisions differ between fp32 and fp64."""
import math

import numpy as np

from path_fp64 import FOV, brute, env_texel, mis, pcg, rng_u, texel  # noqa: F401  (pcg: the restated RNG, for callers)


def _dot(a, b):
    return (a * b).sum(-1)


def refract(w, n, eta):
    """calculate_refraction (:1494-1501)."""
    c = _dot(w, n)
    s2 = np.maximum(0.0, 1.0 - c * c)
    ct = np.sqrt(np.maximum(0.0, 1.0 - eta * eta * s2))
    v = eta * (n * c[:, None] - w) - n * ct[:, None]
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def refracted_point(p, n, wo, ior, dist):
    """The point whose texel the background is read at (:1503-1519, called with 1/ior, which it inverts back to ior): 0.3 D along
    the first refraction, then D along the second, which assumes the first normal again."""
    d1 = refract(wo, n, ior)
    p1 = p + 0.3 * dist * d1
    d2 = refract(-d1, n, 1.0 / ior)
    return p1 + dist * d2


def refracted_texel(o64, p, n, wo, ior, dist, H, W):
    """-> the flat texel of `refracted_point` by the render's own lookup (floor, clamp to the image)."""
    return texel(o64, refracted_point(p, n, wo, ior, dist), H, W)


def d_ggx(cos_h, r):
    alpha2 = r ** 4
    den = (cos_h * cos_h * (alpha2 - 1.0) + 1.0) + 1e-6
    return alpha2 / (math.pi * den * den)


def g_smith(nov, nol, r):
    k = (r + 1.0) ** 2 / 8.0
    return 1.0 / (nol * (1 - k) + k + 1e-6) / (nov * (1 - k) + k + 1e-6)


def eval_trans(o64, wi, wo, n, a, r, m, bg, masked, ior, T):
    """eval_brdf (:1618-1724): wi to the light, wo to the viewer, n the normal, a [N,3] r [N] m [N] the hit texel's maps, bg [N,3] the
    background at the refracted texel, masked [N] bool -> (f [N,3] with its cosine, pdf [N])."""
    wi, wo, n, a, bg = (np.asarray(x, np.float64) for x in (wi, wo, n, a, bg))
    r, m = np.asarray(r, np.float64).reshape(-1), np.asarray(m, np.float64).reshape(-1)
    masked = np.asarray(masked, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        h = wi + wo
        h = h / np.linalg.norm(h, axis=-1, keepdims=True)
        NoL, NoV = np.maximum(_dot(n, wi), 0), np.maximum(_dot(n, wo), 0)
        VoH, NoH = np.maximum(_dot(wo, h), 0), np.maximum(_dot(n, h), 0)
        D = d_ggx(NoH, r)
        pdf = 0.5 * (D / (4 * np.maximum(VoH, 1e-4)) * NoH) + 0.5 * (NoL / math.pi)
        ori, _ = o64.eval_brdf(wi, wo, n, a, r, m)                       # brdf_ori: MatDiffBSDF's Disney form
        G = g_smith(NoV, NoL, r)
        m1 = (1 - m)[:, None]
        kd = a * m1 * (1 - T)
        glass_col = m1 * (bg * T)
        C0 = m1 * 0.04 + m[:, None] * a
        F_m = C0 + (1 - C0) * ((1 - VoH) ** 5)[:, None]
        diff = kd / math.pi * NoL[:, None]
        metal = (D * G)[:, None] * F_m / 4.0 * NoL[:, None]
        LoH = np.maximum(_dot(wi, h), 0)
        hw_in, hw_out = 1 / (LoH + 1e-6), 1 / (VoH + 1e-6)
        nw_in, nw_out = 1 / (NoL + 1e-6), 1 / (NoV + 1e-6)
        R_s = (hw_in - ior * hw_out) / (hw_in + ior * hw_out)
        R_p = (ior * hw_in - hw_out) / (ior * hw_in + hw_out)
        F_glass = 0.5 * (R_s ** 2 + R_p ** 2)
        D_hack = d_ggx(NoH, np.ones_like(r))
        btdf = np.sqrt(glass_col) * (G * D_hack * (1 - F_glass) * (ior ** 2 * hw_in * hw_out) / (nw_in * nw_out * (ior * hw_in + hw_out) ** 2))[:, None]
        spec_edit = glass_col * (D * G / (4 * nw_in))[:, None]
        f_glass = np.where((NoL * NoV > 0)[:, None], spec_edit, btdf)
        edit = diff + metal + f_glass
        f = np.where(masked[:, None], edit, ori)
        f = np.where(f > 0, f, 0.0)
        pdf = np.where(pdf > 0, pdf, 0.0)
    return f, pdf


def sample_trans(o64, sample1, sample2, wo, n, a, r, m, bg, masked, ior, T):
    """sample_brdf (:1567-1616): MatDiffBSDF's directions (sample1 > 0.5: diffuse, else GGX with the texel's roughness), the value
    and pdf there, weight f / (pdf + 1e-4) where pdf > 0 -> (wi, pdf, weight)."""
    wi, _, _ = o64.sample_brdf(sample1, sample2, wo, n, a, r, m)
    f, pdf = eval_trans(o64, wi, wo, n, a, r, m, bg, masked, ior, T)
    w = np.where((pdf > 0)[:, None], f / (pdf + 1e-4)[:, None], 0.0)
    return wi, pdf, w


def replay_trans(o64, V, T, a, r, m, env, tab, H, W, max_depth, seed, mask, bg, ior=1.2, spec_trans=0.4, refract_distance=100.0, sample=0,
                 closest=None, occluded=None):
    """Sample `sample` of every pixel, fp64 -> (L [H,W,3], record).  V: the mesh's vertices rounded to fp32 as the BVH stores them;
    mask [H,W] bool, bg [H,W,3].  The record: `masked_vertex` [H*W] (some vertex of the pixel's path read a masked texel), `below`
    [H*W] (a BSDF sample left below the surface at a masked vertex), `vertices` (per depth: pix, tp, tq, masked, wo, n, wi, ...)."""
    He, We = env.shape[:2]
    envf = env.reshape(-1, 3).astype(np.float64)
    pdf_tab = tab["pdf"].reshape(-1).astype(np.float64)
    row_cdf, col_cdf = tab["row_cdf"], tab["col_cdf"]
    have_tab = tab["row_cdf"][-1] > 0
    P = V[T]
    if closest is None:
        closest = lambda o, d: brute(P, o, d)
    if occluded is None:
        occluded = lambda o, d: np.isfinite(brute(P, o, d)[0])
    nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    nrm *= np.where((nrm * P[:, 0]).sum(-1, keepdims=True) > 0, -1.0, 1.0)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=-1, keepdims=True), 1e-300)
    pix = np.arange(H * W, dtype=np.uint32)
    N = pix.size
    base = pcg(pcg(pcg(np.uint32(seed)) + pix) + np.uint32(sample))
    ii, jj = pix // W, pix % W
    f = (W / 2.0) / math.tan(math.radians(FOV) / 2.0)
    x = jj - 0.5 + rng_u(base, 0, 0)
    y = ii - 0.5 + rng_u(base, 0, 1)
    d = np.stack([(x - (W - 1) / 2) / f, -(y - (H - 1) / 2) / f, -np.ones(N)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.zeros((N, 3))
    L, thr, prev = np.zeros((N, 3)), np.ones((N, 3)), np.zeros(N)
    alive = np.ones(N, bool)
    A, R, M = a.reshape(-1, 3).astype(np.float64), r.reshape(-1).astype(np.float64), m.reshape(-1).astype(np.float64)
    MK, BG = np.asarray(mask).reshape(-1) != 0, np.asarray(bg).reshape(-1, 3).astype(np.float64)
    rec = {"H": H, "W": W, "He": He, "We": We, "pixels": pix.astype(np.int64), "full": True, "escapes": [], "vertices": [],
           "masked_vertex": np.zeros(N, bool), "below": np.zeros(N, bool)}
    for depth in range(max_depth + 1):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        t, k = closest(o[idx], d[idx])
        miss = k < 0
        im = idx[miss]
        if im.size:
            tx = env_texel(d[im], He, We)
            w = np.ones(im.size) if depth == 0 else mis(prev[im], pdf_tab[tx] if have_tab else 0.0)
            L[im] += thr[im] * envf[tx] * w[:, None]
            rec["escapes"].append({"depth": depth, "pix": im, "tx": tx, "w": w})
        alive[im] = False
        if depth + 1 >= max_depth:
            alive[:] = False
            break
        idx, t, k = idx[~miss], t[~miss], k[~miss]
        n = nrm[k]
        wo = -d[idx]
        front = (n * wo).sum(-1) > 0                               # a back-face hit ends the path
        alive[idx[~front]] = False
        idx, t, k, n, wo = idx[front], t[front], k[front], n[front], wo[front]
        if idx.size == 0:
            continue
        p = o[idx] + t[:, None] * d[idx]
        tp = texel(o64, p, H, W)
        av, rv, mv = A[tp], R[tp], M[tp]
        masked = MK[tp]
        tq = tp.copy()
        if masked.any():
            tq[masked] = refracted_texel(o64, p[masked], n[masked], wo[masked], ior, refract_distance, H, W)
        bgv = BG[tq]
        po = p + (1e-5 * (1 + np.abs(p).max(-1)))[:, None] * n
        b = base[idx]
        vert = {"depth": depth, "pix": idx, "tp": tp, "tq": tq, "masked": masked, "wo": wo, "n": n, "em": np.zeros(idx.size, bool),
                "wl": np.zeros((idx.size, 3)), "te": np.zeros(idx.size, np.int64), "we": np.zeros(idx.size)}
        rec["masked_vertex"][idx[masked]] = True
        if have_tab:
            u0, u1, u2, u3 = (rng_u(b, depth, c) for c in (2, 3, 4, 5))
            row = np.searchsorted(row_cdf[:He], u0, side="right") - 1
            col = np.array([np.searchsorted(col_cdf[rr, :We], uu, side="right") - 1 for rr, uu in zip(row, u1)], dtype=np.int64)
            c0, c1 = np.cos(row * np.pi / He), np.cos((row + 1) * np.pi / He)
            ct = c0 + (c1 - c0) * u2
            st = np.sqrt(np.maximum(1 - ct * ct, 0))
            ph = (col + u3) * 2 * np.pi / We
            wl = np.stack([st * np.sin(ph), ct, -st * np.cos(ph)], -1)
            te = row * We + col
            pe = pdf_tab[te]
            fb, pb = eval_trans(o64, wl, wo, n, av, rv, mv, bgv, masked, ior, spec_trans)
            ok = (pe > 0) & ((n * wl).sum(-1) > 0) & (fb > 0).any(-1)    # an emitter sample only above the surface
            if ok.any():
                vis = np.zeros(idx.size, bool)
                vis[np.nonzero(ok)[0]] = ~occluded(po[ok], wl[ok])
                w = np.where(vis, mis(pe, pb) / np.where(pe > 0, pe, 1.0), 0.0)
                L[idx] += thr[idx] * fb * envf[te] * w[:, None]
                vert.update(em=vis, wl=wl, te=te, we=w)
        s1, s2a, s2b = (rng_u(b, depth, c) for c in (6, 7, 8))
        wi, pdf, wgt = sample_trans(o64, s1, np.stack([s2a, s2b], -1), wo, n, av, rv, mv, bgv, masked, ior, spec_trans)
        vert["wi"] = wi
        vert["ip"] = np.where(pdf > 0, 1.0 / (pdf + 1e-4), 0.0)
        rec["vertices"].append(vert)
        rec["below"][idx[masked & ~((n * wi).sum(-1) > 0)]] = True
        thr[idx] *= wgt
        dead = ~(thr[idx] > 0).any(-1)
        alive[idx[dead]] = False
        prev[idx] = pdf
        o[idx], d[idx] = po, wi                                      # the traced direction is the world direction
    return L.reshape(H, W, 3), rec


def trans_maps(a, r, m, mask, keep_albedo_color=False):
    """The maps as trans_edit.py:25-28 sets them inside the mask -> copies (a, r, m)."""
    a, r, m = np.array(a, np.float32), np.array(r, np.float32), np.array(m, np.float32)
    mk = np.asarray(mask, bool)
    if not keep_albedo_color:
        a[mk] = 0.7
    r[mk] = 0.3
    m[mk] = 0.0
    return a, r, m


def groove_mask(H, W):
    """The shared mask on the groove: its left wall from 0.3 H down (columns up to 0.45 W, a ragged border), the floor below the
    step there, and the two rows at the step across the whole width: the step's face is seen at a grazing angle, where BSDF samples
    leave below the surface.  The border crosses the 16 x 8 tiles and more than a third of the image stays unmasked."""
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    step = 2 * H // 3
    return ((j < int(0.45 * W) + (i % 3)) & (i >= int(0.3 * H))) | ((i >= step - 1) & (i <= step))


def trans_scene(pathtrace, H=20, W=24):
    """The scene the host and the GPU tests share: the groove at 24 x 20 (or H x W), a random background, `groove_mask`, the maps as
    trans_edit.py sets them inside it.  `pathtrace`: materialist_amd.pathtrace (for the envmap tables)."""
    from materialist_amd import mesh

    import path_fp64 as pf

    rm = mesh.reference_mesh(pf.groove_scene(H, W), FOV)
    rng = np.random.default_rng(11)
    a, r, m = pf.groove_maps(H, W, rng)
    env = pf.groove_env(rng)
    mask = groove_mask(H, W)
    bg = rng.uniform(0.0, 1.0, (H, W, 3)).astype(np.float32)
    a, r, m = trans_maps(a, r, m, mask)
    return {"rm": rm, "V": rm["vertices"].astype(np.float32).astype(np.float64), "T": rm["triangles"], "a": a, "r": r, "m": m, "env": env,
            "tab": pathtrace.env_tables(env), "mask": mask, "bg": bg, "H": H, "W": W}


# (max_depth, seed, ior, T) of the parity renders: spp 1
CASES = [(d, s, 1.2, 0.4) for d in (2, 4, 16) for s in (0, 1, 2)] + [(4, 0, 1.5, 1.0)]
