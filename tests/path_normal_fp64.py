"""fp64 restatement of the path render under a shading-normal map ("Shading normals"), built on path_fp64.

A depth-mesh vertex has two normals.  `ng`, the hit triangle's face normal turned to the camera side, keeps everything geometric: the
back-face test, the spawn offset, and which side a direction leaves on (an emitter sample or a BSDF sample with ng . w <= 0 carries
nothing).  `ns = nrm[tp]`, the map at the texel the vertex reads its material from, is MatDiffBSDF's `normal`: every cosine, both
samplers' frames, the pdf.

`replay_normal` is `path_fp64.replay` with those rules; its record holds the shading normal of each vertex under "n", so that
path_fp64's `held_radiance` / `held_grad` read it as they read the face normal, and a BSDF sample below the sheet as 1/(pdf + 1e-6) =
0.  `held_radiance_normal` / `held_grad_normal` take the map as a parameter (sampling held); `d_n` is the analytic d f / d n of
`dfdn`, with respect to the three components as free variables.  `normal_scene` is the groove with a tilted unit normal map."""
import math

import numpy as np

import path_fp64 as pf

FOV = pf.FOV
TILT = 0.35        # normal_scene's noise: enough that BSDF samples fall below ng, little enough for the two-traversal cap (test_path_normal_host)


def dfdn(wi, wo, n, a, r, m, g):
    """d (g . f) / d n of MatDiffBSDF.eval_brdf's value f (RGB, with its cosine), lanes [N,...], numpy fp64: gl wi + gv wo + gh h with
    each cosine's gradient passed where the raw cosine is positive (dr.maximum).  Also returns (gl, gv, gh) after the gates."""
    wi, wo, n, a, g = (np.asarray(x, np.float64).reshape(-1, 3) for x in (wi, wo, n, a, g))
    r, m = np.asarray(r, np.float64).reshape(-1), np.asarray(m, np.float64).reshape(-1)
    h = wi + wo
    h = h / np.linalg.norm(h, axis=-1, keepdims=True)
    nl, nv, nh = (n * wi).sum(-1), (n * wo).sum(-1), (n * h).sum(-1)
    NoL, NoV, NoH = np.maximum(nl, 0), np.maximum(nv, 0), np.maximum(nh, 0)
    VoH = np.maximum((wo * h).sum(-1), 0)
    alpha2 = r ** 4
    den = NoH * NoH * (alpha2 - 1) + 1 + 1e-6
    D = alpha2 / (np.pi * den * den)
    dD_dNoH = -4 * alpha2 * NoH * (alpha2 - 1) / (np.pi * den ** 3)
    k = (r + 1) ** 2 / 8
    g1l, g1v = 1 / (NoL * (1 - k) + k + 1e-6), 1 / (NoV * (1 - k) + k + 1e-6)
    G = g1l * g1v
    dG_dNoL, dG_dNoV = -g1l * g1l * (1 - k) * g1v, -g1v * g1v * (1 - k) * g1l
    FDm1 = 2 * VoH * VoH * r - 0.5
    Fo, Fi = 1 + FDm1 * (1 - NoV) ** 5, 1 + FDm1 * (1 - NoL) ** 5
    dFo, dFi = -5 * FDm1 * (1 - NoV) ** 4, -5 * FDm1 * (1 - NoL) ** 4
    x5 = (1 - VoH) ** 5
    kd = a * (1 - m)[:, None] / np.pi
    C0 = (1 - m)[:, None] * 0.04 + m[:, None] * a
    Fm = C0 + (1 - C0) * x5[:, None]
    gd, gs = (g * kd).sum(-1), (g * Fm).sum(-1)
    gl = gd * Fo * (dFi * NoL + Fi) + gs * D / 4 * (dG_dNoL * NoL + G)
    gv = gd * dFo * Fi * NoL + gs * D * dG_dNoV / 4 * NoL
    gh = gs * dD_dNoH * G / 4 * NoL
    gl, gv, gh = np.where(nl > 0, gl, 0.0), np.where(nv > 0, gv, 0.0), np.where(nh > 0, gh, 0.0)
    return gl[:, None] * wi + gv[:, None] * wo + gh[:, None] * h, (gl, gv, gh)


def face_normals(V, T):
    """Unit face normal of every triangle, turned to the camera at the origin (as path_fp64.replay turns them)."""
    P = V[T]
    ng = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    ng *= np.where((ng * P[:, 0]).sum(-1, keepdims=True) > 0, -1.0, 1.0)
    return ng / np.maximum(np.linalg.norm(ng, axis=-1, keepdims=True), 1e-300)


def replay_normal(o64, V, T, a, r, m, env, tab, nrm, H, W, max_depth, seed, pixels=None, sample=0, closest=None, occluded=None):
    """`path_fp64.replay` under the normal map nrm [H,W,3] (used as given) -> (L, record).  The record is path_fp64's, with per vertex
    "n" = the shading normal, "ng" = the face normal, "below" = the BSDF sample left with ng . wi <= 0 (then "ip" is 0: the path ends),
    and per row of the record the masks "below" and "nov0" (a vertex with ns . wo <= 0 was shaded)."""
    He, We = env.shape[:2]
    envf = env.reshape(-1, 3).astype(np.float64)
    pdf_tab = tab["pdf"].reshape(-1).astype(np.float64)
    row_cdf, col_cdf = tab["row_cdf"], tab["col_cdf"]
    have_tab = tab["row_cdf"][-1] > 0
    P = V[T]
    if closest is None:
        closest = lambda o, d: pf.brute(P, o, d)
    if occluded is None:
        occluded = lambda o, d: np.isfinite(pf.brute(P, o, d)[0])
    face = face_normals(V, T)
    NS = np.asarray(nrm, np.float32).reshape(-1, 3).astype(np.float64)
    pix = np.arange(H * W, dtype=np.uint32) if pixels is None else np.asarray(pixels, dtype=np.int64).astype(np.uint32)
    N = pix.size
    base = pf.pcg(pf.pcg(pf.pcg(np.uint32(seed)) + pix) + np.uint32(sample))
    ii, jj = pix // W, pix % W
    f = (W / 2.0) / math.tan(math.radians(FOV) / 2.0)
    x = jj - 0.5 + pf.rng_u(base, 0, 0)
    y = ii - 0.5 + pf.rng_u(base, 0, 1)
    d = np.stack([(x - (W - 1) / 2) / f, -(y - (H - 1) / 2) / f, -np.ones(N)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.zeros((N, 3))
    L, thr, prev = np.zeros((N, 3)), np.ones((N, 3)), np.zeros(N)
    alive = np.ones(N, bool)
    A, R, M = a.reshape(-1, 3).astype(np.float64), r.reshape(-1).astype(np.float64), m.reshape(-1).astype(np.float64)
    rec = {"H": H, "W": W, "He": He, "We": We, "pixels": pix.astype(np.int64), "full": pixels is None, "escapes": [], "vertices": [],
           "below": np.zeros(N, bool), "nov0": np.zeros(N, bool)}
    for depth in range(max_depth + 1):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        t, k = closest(o[idx], d[idx])
        miss = k < 0
        im = idx[miss]
        if im.size:
            tx = pf.env_texel(d[im], He, We)
            w = np.ones(im.size) if depth == 0 else pf.mis(prev[im], pdf_tab[tx] if have_tab else 0.0)
            L[im] += thr[im] * envf[tx] * w[:, None]
            rec["escapes"].append({"depth": depth, "pix": im, "tx": tx, "w": w})
        alive[im] = False
        if depth + 1 >= max_depth:
            alive[:] = False
            break
        idx, t, k = idx[~miss], t[~miss], k[~miss]
        ng = face[k]
        wo = -d[idx]
        front = (ng * wo).sum(-1) > 0                        # geometric: a back-face hit ends the path
        alive[idx[~front]] = False
        idx, t, k, ng, wo = idx[front], t[front], k[front], ng[front], wo[front]
        if idx.size == 0:
            continue
        p = o[idx] + t[:, None] * d[idx]
        tp = pf.texel(o64, p, H, W)
        ns = NS[tp]
        av, rv, mv = A[tp], R[tp], M[tp]
        po = p + (1e-5 * (1 + np.abs(p).max(-1)))[:, None] * ng   # geometric: the spawn offset
        b = base[idx]
        rec["nov0"][idx[(ns * wo).sum(-1) <= 0]] = True
        vert = {"depth": depth, "pix": idx, "tp": tp, "wo": wo, "n": ns, "ng": ng, "em": np.zeros(idx.size, bool), "wl": np.zeros((idx.size, 3)),
                "te": np.zeros(idx.size, np.int64), "we": np.zeros(idx.size)}
        if have_tab:
            u0, u1, u2, u3 = (pf.rng_u(b, depth, c) for c in (2, 3, 4, 5))
            row = np.searchsorted(row_cdf[:He], u0, side="right") - 1
            col = np.array([np.searchsorted(col_cdf[rr, :We], uu, side="right") - 1 for rr, uu in zip(row, u1)])
            c0, c1 = np.cos(row * np.pi / He), np.cos((row + 1) * np.pi / He)
            ct = c0 + (c1 - c0) * u2
            st = np.sqrt(np.maximum(1 - ct * ct, 0))
            ph = (col + u3) * 2 * np.pi / We
            wl = np.stack([st * np.sin(ph), ct, -st * np.cos(ph)], -1)
            te = row * We + col
            pe = pdf_tab[te]
            fb, pb = o64.eval_brdf(wl, wo, ns, av, rv, mv)
            ok = (pe > 0) & ((ng * wl).sum(-1) > 0) & (fb > 0).any(-1)      # ng . wl > 0 as well as f > 0
            if ok.any():
                vis = np.zeros(idx.size, bool)
                vis[np.nonzero(ok)[0]] = ~occluded(po[ok], wl[ok])
                w = np.where(vis, pf.mis(pe, pb) / np.where(pe > 0, pe, 1.0), 0.0)
                L[idx] += thr[idx] * fb * envf[te] * w[:, None]
                vert.update(em=vis, wl=wl, te=te, we=w)
        s1, s2a, s2b = (pf.rng_u(b, depth, c) for c in (6, 7, 8))
        wi, pdf, wgt = o64.sample_brdf(s1, np.stack([s2a, s2b], -1), wo, ns, av, rv, mv)
        below = ~((ng * wi).sum(-1) > 0)                      # geometric: a sample below the sheet ends the path
        wgt = np.where(below[:, None], 0.0, wgt)
        rec["below"][idx[below]] = True
        vert["wi"] = wi
        vert["below"] = below
        vert["ip"] = np.where((pdf > 1e-6) & ~below, 1.0 / (pdf + 1e-6), 0.0)
        rec["vertices"].append(vert)
        thr[idx] *= wgt
        dead = ~(thr[idx] > 0).any(-1)
        alive[idx[dead]] = False
        prev[idx] = pdf
        o[idx], d[idx] = po, wi
    return (L.reshape(H, W, 3) if pixels is None else L), rec


def _with_normals(rec, nrm):
    """The record(s) with every vertex's shading normal read from `nrm` (sampling held: texels, directions and weights stay)."""
    if isinstance(rec, (list, tuple)):
        return [_with_normals(x, nrm) for x in rec]
    NS = np.asarray(nrm, np.float64).reshape(-1, 3)
    return dict(rec, vertices=[dict(v, n=NS[v["tp"]]) for v in rec["vertices"]])


def held_radiance_normal(o64, rec, a, r, m, env, nrm):
    """`path_fp64.held_radiance` of the recorded paths under the maps, the envmap and the normal map `nrm`."""
    return pf.held_radiance(o64, _with_normals(rec, nrm), a, r, m, env)


def held_grad_normal(o64, rec, a, r, m, env, nrm, d_out):
    """d (sum d_out . held_radiance_normal) / d (a, r, m, env, n): path_fp64.held_grad's dict plus "n" [H,W,3]: at every vertex both
    BSDF values, the emitter term's f_e and the sample factor's f_s, send `dfdn` with held_grad's upstreams to the vertex's texel."""
    if isinstance(rec, (list, tuple)):
        gs = [held_grad_normal(o64, x, a, r, m, env, nrm, d_out) for x in rec]
        return {k: sum(g[k] for g in gs) / len(gs) for k in gs[0]}
    rec = _with_normals(rec, nrm)
    out = pf.held_grad(o64, rec, a, r, m, env, d_out)
    H, W = rec["H"], rec["W"]
    g = d_out.reshape(H * W, 3).astype(np.float64)[rec["pixels"]]
    A, R, M = a.reshape(-1, 3).astype(np.float64), r.reshape(-1).astype(np.float64), m.reshape(-1).astype(np.float64)
    E = env.reshape(-1, 3).astype(np.float64)
    rows = pf._terms(o64, rec, a, r, m, env)
    d_n = np.zeros((H * W, 3))
    tail = np.zeros((rec["pixels"].size, 3))
    for k in range(len(rows) - 1, -1, -1):
        row = rows[k]
        if "v" in row:
            v = row["v"]
            pix, tp = v["pix"], v["tp"]
            with np.errstate(divide="ignore", invalid="ignore"):
                gs = np.where(row["fs"] > 0, g[pix] * tail[pix] / row["fs"], 0.0)
            gs = np.where(v["ip"][:, None] > 0, gs, 0.0)
            np.add.at(d_n, tp, dfdn(v["wi"], v["wo"], v["n"], A[tp], R[tp], M[tp], gs)[0])
            em = v["em"]
            if em.any():
                ge = g[pix] * row["thr"] * E[v["te"]] * v["we"][:, None]
                np.add.at(d_n, tp[em], dfdn(v["wl"][em], v["wo"][em], v["n"][em], A[tp[em]], R[tp[em]], M[tp[em]], ge[em])[0])
            tail = tail + row["E"]
        tail = tail + row["S"]
    out["n"] = d_n.reshape(H, W, 3)
    return out


def pixel_normals(rm):
    """The face-derived normal of every pixel: the mesher's area-weighted vertex normal (pixel centres are the vertices); a pixel
    without triangles looks at the camera."""
    n = np.array(rm["normals"], np.float64)
    n[~rm["has_faces"]] = [0.0, 0.0, 1.0]
    return n


def tilted_normals(rm, H, W, tilt=TILT, seed=17, plant=True):
    """normalize(face-derived pixel normal + tilt * noise) as fp32, with planted texels (every 37th, from the 5th) whose normal is
    turned away from their own camera ray: ns . wo = -0.1 at their camera vertex."""
    rng = np.random.default_rng(seed)
    n = pixel_normals(rm) + tilt * rng.normal(size=(H, W, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    planted = np.zeros(H * W, bool)
    if plant:
        planted[5::37] = True
        f = (W / 2.0) / math.tan(math.radians(FOV) / 2.0)
        i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        wo = -np.stack([(j - (W - 1) / 2) / f, -(i - (H - 1) / 2) / f, -np.ones_like(i)], -1)
        wo /= np.linalg.norm(wo, axis=-1, keepdims=True)
        tang = np.cross(wo, np.array([0.0, 1.0, 0.0]))
        tang /= np.linalg.norm(tang, axis=-1, keepdims=True)
        away = tang - 0.1 * wo
        away /= np.linalg.norm(away, axis=-1, keepdims=True)
        n.reshape(-1, 3)[planted] = away.reshape(-1, 3)[planted]
    n32 = n.astype(np.float32)
    n32 /= np.linalg.norm(n32.astype(np.float64), axis=-1, keepdims=True).astype(np.float32)
    return np.ascontiguousarray(n32), planted.reshape(H, W)


# (max_depth, seed) of the forward parity renders, shared by the GPU test and the host test's two-traversal comparison
CASES = [(md, seed) for md in (2, 4) for seed in (0, 1, 2)]
SIZES = [(24, 24), (36, 20), (17, 9)]      # (H, W): the parity scene and the partial tiles


def normal_scene(pathtrace, H=24, W=24):
    """The groove (path_fp64's mesh, maps and envmap) under `tilted_normals`: what every normal-map test renders."""
    from materialist_amd import mesh

    rm = mesh.reference_mesh(pf.groove_scene(H, W), FOV)
    rng = np.random.default_rng(11)
    a, r, m = pf.groove_maps(H, W, rng)
    env = pf.groove_env(rng)
    nrm, planted = tilted_normals(rm, H, W)
    return {"rm": rm, "a": a, "r": r, "m": m, "env": env, "nrm": nrm, "planted": planted, "tab": pathtrace.env_tables(env), "H": H, "W": W,
            "V": rm["vertices"].astype(np.float32).astype(np.float64), "T": rm["triangles"]}
