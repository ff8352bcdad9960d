"""fp64 restatement of the path render with PBR inserted objects ("PBR inserted objects"):
`path_oi_smooth_fp64.replay_oi` with a third object kind, {"type": "pbr", "albedo", "roughness", "metallic"}, whose vertices are the
depth mesh's vertices under "Shading normals" on the constants of the object instead of on a texel:

  * one-sided about the outward face normal ng (ng . wo <= 0 ends the path with nothing added); no texel is read;
  * ns = ng on a flat object, the interpolated corner normal with its three fallbacks on a smooth one;
  * emitter sample (dims 2-5): needs pdf_e > 0 and ng . wl > 0; f and pdf_b from the fp64 BSDF about ns; a shadow ray where some
    f[c] > 0; the power heuristic;
  * BSDF sample (dims 6, 7, 8) about ns: the reference's lobe choice and weight (the oracle's sample_brdf); never a delta event; a
    sample with ng . wi <= 0 ends the path, on a flat object too; the next ray starts at p + eps ng.

The depth mesh, the dielectric and the diffuse object run `path_oi_smooth_fp64.replay_oi`'s statements (without a PBR object the two
functions return the same bits).  The object's constants are rounded to fp32, as the library's record holds them.

The record gains, per pixel: `pbr_vertex` (a vertex on a PBR object), `pbr_smooth_vertex` (on a smooth one), `pbr_below_ng` (a BSDF
sample ended by ng . wi <= 0; `pbr_below_ng_carrying`: one whose weight about ns was not zero already, which only a smooth object
has), `pbr_emitter_below_ng` (an emitter sample the BSDF about ns would have carried, refused by
ng . wl <= 0); `blocked_by_object` and `fallback` as before."""
import math

import numpy as np

import path_oi_fp64 as po
import path_oi_smooth_fp64 as ps
from path_fp64 import FOV, brute, env_texel, mis, pcg, rng_u, texel

SCENE, DIELECTRIC, DIFFUSE, PBR = po.SCENE, po.DIELECTRIC, po.DIFFUSE, 3

PBR_DEFAULTS = {"albedo": 0.8, "roughness": 0.5, "metallic": 0.0}


def pbr_constants(bsdf):
    """(a [3], r, m) of a "pbr" dict in fp64, rounded to fp32 first: the values the library's record holds."""
    f32 = lambda x: np.asarray(x, np.float64).astype(np.float32).astype(np.float64)
    a = np.broadcast_to(f32(bsdf.get("albedo", PBR_DEFAULTS["albedo"])), (3,))
    return a, float(f32(bsdf.get("roughness", PBR_DEFAULTS["roughness"]))), float(f32(bsdf.get("metallic", PBR_DEFAULTS["metallic"])))


def replay_oi(o64, V, T, a, r, m, env, tab, H, W, max_depth, seed, objects=(), sample=0, closest=None, occluded=None):
    """`path_oi_smooth_fp64.replay_oi` where an object's bsdf may be of type "pbr" -> (L [H,W,3], record)."""
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
    kind_of = np.zeros(T.shape[0], np.int64)
    par = np.zeros((T.shape[0], 3))
    mat = np.zeros((T.shape[0], 5))                                # a PBR object's a (3), r, m
    smooth_of = np.zeros(T.shape[0], bool)
    corner = np.zeros((T.shape[0], 3, 3))
    for ob in objects:
        sl = slice(ob["first_tri"], ob["first_tri"] + ob["n_tri"])
        b = ob["bsdf"]
        if b["type"] == "dielectric":
            kind_of[sl], par[sl] = DIELECTRIC, [b["int_ior"], b["ext_ior"], 0.0]
        elif b["type"] == "pbr":
            ca, cr, cm = pbr_constants(b)
            kind_of[sl], mat[sl] = PBR, [*ca, cr, cm]
        else:
            kind_of[sl], par[sl] = DIFFUSE, np.broadcast_to(np.asarray(b["reflectance"], np.float64), (3,))
        if ob.get("corner_normals") is not None:
            smooth_of[sl], corner[sl] = True, np.asarray(ob["corner_normals"], np.float64)
    is_obj = kind_of != SCENE
    P_obj = P[is_obj]
    nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    nrm *= np.where(((nrm * P[:, 0]).sum(-1, keepdims=True) > 0) & ~is_obj[:, None], -1.0, 1.0)
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
    prev_delta = np.zeros(N, bool)
    alive = np.ones(N, bool)
    A, R, M = a.reshape(-1, 3).astype(np.float64), r.reshape(-1).astype(np.float64), m.reshape(-1).astype(np.float64)
    z = lambda: np.zeros(N, bool)
    rec = {"H": H, "W": W, "He": He, "We": We, "pixels": pix.astype(np.int64), "full": True, "escapes": [], "vertices": [],
           "object_vertices": [], "transmitted": z(), "diffuse_object": z(), "blocked_by_object": z(),
           "smooth_transmitted": z(), "smooth_diffuse": z(), "redo": z(), "fallback": z(), "fallback_cause": np.zeros((N, 3), bool),
           "pbr_vertex": z(), "pbr_smooth_vertex": z(), "pbr_below_ng": z(), "pbr_below_ng_carrying": z(),
           "pbr_emitter_below_ng": z()}

    def emitter(b, depth):
        u0, u1, u2, u3 = (rng_u(b, depth, c) for c in (2, 3, 4, 5))
        row = np.searchsorted(row_cdf[:He], u0, side="right") - 1
        col = np.array([np.searchsorted(col_cdf[rr, :We], uu, side="right") - 1 for rr, uu in zip(row, u1)], dtype=np.int64)
        c0, c1 = np.cos(row * np.pi / He), np.cos((row + 1) * np.pi / He)
        ct = c0 + (c1 - c0) * u2
        st = np.sqrt(np.maximum(1 - ct * ct, 0))
        ph = (col + u3) * 2 * np.pi / We
        wl = np.stack([st * np.sin(ph), ct, -st * np.cos(ph)], -1)
        te = row * We + col
        return wl, te, pdf_tab[te]

    def shadow(idx, ok, po_, wl):
        vis = np.zeros(idx.size, bool)
        if ok.any():
            vis[np.nonzero(ok)[0]] = ~occluded(po_[ok], wl[ok])
            if P_obj.shape[0]:
                rec["blocked_by_object"][idx[ok][np.isfinite(brute(P_obj, po_[ok], wl[ok])[0])]] = True
        return vis

    for depth in range(max_depth + 1):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        t, k = closest(o[idx], d[idx])
        miss = k < 0
        im = idx[miss]
        if im.size:
            tx = env_texel(d[im], He, We)
            w = np.ones(im.size) if depth == 0 else np.where(prev_delta[im], 1.0, mis(prev[im], pdf_tab[tx] if have_tab else 0.0))
            L[im] += thr[im] * envf[tx] * w[:, None]
            rec["escapes"].append({"depth": depth, "pix": im, "tx": tx, "w": w})
        alive[im] = False
        if depth + 1 >= max_depth:
            alive[:] = False
            break
        idx, t, k = idx[~miss], t[~miss], k[~miss]
        n = nrm[k]
        wo = -d[idx]
        kind = kind_of[k]
        front = ((n * wo).sum(-1) > 0) | (kind == DIELECTRIC)      # only the dielectric shades from behind
        alive[idx[~front]] = False
        idx, t, k, n, wo, kind = idx[front], t[front], k[front], n[front], wo[front], kind[front]
        if idx.size == 0:
            continue
        p_all = o[idx] + t[:, None] * d[idx]
        eps_all = 1e-5 * (1 + np.abs(p_all).max(-1))
        sm = smooth_of[k]
        nsh = n.copy()
        if sm.any():
            bu, bv = ps.barycentrics(P[k[sm]], o[idx[sm]], d[idx[sm]])
            nsh[sm], cause = ps.shading_normal(corner[k[sm]], bu, bv, n[sm], wo[sm])
            rec["fallback_cause"][idx[sm]] |= cause
            rec["fallback"][idx[sm]] |= cause.any(-1)
        sel = kind == SCENE
        if sel.any():                                              # ---- the depth mesh: path_fp64.replay's statements
            ids, ns, wos, p = idx[sel], n[sel], wo[sel], p_all[sel]
            tp = texel(o64, p, H, W)
            av, rv, mv = A[tp], R[tp], M[tp]
            po_ = p + (1e-5 * (1 + np.abs(p).max(-1)))[:, None] * ns
            b = base[ids]
            vert = {"depth": depth, "pix": ids, "tp": tp, "wo": wos, "n": ns, "em": np.zeros(ids.size, bool), "wl": np.zeros((ids.size, 3)),
                    "te": np.zeros(ids.size, np.int64), "we": np.zeros(ids.size)}
            if have_tab:
                wl, te, pe = emitter(b, depth)
                fb, pb = o64.eval_brdf(wl, wos, ns, av, rv, mv)
                ok = (pe > 0) & ((ns * wl).sum(-1) > 0) & (fb > 0).any(-1)
                if ok.any():
                    vis = shadow(ids, ok, po_, wl)
                    w = np.where(vis, mis(pe, pb) / np.where(pe > 0, pe, 1.0), 0.0)
                    L[ids] += thr[ids] * fb * envf[te] * w[:, None]
                    vert.update(em=vis, wl=wl, te=te, we=w)
            s1, s2a, s2b = (rng_u(b, depth, c) for c in (6, 7, 8))
            wi, pdf, wgt = o64.sample_brdf(s1, np.stack([s2a, s2b], -1), wos, ns, av, rv, mv)
            vert["wi"] = wi
            vert["ip"] = np.where(pdf > 1e-6, 1.0 / (pdf + 1e-6), 0.0)
            rec["vertices"].append(vert)
            thr[ids] *= wgt
            dead = ~(thr[ids] > 0).any(-1)
            alive[ids[dead]] = False
            prev[ids] = pdf
            prev_delta[ids] = False
            o[ids], d[ids] = po_, wi
        sel = kind == PBR
        if sel.any():                                              # ---- a PBR object: the depth mesh's vertex on the object's constants
            ids, ng, ns, wos, p = idx[sel], n[sel], nsh[sel], wo[sel], p_all[sel]
            cm = mat[k[sel]]
            av, rv, mv = cm[:, :3], cm[:, 3], cm[:, 4]
            po_ = p + eps_all[sel][:, None] * ng                   # +eps along ng
            b = base[ids]
            rec["pbr_vertex"][ids] = True
            rec["pbr_smooth_vertex"][ids[sm[sel]]] = True
            if have_tab:
                wl, te, pe = emitter(b, depth)
                fb, pb = o64.eval_brdf(wl, wos, ns, av, rv, mv)
                above = (ng * wl).sum(-1) > 0
                carried = (pe > 0) & (fb > 0).any(-1)
                rec["pbr_emitter_below_ng"][ids[carried & ~above]] = True
                ok = carried & above
                if ok.any():
                    vis = shadow(ids, ok, po_, wl)
                    w = np.where(vis, mis(pe, pb) / np.where(pe > 0, pe, 1.0), 0.0)
                    L[ids] += thr[ids] * fb * envf[te] * w[:, None]
            s1, s2a, s2b = (rng_u(b, depth, c) for c in (6, 7, 8))
            wi, pdf, wgt = o64.sample_brdf(s1, np.stack([s2a, s2b], -1), wos, ns, av, rv, mv)
            below = ~((ng * wi).sum(-1) > 0)                       # a sample that leaves below the face ends the path
            rec["pbr_below_ng"][ids[below]] = True
            rec["pbr_below_ng_carrying"][ids[below & (wgt > 0).any(-1)]] = True
            thr[ids] *= wgt
            dead = ~(thr[ids] > 0).any(-1) | below
            alive[ids[dead]] = False
            prev[ids] = pdf
            prev_delta[ids] = False
            o[ids], d[ids] = po_, wi
            rec["object_vertices"].append({"depth": depth, "pix": ids, "kind": PBR, "wi": wi, "smooth": sm[sel], "below": below})
        sel = kind == DIFFUSE
        if sel.any():                                              # ---- a diffuse object: f cos = rho / pi max(ns . wi, 0)
            ids, ng, ns, p, rho = idx[sel], n[sel], nsh[sel], p_all[sel], par[k[sel]]
            po_ = p + eps_all[sel][:, None] * ng
            b = base[ids]
            rec["diffuse_object"][ids] = True
            rec["smooth_diffuse"][ids[sm[sel]]] = True
            if have_tab:
                wl, te, pe = emitter(b, depth)
                c = np.maximum((ns * wl).sum(-1), 0.0)
                fb, pb = rho * (c / np.pi)[:, None], c / np.pi
                ok = (pe > 0) & ((ng * wl).sum(-1) > 0) & (fb > 0).any(-1)
                vis = shadow(ids, ok, po_, wl)
                w = np.where(vis, mis(pe, pb) / np.where(pe > 0, pe, 1.0), 0.0)
                L[ids] += thr[ids] * fb * envf[te] * w[:, None]
            wi, pdf = po.sample_diffuse(ns, rng_u(b, depth, 7), rng_u(b, depth, 8))
            below = ~((ng * wi).sum(-1) > 0)
            thr[ids] *= np.where(below[:, None], 0.0, rho)
            alive[ids[~(thr[ids] > 0).any(-1)]] = False
            prev[ids] = pdf
            prev_delta[ids] = False
            o[ids], d[ids] = po_, wi
            rec["object_vertices"].append({"depth": depth, "pix": ids, "kind": DIFFUSE, "wi": wi, "smooth": sm[sel], "below": below})
        sel = kind == DIELECTRIC
        if sel.any():                                              # ---- glass: a delta vertex, no emitter sample
            ids, ng, ns, p, pr = idx[sel], n[sel], nsh[sel], p_all[sel], par[k[sel]]
            wi, wgt, prob, trans, redo = ps.sample_dielectric_shading(pr[:, 0], pr[:, 1], ng, ns, wo[sel], rng_u(base[ids], depth, 6))
            side = np.where((ng * wi).sum(-1) > 0, 1.0, -1.0)
            thr[ids] *= wgt[:, None]
            prev[ids] = prob
            prev_delta[ids] = True
            o[ids], d[ids] = p + (side * eps_all[sel])[:, None] * ng, wi
            rec["transmitted"][ids[trans]] = True
            rec["smooth_transmitted"][ids[trans & sm[sel]]] = True
            rec["redo"][ids[redo]] = True
            rec["object_vertices"].append({"depth": depth, "pix": ids, "kind": DIELECTRIC, "wi": wi, "transmitted": trans, "smooth": sm[sel],
                                           "redo": redo})
    return L.reshape(H, W, 3), rec


# ---- the shared test scenes ----------------------------------------------------------------------------------------------------------
METAL = {"type": "pbr", "albedo": (0.95, 0.64, 0.54), "roughness": 0.07, "metallic": 1.0}     # copper-coloured, at the roughness floor
PLASTIC = {"type": "pbr", "albedo": 0.5, "roughness": 0.6, "metallic": 0.0}
METAL_CENTRE, METAL_RADIUS = (0.096, 0.017, -1.30), 0.103
GLASS_CENTRE, GLASS_RADIUS = (-0.083, 0.07, -1.123), 0.104
PBR_CUBE = ((-0.01, 0.17, -1.40), 0.11, (0.5, -0.4, 0.3))
DIFFUSE_CUBE = ((-0.04, -0.15, -1.32), 0.12, (-0.3, 0.7, 0.2))


def table_scene():
    """All four object code paths in one table, in front of a depth mesh at z <= -1.6: a smooth metal icosphere and a smooth glass
    icosphere of level 1 (80 triangles each: at their silhouettes the interpolated normal turns away from the viewer while the face
    still looks at it, and a mirror reflection about it can leave below the face), a flat PBR cube and a flat diffuse cube."""
    Vm, Tm, Nm = ps.icosphere(METAL_CENTRE, METAL_RADIUS, 1)
    Vc, Tc = po.cube(*PBR_CUBE)
    Vg, Tg, Ng = ps.icosphere(GLASS_CENTRE, GLASS_RADIUS, 1)
    Vd, Td = po.cube(*DIFFUSE_CUBE)
    return [{"vertices": Vm, "triangles": Tm, "bsdf": METAL, "normals": Nm},
            {"vertices": Vc, "triangles": Tc, "bsdf": PLASTIC},
            {"vertices": Vg, "triangles": Tg, "bsdf": po.GLASS, "normals": Ng},
            {"vertices": Vd, "triangles": Td, "bsdf": po.DIFFUSE_08}]


merged = ps.merged      # the table entries keep their "bsdf" dicts, so a "pbr" one passes through


def quad(z=-1.5):
    """The unit square of two triangles across the whole view at depth z, wound so that e1 x e2 points at the camera -> (V [4,3],
    T [2,3]): as a depth mesh the builder keeps the winding, as an inserted object it faces the camera.  Its edges are (1, 0, 0),
    (1, 1, 0) and (0, 1, 0): e1 x e2 = (0, 0, 1) without rounding, in any precision."""
    V = np.array([[-0.5, -0.5, z], [0.5, -0.5, z], [0.5, 0.5, z], [-0.5, 0.5, z]], np.float64)
    return V, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


FAR_TRIANGLE = (np.array([[50.0, 50.0, -1.0], [50.001, 50.0, -1.0], [50.0, 50.001, -1.0]]), np.array([[0, 1, 2]], np.int32))   # out of view
