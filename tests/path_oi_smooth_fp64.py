"""fp64 restatement of the path render with smooth inserted objects ("Smooth inserted objects"):
`path_oi_fp64.replay_oi` with corner normals.  An object of the table may carry "corner_normals" [n_tri,3,3] (one normal per corner
of each of its triangles, in input order); at a hit on it the BSDF shades with the normal interpolated at the hit point and the
face normal keeps the geometry.  Objects without them, and the depth mesh, run `replay_oi`'s statements.

The record gains, per pixel: `smooth_transmitted` (a transmitted vertex on a smooth dielectric), `smooth_diffuse` (a vertex on a
smooth diffuse object), `redo` (a dielectric event about ns disagreed with the geometry and was redone about ng) and `fallback`
(one of the three fallbacks to the face normal fired), the last also split by cause in `fallback_cause` [N,3]."""
import math

import numpy as np

import path_oi_fp64 as po
from path_fp64 import FOV, brute, env_texel, mis, pcg, rng_u, texel

SCENE, DIELECTRIC, DIFFUSE = po.SCENE, po.DIELECTRIC, po.DIFFUSE


def barycentrics(P, o, d):
    """Moller-Trumbore's u, v of rays o + t d [N,3] on the triangles P [N,3,3]: u belongs to P[:, 1], v to P[:, 2]."""
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    pv = np.cross(d, e2)
    with np.errstate(divide="ignore", invalid="ignore"):
        idet = 1.0 / (e1 * pv).sum(-1)
        tv = o - P[:, 0]
        u = (tv * pv).sum(-1) * idet
        v = (d * np.cross(tv, e1)).sum(-1) * idet
    return u, v


def shading_normal(cn, u, v, ng, wo=None):
    """ns = normalize((1 - u - v) n0 + u n1 + v n2) for cn [N,3,3]; ns = ng where it is not finite or of zero length, where
    ns . ng <= 0 and, given wo, where (ns . wo)(ng . wo) <= 0 -> (ns [N,3], cause [N,3] bool: which fallback fired)."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        s = (1.0 - u - v)[:, None] * cn[:, 0] + u[:, None] * cn[:, 1] + v[:, None] * cn[:, 2]
        ln = np.linalg.norm(s, axis=-1)
        bad0 = ~(np.isfinite(ln) & (ln > 0))
        ns = np.where(bad0[:, None], ng, s / np.where(bad0, 1.0, ln)[:, None])
        bad1 = ~bad0 & ~((ns * ng).sum(-1) > 0)
        ns = np.where(bad1[:, None], ng, ns)
        bad2 = np.zeros_like(bad0)
        if wo is not None:
            bad2 = ~bad0 & ~bad1 & ~((ns * wo).sum(-1) * (ng * wo).sum(-1) > 0)
            ns = np.where(bad2[:, None], ng, ns)
    return ns, np.stack([bad0, bad1, bad2], -1)


def sample_dielectric_shading(int_ior, ext_ior, ng, ns, wo, u):
    """`path_oi_fp64.sample_dielectric` about ns, checked against the geometry: a reflected wi lies on wo's side of ng, a transmitted
    one on the other; where that fails the event is redone about ng with the same u -> (wi, weight, probability, transmitted, redone)."""
    wi, wgt, prob, trans = po.sample_dielectric(int_ior, ext_ior, ns, wo, u)
    side = (ng * wi).sum(-1) * (ng * wo).sum(-1)
    redo = ~np.where(trans, side < 0, side > 0)
    if redo.any():
        wi2, wgt2, prob2, trans2 = po.sample_dielectric(int_ior, ext_ior, ng, wo, u)
        wi, wgt = np.where(redo[:, None], wi2, wi), np.where(redo, wgt2, wgt)
        prob, trans = np.where(redo, prob2, prob), np.where(redo, trans2, trans)
    return wi, wgt, prob, trans, redo


def replay_oi(o64, V, T, a, r, m, env, tab, H, W, max_depth, seed, objects=(), sample=0, closest=None, occluded=None):
    """`path_oi_fp64.replay_oi` where an object may carry "corner_normals" -> (L [H,W,3], record)."""
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
    smooth_of = np.zeros(T.shape[0], bool)
    corner = np.zeros((T.shape[0], 3, 3))
    for ob in objects:
        sl = slice(ob["first_tri"], ob["first_tri"] + ob["n_tri"])
        b = ob["bsdf"]
        if b["type"] == "dielectric":
            kind_of[sl], par[sl] = DIELECTRIC, [b["int_ior"], b["ext_ior"], 0.0]
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
           "smooth_transmitted": z(), "smooth_diffuse": z(), "redo": z(), "fallback": z(), "fallback_cause": np.zeros((N, 3), bool)}

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
        front = ((n * wo).sum(-1) > 0) | (kind == DIELECTRIC)
        alive[idx[~front]] = False
        idx, t, k, n, wo, kind = idx[front], t[front], k[front], n[front], wo[front], kind[front]
        if idx.size == 0:
            continue
        p_all = o[idx] + t[:, None] * d[idx]
        eps_all = 1e-5 * (1 + np.abs(p_all).max(-1))
        # the shading normal: the interpolated corner normal on a smooth object, the face normal everywhere else
        sm = smooth_of[k]
        nsh = n.copy()
        if sm.any():
            bu, bv = barycentrics(P[k[sm]], o[idx[sm]], d[idx[sm]])
            nsh[sm], cause = shading_normal(corner[k[sm]], bu, bv, n[sm], wo[sm])
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
            below = ~((ng * wi).sum(-1) > 0)                       # sampled below the face: the path ends
            thr[ids] *= np.where(below[:, None], 0.0, rho)
            alive[ids[~(thr[ids] > 0).any(-1)]] = False
            prev[ids] = pdf
            prev_delta[ids] = False
            o[ids], d[ids] = po_, wi
            rec["object_vertices"].append({"depth": depth, "pix": ids, "kind": DIFFUSE, "wi": wi, "smooth": sm[sel], "below": below})
        sel = kind == DIELECTRIC
        if sel.any():                                              # ---- glass: a delta vertex, no emitter sample
            ids, ng, ns, p, pr = idx[sel], n[sel], nsh[sel], p_all[sel], par[k[sel]]
            wi, wgt, prob, trans, redo = sample_dielectric_shading(pr[:, 0], pr[:, 1], ng, ns, wo[sel], rng_u(base[ids], depth, 6))
            side = np.where((ng * wi).sum(-1) > 0, 1.0, -1.0)      # spawn on the side the new ray leaves on
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


# ---- meshes and the shared test scene ------------------------------------------------------------------------------------------------
def icosphere(centre, radius, levels):
    """An icosahedron subdivided `levels` times (20 x 4^levels triangles), outward winding -> (V, T, unit radial normals per vertex)."""
    t = (1 + 5 ** 0.5) / 2
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    V = [np.array(v, np.float64) / np.linalg.norm(v) for v in V]
    T = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(levels):
        mid, T2 = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                v = V[i] + V[j]
                V.append(v / np.linalg.norm(v))
                mid[key] = len(V) - 1
            return mid[key]

        for a, b, c in T:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            T2 += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        T = T2
    U = np.array(V)
    return U * radius + np.asarray(centre, np.float64), np.array(T, np.int32), U


GLASS_CENTRE, GLASS_RADIUS = (-0.08, 0.03, -1.15), 0.11
BALL_CENTRE, BALL_RADIUS = (0.10, -0.01, -1.30), 0.10


def table_scene():
    """One table with smooth and flat objects mixed, in front of a depth mesh at z <= -1.6: a smooth glass icosphere and a smooth
    diffuse icosphere of level 1 (80 triangles each; their silhouettes are where the interpolated normal turns away from the viewer
    while the face still looks at it, so the fallbacks and the redo occur) and `path_oi_fp64`'s flat diffuse cube."""
    Vg, Tg, Ng = icosphere(GLASS_CENTRE, GLASS_RADIUS, 1)
    Vb, Tb, Nb = icosphere(BALL_CENTRE, BALL_RADIUS, 1)
    Vd, Td = po.cube((-0.02, -0.13, -1.32), 0.12, (-0.3, 0.7, 0.2))
    return [{"vertices": Vg, "triangles": Tg, "bsdf": po.GLASS, "normals": Ng},
            {"vertices": Vb, "triangles": Tb, "bsdf": po.DIFFUSE_08, "normals": Nb},
            {"vertices": Vd, "triangles": Td, "bsdf": po.DIFFUSE_08}]


def corner_normals(ob):
    """The object's "normals" as the library stores them: normalised in fp64, one per triangle corner, rounded to fp32; None if flat."""
    if ob.get("normals") is None:
        return None
    Nn = np.asarray(ob["normals"], np.float64)
    Nn = Nn / np.linalg.norm(Nn, axis=-1, keepdims=True)
    return Nn[np.asarray(ob["triangles"], np.int64)].astype(np.float32).astype(np.float64)


def merged(V, T, objects):
    """`path_oi_fp64.merged` with each table entry carrying its "corner_normals"."""
    Vm, Tm, table = po.merged(V, T, objects)
    for entry, ob in zip(table, objects):
        entry["corner_normals"] = corner_normals(ob)
    return Vm, Tm, table
