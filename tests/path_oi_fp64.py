"""fp64 restatement of the path render with inserted objects ("Inserted objects"): `path_fp64.replay` with
Mitsuba's smooth `dielectric` and `diffuse` written out in numpy, and the test scene the object tests share.

`replay_oi` walks one sample of every pixel as `path_fp64.replay` does; the depth mesh's vertices run the same statements in the
same order (without objects the two functions return the same bits).  An object is {"first_tri", "n_tri", "bsdf"}: a range of
triangle ids of the merged mesh and PathTracer's bsdf dict.  The record gains, per depth, the object vertices with the event each
took, and per emitter sample whether an inserted object blocked it.

No BVH and no library code; `closest` / `occluded` may be bound to the library's fp32 traversal to tell the paths whose hit
decisions differ between fp32 and fp64."""
import math

import numpy as np

from path_fp64 import FOV, brute, env_texel, mis, pcg, rng_u, texel  # noqa: F401  (pcg: the restated RNG, for callers)

SCENE, DIELECTRIC, DIFFUSE = 0, 1, 2


# ---- the two BSDFs ----------------------------------------------------------------------------------------------------------------
def fresnel(cos_i, eta_it):
    """Exact unpolarised Fresnel reflectance for cos_i = |n . wo| >= 0 and eta_it = n_transmitted / n_incident -> (R, cos_t);
    R = 1 and cos_t = 0 at total internal reflection."""
    cos_t2 = 1.0 - (1.0 - cos_i * cos_i) / (eta_it * eta_it)
    tir = cos_t2 <= 0
    cos_t = np.sqrt(np.where(tir, 0.0, cos_t2))
    with np.errstate(divide="ignore", invalid="ignore"):
        a_s = (cos_i - eta_it * cos_t) / (cos_i + eta_it * cos_t)
        a_p = (cos_t - eta_it * cos_i) / (cos_t + eta_it * cos_i)
    return np.where(tir, 1.0, 0.5 * (a_s * a_s + a_p * a_p)), cos_t


def sample_dielectric(int_ior, ext_ior, n, wo, u):
    """n, wo [N,3], u [N] (dim 6) -> wi, weight [N], probability of the event [N], transmitted [N] bool."""
    eta = int_ior / ext_ior
    cos_o = (n * wo).sum(-1)
    entering = cos_o > 0
    eta_it = np.where(entering, eta, 1.0 / eta)
    eta_ti = 1.0 / eta_it
    ci = np.abs(cos_o)
    R, ct = fresnel(ci, eta_it)
    refl = u <= R
    wi_r = 2.0 * cos_o[:, None] * n - wo
    wi_t = (np.where(entering, 1.0, -1.0) * (eta_ti * ci - ct))[:, None] * n - eta_ti[:, None] * wo
    return (np.where(refl[:, None], wi_r, wi_t), np.where(refl, 1.0, eta_ti * eta_ti), np.where(refl, R, 1.0 - R), ~refl)


def sample_diffuse(n, u0, u1):
    """Cosine-weighted direction about n [N,3] (sin^2 theta = u0, phi = 2 pi u1, the branchless frame of Duff et al. 2017, the one
    the kernel builds) -> wi, pdf = cos / pi."""
    st, ct = np.sqrt(u0), np.sqrt(1.0 - u0)
    x, y = st * np.cos(2 * np.pi * u1), st * np.sin(2 * np.pi * u1)
    sg = np.copysign(1.0, n[:, 2])
    a = -1.0 / (sg + n[:, 2])
    b = n[:, 0] * n[:, 1] * a
    s = np.stack([1.0 + sg * n[:, 0] ** 2 * a, sg * b, -sg * n[:, 0]], -1)
    t = np.stack([b, sg + n[:, 1] ** 2 * a, -n[:, 1]], -1)
    return s * x[:, None] + t * y[:, None] + n * ct[:, None], ct / np.pi


# ---- the walk ----------------------------------------------------------------------------------------------------------------------
def replay_oi(o64, V, T, a, r, m, env, tab, H, W, max_depth, seed, objects=(), sample=0, closest=None, occluded=None):
    """Sample `sample` of every pixel, fp64 -> (L [H,W,3], record).  V, T: the merged mesh (vertices rounded to fp32 as the BVH
    stores them); triangles in no object's range are the depth mesh's."""
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
    for ob in objects:
        sl = slice(ob["first_tri"], ob["first_tri"] + ob["n_tri"])
        b = ob["bsdf"]
        if b["type"] == "dielectric":
            kind_of[sl], par[sl] = DIELECTRIC, [b["int_ior"], b["ext_ior"], 0.0]
        else:
            kind_of[sl], par[sl] = DIFFUSE, np.broadcast_to(np.asarray(b["reflectance"], np.float64), (3,))
    is_obj = kind_of != SCENE
    P_obj = P[is_obj]
    nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    # the depth mesh's normals face the camera; an inserted mesh keeps its winding (outward)
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
    rec = {"H": H, "W": W, "He": He, "We": We, "pixels": pix.astype(np.int64), "full": True, "escapes": [], "vertices": [],
           "object_vertices": [], "transmitted": np.zeros(N, bool), "diffuse_object": np.zeros(N, bool),
           "blocked_by_object": np.zeros(N, bool)}

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

    def shadow(idx, ok, po, wl):
        """visibility of the emitter samples `ok`; notes the pixels an inserted object shadows"""
        vis = np.zeros(idx.size, bool)
        if ok.any():
            vis[np.nonzero(ok)[0]] = ~occluded(po[ok], wl[ok])
            if P_obj.shape[0]:
                rec["blocked_by_object"][idx[ok][np.isfinite(brute(P_obj, po[ok], wl[ok])[0])]] = True
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
            # after a delta vertex no emitter sample competed: weight 1 (Mitsuba's prev_bsdf_delta)
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
        front = ((n * wo).sum(-1) > 0) | (kind == DIELECTRIC)      # glass shades from both sides; everything else is one-sided
        alive[idx[~front]] = False
        idx, t, k, n, wo, kind = idx[front], t[front], k[front], n[front], wo[front], kind[front]
        if idx.size == 0:
            continue
        p_all = o[idx] + t[:, None] * d[idx]
        eps_all = 1e-5 * (1 + np.abs(p_all).max(-1))
        sel = kind == SCENE
        if sel.any():                                              # ---- the depth mesh: path_fp64.replay's statements
            ids, ns, wos, p = idx[sel], n[sel], wo[sel], p_all[sel]
            tp = texel(o64, p, H, W)
            av, rv, mv = A[tp], R[tp], M[tp]
            po = p + (1e-5 * (1 + np.abs(p).max(-1)))[:, None] * ns
            b = base[ids]
            vert = {"depth": depth, "pix": ids, "tp": tp, "wo": wos, "n": ns, "em": np.zeros(ids.size, bool), "wl": np.zeros((ids.size, 3)),
                    "te": np.zeros(ids.size, np.int64), "we": np.zeros(ids.size)}
            if have_tab:
                wl, te, pe = emitter(b, depth)
                fb, pb = o64.eval_brdf(wl, wos, ns, av, rv, mv)
                ok = (pe > 0) & ((ns * wl).sum(-1) > 0) & (fb > 0).any(-1)
                if ok.any():
                    vis = shadow(ids, ok, po, wl)
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
            o[ids], d[ids] = po, wi
        sel = kind == DIFFUSE
        if sel.any():                                              # ---- a diffuse object: f cos = rho / pi max(n . wi, 0)
            ids, ns, p, rho = idx[sel], n[sel], p_all[sel], par[k[sel]]
            po = p + eps_all[sel][:, None] * ns
            b = base[ids]
            rec["diffuse_object"][ids] = True
            if have_tab:
                wl, te, pe = emitter(b, depth)
                c = np.maximum((ns * wl).sum(-1), 0.0)
                fb, pb = rho * (c / np.pi)[:, None], c / np.pi
                ok = (pe > 0) & (c > 0) & (fb > 0).any(-1)
                vis = shadow(ids, ok, po, wl)
                w = np.where(vis, mis(pe, pb) / np.where(pe > 0, pe, 1.0), 0.0)
                L[ids] += thr[ids] * fb * envf[te] * w[:, None]
            wi, pdf = sample_diffuse(ns, rng_u(b, depth, 7), rng_u(b, depth, 8))
            thr[ids] *= rho
            alive[ids[~(thr[ids] > 0).any(-1)]] = False
            prev[ids] = pdf
            prev_delta[ids] = False
            o[ids], d[ids] = po, wi
            rec["object_vertices"].append({"depth": depth, "pix": ids, "kind": DIFFUSE, "wi": wi})
        sel = kind == DIELECTRIC
        if sel.any():                                              # ---- glass: a delta vertex, no emitter sample
            ids, ns, p, pr = idx[sel], n[sel], p_all[sel], par[k[sel]]
            wi, wgt, prob, trans = sample_dielectric(pr[:, 0], pr[:, 1], ns, wo[sel], rng_u(base[ids], depth, 6))
            side = np.where((ns * wi).sum(-1) > 0, 1.0, -1.0)      # spawn on the side the new ray leaves on
            thr[ids] *= wgt[:, None]
            prev[ids] = prob
            prev_delta[ids] = True
            o[ids], d[ids] = p + (side * eps_all[sel])[:, None] * ns, wi
            rec["transmitted"][ids[trans]] = True
            rec["object_vertices"].append({"depth": depth, "pix": ids, "kind": DIELECTRIC, "wi": wi, "transmitted": trans})
    return L.reshape(H, W, 3), rec


# ---- the shared test scene ---------------------------------------------------------------------------------------------------------
def cube(centre, side, angles):
    """12 triangles, outward winding, rotated by `angles` (radians about x, y, z in turn) about its centre -> (V [8,3], T [12,3])."""
    c = np.array([[x, y, z] for z in (-0.5, 0.5) for y in (-0.5, 0.5) for x in (-0.5, 0.5)], np.float64) * side
    ax, ay, az = angles
    Rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
    Ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    Rz = np.array([[math.cos(az), -math.sin(az), 0], [math.sin(az), math.cos(az), 0], [0, 0, 1]])
    V = c @ (Rz @ Ry @ Rx).T + np.asarray(centre, np.float64)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]   # -z +z -y +y -x +x, seen from outside
    T = np.array([t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))], np.int32)
    return V, T


GLASS = {"type": "dielectric", "int_ior": 1.49, "ext_ior": 1.000277}
DIFFUSE_08 = {"type": "diffuse", "reflectance": (0.8, 0.8, 0.8)}


def two_cubes():
    """A glass and a diffuse cube, neither aligned with an axis, in front of a depth mesh at z <= -1.6: together they cover the
    image centre, the diffuse one partly behind the glass one, and each casts a shadow on the mesh behind."""
    Vg, Tg = cube((-0.05, 0.02, -1.15), 0.22, (0.4, 0.5, 0.3))
    Vd, Td = cube((0.10, -0.04, -1.40), 0.20, (-0.3, 0.7, 0.2))
    return [{"vertices": Vg, "triangles": Tg, "bsdf": GLASS}, {"vertices": Vd, "triangles": Td, "bsdf": DIFFUSE_08}]


def merged(V, T, objects):
    """The depth mesh with the objects appended, as PathTracer merges them -> (V fp32-rounded float64, T, [replay_oi objects])."""
    Vs, Ts, table = [np.asarray(V, np.float64)], [np.asarray(T, np.int64)], []
    nv, nt = Vs[0].shape[0], Ts[0].shape[0]
    for ob in objects:
        Vs.append(np.asarray(ob["vertices"], np.float64))
        Ts.append(np.asarray(ob["triangles"], np.int64) + nv)
        table.append({"first_tri": nt, "n_tri": len(ob["triangles"]), "bsdf": ob["bsdf"]})
        nv, nt = nv + len(ob["vertices"]), nt + len(ob["triangles"])
    return np.concatenate(Vs).astype(np.float32).astype(np.float64), np.concatenate(Ts).astype(np.int32), table
