"""fp64 restatement of the path render with emissive inserted objects ("Emissive inserted objects"):
`path_oi_pbr_fp64.replay_oi` with a fourth object kind, {"type": "area", "radiance": scalar or 3 values}, an area light.

  * The emitters of a scene: the envmap where it has tables, then the area objects in table order; n_e is their count.
  * Emitter sample at a non-delta vertex (dims 2-5): idx = min(int(u2 n_e), n_e - 1), u2' = u2 n_e - idx kept below 1 (both formed
    in fp32, as the kernel forms them: they are sampling decisions, like the fp32 tables); the envmap by (u2', u3, u4, u5) with
    pdf_e / n_e; light l by the first triangle whose cumulative area (fp64 sums stored fp32, the last exactly 1) exceeds u2', the
    point y = v0 + (1 - s) e1 + s u4 e2 with s = sqrt(1 - u3), wl = normalize(y - po), dist = |y - po|,
    pdf = dist^2 / (A cos_l n_e); the sample needs cos_l = n_l . (-wl) > 0, ng . wl > 0, dist > 0; the shadow ray reaches
    dist (1 - 1e-3); it adds thr f p mis(pdf, pdf_b) / pdf with f, pdf_b from the vertex's BSDF.
  * A traced ray that lands on a light: on its front (ng . wo > 0) it adds thr p w, w = 1 at depth 0 or after a delta vertex, else
    mis(prev_pdf, t^2 / (A (ng . wo) n_e)), BEFORE the max_depth test; front or back, the path ends.
  * An escaped ray's weight takes env_pdf / n_e.

Every other statement is `path_oi_pbr_fp64.replay_oi`'s (without an area object the two functions return the same bits).  Radiance and
area are rounded to fp32, as the library holds them.  No library code: the default intersection is `path_fp64.brute`.

The record gains, per pixel: `light_sample_arrives`, `light_sample_blocked` (a light sample whose shadow ray an object or the mesh
stops), `bsdf_hits_light_front` / `bsdf_hits_light_back` (a ray sampled at a non-delta vertex), `light_through_glass` (a front hit
after a delta vertex), `light_at_depth0`, `env_sample` (an envmap emitter sample taken while lights compete)."""
import math

import numpy as np

import path_oi_fp64 as po
import path_oi_pbr_fp64 as pp
import path_oi_smooth_fp64 as ps
from path_fp64 import FOV, brute, env_texel, mis, pcg, rng_u, texel

SCENE, DIELECTRIC, DIFFUSE, PBR, AREA = po.SCENE, po.DIELECTRIC, po.DIFFUSE, pp.PBR, 4
SHADOW_EPS = 1e-3
BELOW_ONE = np.float32(1.0 - 2.0 ** -24)


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def light_table(P):
    """One light's triangles P [n,3,3] -> (areas fp64 [n], A as fp32, cdf fp32 [n]: cumulative / total, from the last triangle of
    positive area on exactly 1)."""
    a = 0.5 * np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=-1)
    A = math.fsum(a)
    cdf = np.minimum((np.cumsum(a) / A).astype(np.float32), np.float32(1.0))
    cdf[np.nonzero(a > 0)[0][-1]:] = 1.0
    return a, float(np.float32(A)), cdf


def choose(u2, n_e):
    """The emitter by sample reuse, in fp32 -> (idx, u2')."""
    x = u2.astype(np.float32) * np.float32(n_e)
    idx = np.minimum(x.astype(np.int64), n_e - 1)
    return idx, np.minimum(x - idx.astype(np.float32), BELOW_ONE).astype(np.float64)


def sample_light(P, A, cdf, u_tri, u3, u4, po_, n_e):
    """Points of one light seen from po_ [N,3] -> (triangle [N], y, wl, dist, pdf: 0 where the light faces away or dist = 0)."""
    t = np.searchsorted(cdf, u_tri.astype(np.float32), side="right")        # the first entry > u
    v0, e1, e2 = P[t, 0], P[t, 1] - P[t, 0], P[t, 2] - P[t, 0]
    s = np.sqrt(np.maximum(1 - u3, 0))
    y = v0 + (1 - s)[:, None] * e1 + (s * u4)[:, None] * e2
    dv = y - po_
    dist = np.linalg.norm(dv, axis=-1)
    wl = dv / np.where(dist > 0, dist, 1.0)[:, None]
    nl = np.cross(e1, e2)
    nl /= np.maximum(np.linalg.norm(nl, axis=-1, keepdims=True), 1e-300)
    cos_l = -(nl * wl).sum(-1)
    ok = (cos_l > 0) & (dist > 0)
    pdf = np.where(ok, dist * dist / np.where(ok, A * cos_l * n_e, 1.0), 0.0)
    return t, y, wl, dist, pdf


def replay_lights(o64, V, T, a, r, m, env, tab, H, W, max_depth, seed, objects=(), sample=0, closest=None, lanes=None):
    """`path_oi_pbr_fp64.replay_oi` where an object's bsdf may be of type "area" -> (L [H,W,3], record).  `closest(o, d)` -> (t,
    index): the intersection routine (default `brute`); a shadow ray is occluded where its closest hit lies nearer than its reach.
    `lanes` = (pixel [N], seed [N], sample [N]): these samples in one walk instead of one sample of every pixel -> L [N,3] (the
    record's entries are per lane then)."""
    He, We = env.shape[:2]
    envf = env.reshape(-1, 3).astype(np.float64)
    pdf_tab = tab["pdf"].reshape(-1).astype(np.float64)
    row_cdf, col_cdf = tab["row_cdf"], tab["col_cdf"]
    have_tab = bool(tab["row_cdf"][-1] > 0)
    P = V[T]
    if closest is None:
        closest = lambda o, d: brute(P, o, d)
    kind_of = np.zeros(T.shape[0], np.int64)
    par = np.zeros((T.shape[0], 3))
    mat = np.zeros((T.shape[0], 5))
    smooth_of = np.zeros(T.shape[0], bool)
    corner = np.zeros((T.shape[0], 3, 3))
    area_of = np.zeros(T.shape[0])
    lights = []                                                    # per light: (P, A, cdf, radiance)
    for ob in objects:
        sl = slice(ob["first_tri"], ob["first_tri"] + ob["n_tri"])
        b = ob["bsdf"]
        if b["type"] == "dielectric":
            kind_of[sl], par[sl] = DIELECTRIC, [b["int_ior"], b["ext_ior"], 0.0]
        elif b["type"] == "pbr":
            ca, cr, cm = pp.pbr_constants(b)
            kind_of[sl], mat[sl] = PBR, [*ca, cr, cm]
        elif b["type"] == "area":
            rad = np.broadcast_to(f32(b.get("radiance", 1.0)), (3,))
            _, A, cdf = light_table(P[sl])
            kind_of[sl], par[sl], area_of[sl] = AREA, rad, A
            lights.append((P[sl], A, cdf, rad))
        else:
            kind_of[sl], par[sl] = DIFFUSE, np.broadcast_to(np.asarray(b["reflectance"], np.float64), (3,))
        if ob.get("corner_normals") is not None:
            assert b["type"] != "area", "an area light has no shading normals"
            smooth_of[sl], corner[sl] = True, np.asarray(ob["corner_normals"], np.float64)
    n_e = int(have_tab) + len(lights)
    is_obj = kind_of != SCENE
    P_obj = P[is_obj]
    nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    nrm *= np.where(((nrm * P[:, 0]).sum(-1, keepdims=True) > 0) & ~is_obj[:, None], -1.0, 1.0)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=-1, keepdims=True), 1e-300)
    if lanes is None:
        pix = np.arange(H * W, dtype=np.uint32)
        base = pcg(pcg(pcg(np.uint32(seed)) + pix) + np.uint32(sample))
    else:
        pix = np.asarray(lanes[0], dtype=np.uint32)
        base = pcg(pcg(pcg(np.asarray(lanes[1], dtype=np.uint32)) + pix) + np.asarray(lanes[2], dtype=np.uint32))
    N = pix.size
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
    A_, R_, M_ = a.reshape(-1, 3).astype(np.float64), r.reshape(-1).astype(np.float64), m.reshape(-1).astype(np.float64)
    z = lambda: np.zeros(N, bool)
    rec = {"H": H, "W": W, "n_e": n_e, "transmitted": z(), "diffuse_object": z(), "blocked_by_object": z(), "fallback": z(),
           "pbr_vertex": z(), "light_sample_arrives": z(), "light_sample_blocked": z(), "bsdf_hits_light_front": z(),
           "bsdf_hits_light_back": z(), "light_through_glass": z(), "light_at_depth0": z(), "env_sample": z()}

    def emitter(ids, b, depth, po_):
        """One emitter sample per lane -> (wl, radiance [n,3], pdf with its 1 / n_e, the shadow ray's reach, from a light)."""
        u2, u3, u4, u5 = (rng_u(b, depth, c) for c in (2, 3, 4, 5))
        n = ids.size
        idx, u_re = choose(u2, n_e)
        wl, Le, pe, reach, lit = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n), np.full(n, np.inf), np.zeros(n, bool)
        if have_tab:
            e = idx == 0
            if e.any():
                row = np.searchsorted(row_cdf[:He], u_re[e], side="right") - 1
                col = np.array([np.searchsorted(col_cdf[rr, :We], uu, side="right") - 1 for rr, uu in zip(row, u3[e])], dtype=np.int64)
                c0, c1 = np.cos(row * np.pi / He), np.cos((row + 1) * np.pi / He)
                ct = c0 + (c1 - c0) * u4[e]
                st = np.sqrt(np.maximum(1 - ct * ct, 0))
                ph = (col + u5[e]) * 2 * np.pi / We
                wl[e] = np.stack([st * np.sin(ph), ct, -st * np.cos(ph)], -1)
                te = row * We + col
                Le[e], pe[e] = envf[te], pdf_tab[te] / n_e
                if lights:
                    rec["env_sample"][ids[e]] = True
        for l, (Pl, A, cdf, rad) in enumerate(lights):
            e = idx == l + int(have_tab)
            if e.any():
                _, _, wl[e], dist, pe[e] = sample_light(Pl, A, cdf, u_re[e], u3[e], u4[e], po_[e], n_e)
                Le[e], reach[e], lit[e] = rad, dist * (1 - SHADOW_EPS), True
        return wl, Le, pe, reach, lit

    def emitter_term(ids, b, depth, po_, ng, eval_f):
        """The emitter sample of a non-delta vertex added to L; eval_f(wl) -> (f with its cosine, pdf_b)."""
        if n_e == 0:
            return
        wl, Le, pe, reach, lit = emitter(ids, b, depth, po_)
        fb, pb = eval_f(wl)
        ok = (pe > 0) & ((ng * wl).sum(-1) > 0) & (fb > 0).any(-1)
        vis = np.zeros(ids.size, bool)
        if ok.any():
            q = np.nonzero(ok)[0]
            vis[q] = ~(closest(po_[ok], wl[ok])[0] < reach[ok])
            if P_obj.shape[0]:
                rec["blocked_by_object"][ids[q[brute(P_obj, po_[ok], wl[ok])[0] < reach[ok]]]] = True
        w = np.where(vis, mis(pe, pb) / np.where(pe > 0, pe, 1.0), 0.0)
        L[ids] += thr[ids] * fb * Le * w[:, None]
        rec["light_sample_arrives"][ids[vis & lit & (Le > 0).any(-1)]] = True
        rec["light_sample_blocked"][ids[ok & ~vis & lit]] = True

    for depth in range(max_depth + 1):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        t, k = closest(o[idx], d[idx])
        miss = k < 0
        im = idx[miss]
        if im.size:
            tx = env_texel(d[im], He, We)
            w = np.ones(im.size) if depth == 0 else np.where(prev_delta[im], 1.0, mis(prev[im], pdf_tab[tx] / n_e if have_tab else 0.0))
            L[im] += thr[im] * envf[tx] * w[:, None]
        alive[im] = False
        idx, t, k = idx[~miss], t[~miss], k[~miss]
        lit = kind_of[k] == AREA                                   # ---- a light: its emission before the max_depth test
        if lit.any():
            il, tl, kl = idx[lit], t[lit], k[lit]
            cos_o = -(nrm[kl] * d[il]).sum(-1)
            front = cos_o > 0
            unweighted = np.full(il.size, depth == 0) | prev_delta[il]
            pdf_l = tl * tl / np.where(front, area_of[kl] * cos_o * n_e, 1.0)
            w = np.where(unweighted, 1.0, mis(prev[il], pdf_l))
            L[il] += np.where(front[:, None], thr[il] * par[kl] * w[:, None], 0.0)
            alive[il] = False
            if depth == 0:
                rec["light_at_depth0"][il[front]] = True
            else:
                rec["light_through_glass"][il[front & prev_delta[il]]] = True
                rec["bsdf_hits_light_front"][il[front & ~prev_delta[il]]] = True
                rec["bsdf_hits_light_back"][il[~front & ~prev_delta[il]]] = True
            idx, t, k = idx[~lit], t[~lit], k[~lit]
        if depth + 1 >= max_depth:
            alive[:] = False
            break
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
        sm = smooth_of[k]
        nsh = n.copy()
        if sm.any():
            bu, bv = ps.barycentrics(P[k[sm]], o[idx[sm]], d[idx[sm]])
            nsh[sm], cause = ps.shading_normal(corner[k[sm]], bu, bv, n[sm], wo[sm])
            rec["fallback"][idx[sm]] |= cause.any(-1)
        sel = kind == SCENE
        if sel.any():                                              # ---- the depth mesh
            ids, ns, wos, p = idx[sel], n[sel], wo[sel], p_all[sel]
            tp = texel(o64, p, H, W)
            av, rv, mv = A_[tp], R_[tp], M_[tp]
            po_ = p + (1e-5 * (1 + np.abs(p).max(-1)))[:, None] * ns
            b = base[ids]
            emitter_term(ids, b, depth, po_, ns, lambda wl: o64.eval_brdf(wl, wos, ns, av, rv, mv))
            s1, s2a, s2b = (rng_u(b, depth, c) for c in (6, 7, 8))
            wi, pdf, wgt = o64.sample_brdf(s1, np.stack([s2a, s2b], -1), wos, ns, av, rv, mv)
            thr[ids] *= wgt
            alive[ids[~(thr[ids] > 0).any(-1)]] = False
            prev[ids] = pdf
            prev_delta[ids] = False
            o[ids], d[ids] = po_, wi
        sel = kind == PBR
        if sel.any():                                              # ---- a PBR object
            ids, ng, ns, wos, p = idx[sel], n[sel], nsh[sel], wo[sel], p_all[sel]
            cm = mat[k[sel]]
            av, rv, mv = cm[:, :3], cm[:, 3], cm[:, 4]
            po_ = p + eps_all[sel][:, None] * ng
            b = base[ids]
            rec["pbr_vertex"][ids] = True
            emitter_term(ids, b, depth, po_, ng, lambda wl: o64.eval_brdf(wl, wos, ns, av, rv, mv))
            s1, s2a, s2b = (rng_u(b, depth, c) for c in (6, 7, 8))
            wi, pdf, wgt = o64.sample_brdf(s1, np.stack([s2a, s2b], -1), wos, ns, av, rv, mv)
            below = ~((ng * wi).sum(-1) > 0)
            thr[ids] *= wgt
            alive[ids[~(thr[ids] > 0).any(-1) | below]] = False
            prev[ids] = pdf
            prev_delta[ids] = False
            o[ids], d[ids] = po_, wi
        sel = kind == DIFFUSE
        if sel.any():                                              # ---- a diffuse object
            ids, ng, ns, p, rho = idx[sel], n[sel], nsh[sel], p_all[sel], par[k[sel]]
            po_ = p + eps_all[sel][:, None] * ng
            b = base[ids]
            rec["diffuse_object"][ids] = True

            def lambert(wl):
                c = np.maximum((ns * wl).sum(-1), 0.0)
                return rho * (c / np.pi)[:, None], c / np.pi

            emitter_term(ids, b, depth, po_, ng, lambert)
            wi, pdf = po.sample_diffuse(ns, rng_u(b, depth, 7), rng_u(b, depth, 8))
            below = ~((ng * wi).sum(-1) > 0)
            thr[ids] *= np.where(below[:, None], 0.0, rho)
            alive[ids[~(thr[ids] > 0).any(-1)]] = False
            prev[ids] = pdf
            prev_delta[ids] = False
            o[ids], d[ids] = po_, wi
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
    return (L.reshape(H, W, 3) if lanes is None else L), rec


def replay_mean(H, W, spp, seeds, max_depth, V, T, env, tab, objects, chunk=4):
    """The spp-sample estimate of every pixel for each seed, over a depth mesh that no ray meets (no maps, no oracle) ->
    [len(seeds), H, W, 3]; `chunk` seeds per walk."""
    maps = (np.zeros((H, W, 3), np.float32), np.ones((H, W, 1), np.float32), np.zeros((H, W, 1), np.float32))
    out = np.zeros((len(seeds), H, W, 3))
    pix, smp = np.meshgrid(np.arange(H * W), np.arange(spp), indexing="ij")
    for c0 in range(0, len(seeds), chunk):
        sd = np.asarray(seeds[c0:c0 + chunk])
        lanes = (np.tile(pix.reshape(-1), sd.size), np.repeat(sd, pix.size), np.tile(smp.reshape(-1), sd.size))
        L, _ = replay_lights(None, V, T, *maps, env, tab, H, W, max_depth, 0, objects, lanes=lanes)
        out[c0:c0 + sd.size] = L.reshape(sd.size, H, W, spp, 3).mean(3)
    return out


# ---- the shared test scenes ----------------------------------------------------------------------------------------------------------
def rotation(angles):
    """`path_oi_fp64.cube`'s rotation: radians about x, y, z in turn."""
    ax, ay, az = angles
    Rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
    Ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    Rz = np.array([[math.cos(az), -math.sin(az), 0], [math.sin(az), math.cos(az), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def box(centre, sides, angles=(0.0, 0.0, 0.0), inward=False):
    """A box of unequal sides (12 triangles, three distinct areas), `path_oi_fp64.cube` scaled per axis; `inward`: wound so that its
    faces look into it -> (V [8,3], T [12,3])."""
    V, T = po.cube((0.0, 0.0, 0.0), 1.0, (0.0, 0.0, 0.0))
    V = (V * np.asarray(sides, np.float64)) @ rotation(angles).T + np.asarray(centre, np.float64)
    return V, (T[:, ::-1].copy() if inward else T)


def quad(corners):
    """Two triangles over four corners in order; e1 x e2 follows the right-hand rule of that order -> (V [4,3], T [2,3])."""
    return np.asarray(corners, np.float64), np.array([[0, 1, 2], [0, 2, 3]], np.int32)


BOX_LIGHT = {"type": "area", "radiance": (6.0, 5.0, 4.0)}
QUAD_LIGHT = {"type": "area", "radiance": (25.0, 24.0, 20.0)}
LIGHT_BOX = ((0.08, 0.13, -1.30), (0.26, 0.22, 0.08), (0.1, -0.2, 0.1))
LIGHT_QUAD = [[-0.0366, -0.05, -1.328], [0.0474, -0.05, -1.216], [0.0474, -0.19, -1.216], [-0.0366, -0.19, -1.328]]   # front (0.8, 0, -0.6): the groove's right wall, the PBR cube; back: the diffuse cube, the camera
GLASS_CENTRE, GLASS_RADIUS = (0.08, 0.12, -1.10), 0.09
PBR_CUBE = ((0.13, -0.12, -1.36), 0.14, (0.0, 0.5, 0.0))
DIFFUSE_CUBE = ((-0.10, -0.12, -1.30), 0.14, (0.0, -0.5, 0.0))


def table_scene():
    """The GPU parity scene's table, in front of a depth mesh at z <= -1.6: the unequal-sided emitter box, a single emitter quad
    facing the groove and the objects, a smooth glass icosphere, a flat PBR cube and a diffuse cube."""
    Vb, Tb = box(*LIGHT_BOX)
    Vq, Tq = quad(LIGHT_QUAD)
    Vg, Tg, Ng = ps.icosphere(GLASS_CENTRE, GLASS_RADIUS, 1)
    Vc, Tc = po.cube(*PBR_CUBE)
    Vd, Td = po.cube(*DIFFUSE_CUBE)
    return [{"vertices": Vb, "triangles": Tb, "bsdf": BOX_LIGHT},
            {"vertices": Vq, "triangles": Tq, "bsdf": QUAD_LIGHT},
            {"vertices": Vg, "triangles": Tg, "bsdf": po.GLASS, "normals": Ng},
            {"vertices": Vc, "triangles": Tc, "bsdf": pp.PLASTIC},
            {"vertices": Vd, "triangles": Td, "bsdf": po.DIFFUSE_08}]


merged = ps.merged
RECORD_KEYS = ("light_sample_arrives", "light_sample_blocked", "bsdf_hits_light_front", "bsdf_hits_light_back", "light_through_glass",
               "light_at_depth0")


# ---- closed forms ------------------------------------------------------------------------------------------------------------------------
def lambert_irradiance(x, n, poly):
    """Lambert's polygon formula: the irradiance at points x [N,3] (normal n) from a polygon of unit radiance, corners `poly` [k,3]
    in order, the whole polygon above the horizon of n: E = 1/2 |sum_i acos(v_i . v_i+1) (v_i x v_i+1) / |v_i x v_i+1| . n| (the
    sign is the winding's)."""
    v = np.asarray(poly, np.float64)[None] - np.asarray(x, np.float64)[:, None]
    v /= np.linalg.norm(v, axis=-1, keepdims=True)
    E = np.zeros(v.shape[0])
    for i in range(v.shape[1]):
        a, b = v[:, i], v[:, (i + 1) % v.shape[1]]
        c = np.cross(a, b)
        E += np.arccos(np.clip((a * b).sum(-1), -1, 1)) * ((c / np.linalg.norm(c, axis=-1, keepdims=True)) @ np.asarray(n, np.float64))
    return np.abs(0.5 * E)


FLOOR_Y, FLOOR_RHO = -0.25, (0.7, 0.5, 0.3)
FLOOR = [[-3.0, FLOOR_Y, -0.2], [3.0, FLOOR_Y, -0.2], [3.0, FLOOR_Y, -6.0], [-3.0, FLOOR_Y, -6.0]]       # faces +y
LAMP = [[-0.3, 0.2, -2.2], [0.3, 0.2, -2.2], [0.3, 0.2, -1.6], [-0.3, 0.2, -1.6]]                        # faces -y
LAMP_RADIANCE = (3.0, 2.5, 2.0)


def lambert_scene():
    """Closed form (a): a diffuse floor quad under a downward-facing emitter quad; the depth mesh is `FAR_TRIANGLE`."""
    Vf, Tf = quad(FLOOR)
    Vl, Tl = quad(LAMP)
    return [{"vertices": Vf, "triangles": Tf, "bsdf": {"type": "diffuse", "reflectance": FLOOR_RHO}},
            {"vertices": Vl, "triangles": Tl, "bsdf": {"type": "area", "radiance": LAMP_RADIANCE}}]


def lambert_expected(H, W, n=8):
    """Per pixel: rho / pi L E averaged over the pixel's footprint with an n x n midpoint rule, where the whole footprint (the
    midpoints and a 9 x 9 grid with its border) sees the floor and not the lamp -> (expected [H,W,3], covered [H,W])."""
    f = (W / 2.0) / math.tan(math.radians(FOV) / 2.0)
    lamp, rho, rad = np.asarray(LAMP), np.asarray(FLOOR_RHO), f32(LAMP_RADIANCE)
    lamp_P = lamp[np.array([[0, 1, 2], [0, 2, 3]])]

    def floor_points(g):
        yy, xx = np.meshgrid((np.arange(H)[:, None] + g[None]).reshape(-1), (np.arange(W)[:, None] + g[None]).reshape(-1), indexing="ij")
        d = np.stack([(xx - (W - 1) / 2) / f, -(yy - (H - 1) / 2) / f, -np.ones_like(xx)], -1).reshape(-1, 3)
        t = np.where(d[:, 1] < 0, FLOOR_Y / np.where(d[:, 1] < 0, d[:, 1], -1.0), -1.0)
        x = t[:, None] * d
        on = (t > 0) & (np.abs(x[:, 0]) < 3) & (x[:, 2] < -0.2) & (x[:, 2] > -6)
        on &= ~np.isfinite(brute(lamp_P, np.zeros_like(d), d / np.linalg.norm(d, axis=-1, keepdims=True))[0])
        return x, on.reshape(H, g.size, W, g.size)

    _, on_b = floor_points(np.linspace(-0.5, 0.5, 9))
    x, on_m = floor_points((np.arange(n) + 0.5) / n - 0.5)
    cov = on_b.all(axis=(1, 3)) & on_m.all(axis=(1, 3))
    E = np.where(on_m.reshape(-1), lambert_irradiance(x, (0.0, 1.0, 0.0), lamp), 0.0).reshape(H, n, W, n).mean(axis=(1, 3))
    return np.where(cov[..., None], rho / math.pi * rad * E[..., None], 0.0), cov


FURNACE_L = 0.8
FURNACE_BOX = ((0.0, 0.0, -0.5), (3.0, 2.4, 4.0))
FURNACE_RHO = (0.75, 0.5, 0.25)


def furnace_scene(inner):
    """Closed form (b): a closed box whose faces emit FURNACE_L inwards, around the camera and `inner` ("diffuse": a convex diffuse
    cube of reflectance FURNACE_RHO, which shows rho L at max_depth 2; "glass": a smooth glass icosphere, which shows L)."""
    Vb, Tb = box(*FURNACE_BOX, inward=True)
    if inner == "diffuse":
        Vi, Ti = po.cube((0.02, -0.01, -1.2), 0.3, (0.4, 0.5, 0.3))
        ob = {"vertices": Vi, "triangles": Ti, "bsdf": {"type": "diffuse", "reflectance": FURNACE_RHO}}
    else:
        Vi, Ti, Ni = ps.icosphere((0.02, -0.01, -1.2), 0.2, 1)
        ob = {"vertices": Vi, "triangles": Ti, "bsdf": po.GLASS, "normals": Ni}
    return [{"vertices": Vb, "triangles": Tb, "bsdf": {"type": "area", "radiance": FURNACE_L}}, ob]


def within_five_sigma(values, expected, covered):
    """The closed forms' statistic: `values` [S,H,W,3] are S seed-level estimates; every covered pixel's mean lies within 5 standard
    errors (estimated from the S values) of `expected` plus 1e-3 relative -> (ok, the worst excess in units of the bound)."""
    mean = values.mean(0)
    se = values.std(0, ddof=1) / math.sqrt(values.shape[0])
    bound = 5 * se + 1e-3 * np.abs(expected)
    excess = (np.abs(mean - expected) / np.maximum(bound, 1e-300))[covered]
    return bool((excess <= 1.0).all()), float(excess.max()) if excess.size else 0.0
