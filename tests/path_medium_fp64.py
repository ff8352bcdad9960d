"""fp64 restatement of the path render with media inside glass objects ("Media inside glass"): a walk of its
own beside `path_objects_fp64.replay_objects`, built from the samplers the feature modules export.  It covers the depth mesh's
vertices and objects of kinds 1 (dielectric), 2 (diffuse), 4 (area) and 5 (roughdielectric), flat or smooth; on a table without a
medium it runs `replay_objects`' statements in their order and returns its bits.

The medium rule.  A dielectric or roughdielectric table entry may carry "medium" = (sigma_a [3], sigma_s, g), rounded to fp32 as the
library's record is (`medium_record`).  The path carries `med`, an object index or -1 (-1 at the camera).  After the BSDF sample at a
vertex on an object with a medium, med = that object where ng . wi < 0 (ng the outward face normal), else -1; a vertex on anything
else leaves med alone.  A ray that escapes with med >= 0 takes the envmap unattenuated.  A segment with med >= 0 whose trace hit at t:
where sigma_s > 0, s = -log(1 - u9) / sigma_s and, where s < t, the depth is a medium vertex at o + s d: thr *= exp(-sigma_a s), the
max_depth test, no emitter sample, the new direction from Henyey-Greenstein about d by dims 10, 11 (`phase_sample`) with weight 1,
no spawn offset, med unchanged, and the next hit or escape takes MIS weight 1.  Otherwise thr *= exp(-sigma_a t) and the surface
vertex runs as without a medium.

The record holds `replay_objects`' keys for these kinds and, per pixel (or lane): `absorbed_segment` (a segment inside a medium that
reached its hit), `medium_vertex`, `scatter_then_exit` (a path that left its medium through the boundary after a medium vertex),
`cut_inside_medium` (max_depth ended the path at a medium vertex), `light_hit_from_medium` (a ray that left a medium vertex landed
on a light's front)."""
import math

import numpy as np

import path_light_fp64 as pl
import path_oi_fp64 as po
import path_oi_smooth_fp64 as ps
from path_fp64 import FOV, brute, env_texel, mis, pcg, rng_u, texel
from path_rough_fp64 import AREA, DIELECTRIC, DIFFUSE, ROUGH, SCENE, f32, rough_eval, rough_params, rough_sample

RECORD_KEYS = ("absorbed_segment", "medium_vertex", "scatter_then_exit", "cut_inside_medium", "light_hit_from_medium")
FLAGS = ("transmitted", "diffuse_object", "blocked_by_object", "smooth_transmitted", "smooth_diffuse", "redo", "fallback",
         "light_sample_arrives", "light_sample_blocked", "bsdf_hits_light_front", "bsdf_hits_light_back", "light_through_glass",
         "light_at_depth0", "env_sample", "rough_reflected", "rough_transmitted", "rough_emitter_reflection_side",
         "rough_emitter_blocked_inside", "rough_bsdf_hits_light", "rough_killed_by_normals") + RECORD_KEYS
G_ISOTROPIC = 1e-3                                                 # below it the phase function is sampled as the isotropic one


def medium_record(medium):
    """A bsdf's "medium" dict (either form) -> (sigma_a [3], sigma_s, g), each rounded to fp32 as the library's record is; None
    without one."""
    if medium is None:
        return None
    if "color" in medium:
        sa = -np.log(np.broadcast_to(np.asarray(medium["color"], np.float64), (3,))) / float(medium["at"])
    else:
        sa = np.broadcast_to(np.asarray(medium.get("sigma_a", 0.0), np.float64), (3,))
    return f32(sa).astype(np.float64) + 0.0, float(f32(medium.get("scatter", 0.0))), float(f32(medium.get("g", 0.0)))


def flight(sigma_s, u):
    """The free flight of a medium with sigma_s > 0."""
    return -np.log1p(-np.asarray(u, np.float64)) / sigma_s


def phase_cos(g, u):
    """The cosine of Henyey-Greenstein's angle to the propagation direction, by inversion; isotropic below |g| = 1e-3."""
    u = np.asarray(u, np.float64)
    if abs(g) < G_ISOTROPIC:
        return 1.0 - 2.0 * u
    q = (1.0 - g * g) / (1.0 - g + 2.0 * g * u)
    return np.clip((1.0 + g * g - q * q) / (2.0 * g), -1.0, 1.0)


def phase_sample(g, d, u0, u1):
    """wi about the unit direction d: the cosine by `phase_cos`, phi = 2 pi u1, the frame of Duff et al. 2017 (`sample_diffuse`'s)."""
    d = np.asarray(d, np.float64)
    ct = phase_cos(g, u0)
    st = np.sqrt(np.maximum(1.0 - ct * ct, 0.0))
    ph = 2.0 * np.pi * np.asarray(u1, np.float64)
    x, y = st * np.cos(ph), st * np.sin(ph)
    sg = np.copysign(1.0, d[..., 2])
    a = -1.0 / (sg + d[..., 2])
    b = d[..., 0] * d[..., 1] * a
    s = np.stack([1.0 + sg * d[..., 0] ** 2 * a, sg * b, -sg * d[..., 0]], -1)
    t = np.stack([b, sg + d[..., 1] ** 2 * a, -d[..., 1]], -1)
    return s * x[..., None] + t * y[..., None] + d * ct[..., None]


def replay_medium(o64, V, T, a, r, m, env, tab, H, W, max_depth, seed, objects=(), sample=0, closest=None, lanes=None):
    """-> (L [H,W,3], record), `replay_objects`' arguments (no `occluded`, no `emitter_sample`).  `closest(o, d)` -> (t, index): the
    intersection routine (default `brute`).  `lanes` = (pixel [N], seed [N], sample [N]): these samples in one walk -> L [N,3]."""
    He, We = env.shape[:2]
    envf = env.reshape(-1, 3).astype(np.float64)
    pdf_tab = tab["pdf"].reshape(-1).astype(np.float64)
    row_cdf, col_cdf = tab["row_cdf"], tab["col_cdf"]
    have_tab = bool(tab["row_cdf"][-1] > 0)
    P = V[T]
    if closest is None:
        closest = lambda o, d: brute(P, o, d)
    kind_of = np.zeros(T.shape[0], np.int64)
    obj_of = np.full(T.shape[0], -1, np.int64)
    par = np.zeros((T.shape[0], 3))
    smooth_of = np.zeros(T.shape[0], bool)
    corner = np.zeros((T.shape[0], 3, 3))
    area_of = np.zeros(T.shape[0])
    medium_of = np.zeros(T.shape[0], bool)                          # the triangle bounds a medium
    media = {}                                                     # object -> (sigma_a [3], sigma_s, g)
    lights = []
    for j, ob in enumerate(objects):
        sl = slice(ob["first_tri"], ob["first_tri"] + ob["n_tri"])
        b = ob["bsdf"]
        obj_of[sl] = j
        if b["type"] == "dielectric":
            kind_of[sl], par[sl] = DIELECTRIC, [b["int_ior"], b["ext_ior"], 0.0]
        elif b["type"] == "roughdielectric":
            kind_of[sl], par[sl] = ROUGH, rough_params(b)
        elif b["type"] == "area":
            rad = np.broadcast_to(f32(b.get("radiance", 1.0)), (3,))
            _, A, cdf = pl.light_table(P[sl])
            kind_of[sl], par[sl], area_of[sl] = AREA, rad, A
            lights.append((P[sl], A, cdf, rad))
        elif b["type"] == "diffuse":
            kind_of[sl], par[sl] = DIFFUSE, np.broadcast_to(np.asarray(b["reflectance"], np.float64), (3,))
        else:
            raise ValueError(f"this walk knows kinds 1, 2, 4 and 5, got {b['type']!r}")
        if ob.get("corner_normals") is not None:
            assert b["type"] != "area", "an area light has no shading normals"
            smooth_of[sl], corner[sl] = True, np.asarray(ob["corner_normals"], np.float64)
        if b.get("medium") is not None:
            assert b["type"] in ("dielectric", "roughdielectric"), "a medium fills a dielectric or a roughdielectric object"
            medium_of[sl], media[j] = True, medium_record(b["medium"])
    shadowed = lambda o_, d_, reach: closest(o_, d_)[0] < reach
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
    prev_rough_t = np.zeros(N, bool)
    med = np.full(N, -1, np.int64)                                 # the object whose medium the ray is in
    scattered_in = np.full(N, -1, np.int64)                        # the medium of the path's last medium vertex, while it stays inside
    from_medium_vertex = np.zeros(N, bool)                         # the ray left a medium vertex
    alive = np.ones(N, bool)
    A_, R_, M_ = a.reshape(-1, 3).astype(np.float64), r.reshape(-1).astype(np.float64), m.reshape(-1).astype(np.float64)
    rec = {"H": H, "W": W, "n_e": n_e, **{key: np.zeros(N, bool) for key in FLAGS}, "fallback_cause": np.zeros((N, 3), bool)}

    def emitter(ids, b, depth, po_):
        u2, u3, u4, u5 = (rng_u(b, depth, c) for c in (2, 3, 4, 5))
        n = ids.size
        idx, u_re = pl.choose(u2, n_e)
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
                _, _, wl[e], dist, pe[e] = pl.sample_light(Pl, A, cdf, u_re[e], u3[e], u4[e], po_[e], n_e)
                Le[e], reach[e], lit[e] = rad, dist * (1 - pl.SHADOW_EPS), True
        return wl, Le, pe, reach, lit

    def emitter_term(ids, b, depth, po_, ng, eval_f, two_sided=None):
        if n_e == 0:
            return
        wl, Le, pe, reach, lit = emitter(ids, b, depth, po_)
        fb, pb = eval_f(wl)
        gl = (ng * wl).sum(-1)
        ok = (pe > 0) & (fb > 0).any(-1)
        org = po_
        if two_sided is None:
            ok &= gl > 0
        else:
            org = two_sided[0] + (np.where(gl > 0, 1.0, -1.0) * two_sided[1])[:, None] * ng
        vis = np.zeros(ids.size, bool)
        if ok.any():
            q = np.nonzero(ok)[0]
            vis[q] = ~shadowed(org[ok], wl[ok], reach[ok])
            if P_obj.shape[0]:
                rec["blocked_by_object"][ids[q[brute(P_obj, org[ok], wl[ok])[0] < reach[ok]]]] = True
        w = np.where(vis, mis(pe, pb) / np.where(pe > 0, pe, 1.0), 0.0)
        L[ids] += thr[ids] * fb * Le * w[:, None]
        rec["light_sample_arrives"][ids[vis & lit & (Le > 0).any(-1)]] = True
        rec["light_sample_blocked"][ids[ok & ~vis & lit]] = True
        if two_sided is not None:
            same = gl * (ng * two_sided[2]).sum(-1) > 0
            rec["rough_emitter_reflection_side"][ids[vis & same & (Le > 0).any(-1)]] = True
            rec["rough_emitter_blocked_inside"][ids[ok & ~vis & (gl < 0)]] = True

    def enter_or_leave(ids, k_, ng, wi):
        """The medium rule at a vertex on an object with a medium: the side the new ray leaves on decides."""
        has = medium_of[k_]
        if has.any():
            inside = (ng[has] * wi[has]).sum(-1) < 0
            left = ids[has][~inside]
            rec["scatter_then_exit"][left[scattered_in[left] == obj_of[k_[has]][~inside]]] = True
            med[ids[has]] = np.where(inside, obj_of[k_[has]], -1)
            scattered_in[left] = -1

    for depth in range(max_depth + 1):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        t, k = closest(o[idx], d[idx])
        miss = k < 0
        seg = (med[idx] >= 0) & ~miss                                # ---- a segment inside a medium that the trace closed at t
        if seg.any():
            scat = np.zeros(idx.size, bool)
            for j in np.unique(med[idx[seg]]):
                sa, ss, g = media[j]
                s2 = seg & (med[idx] == j)
                ids = idx[s2]
                dist = t[s2].copy()
                sc = np.zeros(ids.size, bool)
                if ss > 0:
                    s_ = flight(ss, rng_u(base[ids], depth, 9))
                    sc = s_ < dist
                    dist = np.where(sc, s_, dist)
                thr[ids] *= np.exp(-sa[None, :] * dist[:, None])
                rec["absorbed_segment"][ids[~sc]] = True
                iv = ids[sc]
                if iv.size:
                    rec["medium_vertex"][iv] = True
                    scat[np.nonzero(s2)[0][sc]] = True
                    if depth + 1 >= max_depth:
                        rec["cut_inside_medium"][iv] = True
                        alive[iv] = False
                    else:
                        o[iv] = o[iv] + dist[sc][:, None] * d[iv]
                        d[iv] = phase_sample(g, d[iv], rng_u(base[iv], depth, 10), rng_u(base[iv], depth, 11))
                        prev_delta[iv] = True
                        from_medium_vertex[iv] = True
                        scattered_in[iv] = j
            idx, t, k, miss = idx[~scat], t[~scat], k[~scat], miss[~scat]
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
            rec["light_hit_from_medium"][il[front & from_medium_vertex[il]]] = True
            if depth == 0:
                rec["light_at_depth0"][il[front]] = True
            else:
                rec["light_through_glass"][il[front & prev_delta[il]]] = True
                rec["bsdf_hits_light_front"][il[front & ~prev_delta[il]]] = True
                rec["bsdf_hits_light_back"][il[~front & ~prev_delta[il]]] = True
                rec["rough_bsdf_hits_light"][il[front & prev_rough_t[il]]] = True
            idx, t, k = idx[~lit], t[~lit], k[~lit]
        if depth + 1 >= max_depth:
            alive[:] = False
            break
        from_medium_vertex[idx] = False
        n = nrm[k]
        wo = -d[idx]
        kind = kind_of[k]
        front = ((n * wo).sum(-1) > 0) | (kind == DIELECTRIC) | (kind == ROUGH)
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
        prev_rough_t[idx] = False
        sel = kind == SCENE
        if sel.any():                                              # ---- the depth mesh: path_fp64.replay's statements
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
        sel = kind == DIFFUSE
        if sel.any():                                              # ---- a diffuse object: f cos = rho / pi max(ns . wi, 0)
            ids, ng, ns, p, rho = idx[sel], n[sel], nsh[sel], p_all[sel], par[k[sel]]
            po_ = p + eps_all[sel][:, None] * ng
            b = base[ids]
            rec["diffuse_object"][ids] = True
            rec["smooth_diffuse"][ids[sm[sel]]] = True

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
            rec["smooth_transmitted"][ids[trans & sm[sel]]] = True
            rec["redo"][ids[redo]] = True
            enter_or_leave(ids, k[sel], ng, wi)
        sel = kind == ROUGH
        if sel.any():                                              # ---- rough glass: two-sided, never delta; one walk per parameter set
            for pr in np.unique(par[k[sel]], axis=0):
                s2 = sel & (par[k] == pr).all(-1)
                ids, ng, ns, wos, p, eps = idx[s2], n[s2], nsh[s2], wo[s2], p_all[s2], eps_all[s2]
                po_ = p + eps[:, None] * ng
                b = base[ids]

                def glass(wl):
                    e = rough_eval(pr, ng, ns, wos, wl)
                    rec["rough_killed_by_normals"][ids[e["killed"]]] = True
                    return np.repeat(e["f"][:, None], 3, -1), e["pdf"]

                emitter_term(ids, b, depth, po_, ng, glass, two_sided=(p, eps, wos))
                sp = rough_sample(pr, ng, ns, wos, np.stack([rng_u(b, depth, c) for c in (6, 7, 8)], -1))
                wi = sp["wi"]
                side = np.where((ng * wi).sum(-1) > 0, 1.0, -1.0)
                thr[ids] *= sp["weight"][:, None]
                go = (thr[ids] > 0).any(-1)
                alive[ids[~go]] = False
                prev[ids] = sp["pdf"]
                prev_delta[ids] = False
                prev_rough_t[ids] = sp["transmitted"] & go
                o[ids], d[ids] = p + (side * eps)[:, None] * ng, wi
                rec["rough_killed_by_normals"][ids[sp["killed"]]] = True
                rec["rough_reflected"][ids[go & ~sp["transmitted"]]] = True
                rec["rough_transmitted"][ids[go & sp["transmitted"]]] = True
                enter_or_leave(ids, k[s2], ng, wi)
    return (L.reshape(H, W, 3) if lanes is None else L), rec


def merged(V, T, objects):
    """`path_oi_fp64.merged` with each table entry carrying its object's "corner_normals" (None for a flat one); a "medium" travels in
    the entry's bsdf."""
    Vm, Tm, table = po.merged(V, T, objects)
    for entry, ob in zip(table, objects):
        entry["corner_normals"] = ps.corner_normals(ob)
    return Vm, Tm, table


# ---- the shared test scenes ----------------------------------------------------------------------------------------------------------
TINT = {"sigma_a": [4.0, 9.0, 16.0]}                               # per scene unit: the clear sphere's radius is 0.07
CLOUDY_SIDE = 0.16                                                 # `path_rough_fp64.ROUGH_CUBE`'s side: sigma_s side = 0.96
CLOUDY = {"sigma_a": [0.5, 1.0, 2.0], "scatter": 6.0, "g": 0.5}


def table_scene():
    """`path_rough_fp64.table_scene`'s places with media: a smooth-flagged tinted clear-glass icosphere, a cloudy flat rough-glass cube
    (sigma_s side about 1, g 0.5) around the small emitter quad, and a diffuse cube, in front of a depth mesh at z <= -1.6."""
    import path_rough_fp64 as pr

    Vg, Tg, Ng = ps.icosphere(*pr.CLEAR_SPHERE, 1)
    Vc, Tc = po.cube(*pr.ROUGH_CUBE)
    Vq, Tq = pr.inner_quad(pr.ROUGH_CUBE[0], pr.INNER_QUAD_HALF)
    Vd, Td = po.cube(*pl.DIFFUSE_CUBE)
    return [{"vertices": Vg, "triangles": Tg, "bsdf": dict(po.GLASS, medium=TINT), "normals": Ng},
            {"vertices": Vc, "triangles": Tc, "bsdf": dict(pr.FROSTED_005, medium=CLOUDY)},
            {"vertices": Vq, "triangles": Tq, "bsdf": pl.QUAD_LIGHT},
            {"vertices": Vd, "triangles": Td, "bsdf": po.DIFFUSE_08}]


def chords(V, T, o, d):
    """The length of each ray o + t d inside the closed mesh (V, T), by brute force: the sum of its inside intervals between sorted
    crossings -> (length [N], the number of crossings [N])."""
    P = np.asarray(V, np.float64)[np.asarray(T)]
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    pv = np.cross(d[:, None, :], e2[None])
    det = (e1[None] * pv).sum(-1)
    ok = np.abs(det) > 0
    inv = 1.0 / np.where(ok, det, 1.0)
    tv = o[:, None, :] - P[None, :, 0]
    u = (tv * pv).sum(-1) * inv
    qv = np.cross(tv, e1[None])
    v = (d[:, None, :] * qv).sum(-1) * inv
    tt = (e2[None] * qv).sum(-1) * inv
    hit = ok & (u >= 0) & (v >= 0) & (u + v <= 1) & (tt > 0)
    ts = np.sort(np.where(hit, tt, np.inf), axis=1)
    n = hit.sum(1)
    length = np.zeros(o.shape[0])
    for c in range(0, ts.shape[1] - 1, 2):
        both = n >= c + 2
        length += np.where(both, np.where(both, ts[:, c + 1], 0.0) - np.where(both, ts[:, c], 0.0), 0.0)
    return length, n
