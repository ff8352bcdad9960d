"""fp64 restatement of the path render with vertex-coloured inserted objects ("Vertex-coloured inserted
objects"): `path_rough_fp64.replay_rough` with the colour rule.

  * An object of type "diffuse" or "pbr" may carry "colors" [Nv,3], linear RGB in [0, 1]; the table entry holds them as the library
    does, one triple per triangle corner, rounded to fp32 ("corner_colors").
  * At a hit on such an object u, v are Moller-Trumbore's (`path_oi_smooth_fp64.barycentrics`, the ones the smooth normal uses) and
    c = clip(c0 + u (c1 - c0) + v (c2 - c0), 0, 1) per channel.
  * diffuse: reflectance = p (.) c; pbr: albedo = a (.) c, roughness and metallic the record's.  Nothing else changes: neither
    sampler depends on the colour, so the object walks the paths of its uncoloured twin.

Every other statement is `replay_rough`'s: with every corner colour (1, 1, 1), or without a coloured object, the two functions return
the same bits.  No library code.

The record gains `colored_camera` [N,8] (the camera ray's first hit lies on coloured object k) and `colored_indirect` (a later vertex
ray lands on a coloured object, whether max_depth lets it shade there or not)."""
import math

import numpy as np

import path_light_fp64 as pl
import path_oi_fp64 as po
import path_oi_pbr_fp64 as pp
import path_oi_smooth_fp64 as ps
import path_rough_fp64 as pr
from path_fp64 import FOV, brute, env_texel, mis, pcg, rng_u, texel
from path_rough_fp64 import AREA, DIELECTRIC, DIFFUSE, PBR, ROUGH, SCENE, f32, rough_eval, rough_params, rough_sample


def vertex_color(cc, u, v):
    """c = clip(c0 + u (c1 - c0) + v (c2 - c0), 0, 1) for corner colours cc [N,3,3] and barycentrics u, v [N] -> [N,3]; a u, v that is
    not a number gives 0, as the library's clamp does."""
    with np.errstate(invalid="ignore", over="ignore"):
        c = cc[:, 0] + u[:, None] * (cc[:, 1] - cc[:, 0]) + v[:, None] * (cc[:, 2] - cc[:, 0])
    return np.clip(np.where(np.isnan(c), 0.0, c), 0.0, 1.0)


# ---- the walk ----------------------------------------------------------------------------------------------------------------------------
def replay_color(o64, V, T, a, r, m, env, tab, H, W, max_depth, seed, objects=(), sample=0, closest=None, lanes=None, emitter_sample=True):
    """`path_rough_fp64.replay_rough`, statement for statement, where a diffuse or pbr object may carry "corner_colors" [n_tri,3,3] ->
    (L, record).  `emitter_sample=False`: no emitter sample at any vertex and every MIS weight 1."""
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
    colored_of = np.zeros(T.shape[0], bool)
    tint = np.ones((T.shape[0], 3, 3))
    lights = []                                                    # per light: (P, A, cdf, radiance)
    for ob in objects:
        sl = slice(ob["first_tri"], ob["first_tri"] + ob["n_tri"])
        b = ob["bsdf"]
        if b["type"] == "dielectric":
            kind_of[sl], par[sl] = DIELECTRIC, [b["int_ior"], b["ext_ior"], 0.0]
        elif b["type"] == "roughdielectric":
            kind_of[sl], par[sl] = ROUGH, rough_params(b)
        elif b["type"] == "pbr":
            ca, cr, cm = pp.pbr_constants(b)
            kind_of[sl], mat[sl] = PBR, [*ca, cr, cm]
        elif b["type"] == "area":
            rad = np.broadcast_to(f32(b.get("radiance", 1.0)), (3,))
            _, A, cdf = pl.light_table(P[sl])
            kind_of[sl], par[sl], area_of[sl] = AREA, rad, A
            lights.append((P[sl], A, cdf, rad))
        else:
            kind_of[sl], par[sl] = DIFFUSE, np.broadcast_to(np.asarray(b["reflectance"], np.float64), (3,))
        if ob.get("corner_normals") is not None:
            assert b["type"] != "area", "an area light has no shading normals"
            smooth_of[sl], corner[sl] = True, np.asarray(ob["corner_normals"], np.float64)
        if ob.get("corner_colors") is not None:
            assert b["type"] in ("diffuse", "pbr"), "vertex colours tint a diffuse or a pbr object"
            colored_of[sl], tint[sl] = True, np.asarray(ob["corner_colors"], np.float64)
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
    prev_rough_t = np.zeros(N, bool)                               # the ray was transmitted by a rough vertex
    alive = np.ones(N, bool)
    A_, R_, M_ = a.reshape(-1, 3).astype(np.float64), r.reshape(-1).astype(np.float64), m.reshape(-1).astype(np.float64)
    z = lambda: np.zeros(N, bool)
    rec = {"H": H, "W": W, "n_e": n_e, "transmitted": z(), "diffuse_object": z(), "blocked_by_object": z(), "fallback": z(),
           "pbr_vertex": z(), "light_sample_arrives": z(), "light_sample_blocked": z(), "bsdf_hits_light_front": z(),
           "bsdf_hits_light_back": z(), "light_through_glass": z(), "light_at_depth0": z(), "env_sample": z(),
           "rough_reflected": z(), "rough_transmitted": z(), "rough_emitter_reflection_side": z(), "rough_emitter_blocked_inside": z(),
           "rough_bsdf_hits_light": z(), "rough_killed_by_normals": z(), "colored_camera": np.zeros((N, 8), bool), "colored_indirect": z()}

    def emitter(ids, b, depth, po_):
        """One emitter sample per lane -> (wl, radiance [n,3], pdf with its 1 / n_e, the shadow ray's reach, from a light)."""
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
        """The emitter sample of a non-delta vertex added to L; eval_f(wl) -> (f with its cosine, pdf_b).  `two_sided` = (p, eps, wo): a
        rough vertex, whose sample needs no ng . wl > 0 and whose shadow ray starts on wl's side of the face."""
        if n_e == 0 or not emitter_sample:
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
            vis[q] = ~(closest(org[ok], wl[ok])[0] < reach[ok])
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

    for depth in range(max_depth + 1):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        t, k = closest(o[idx], d[idx])
        miss = k < 0
        im = idx[miss]
        if im.size:
            tx = env_texel(d[im], He, We)
            w = np.ones(im.size) if depth == 0 or not emitter_sample else np.where(prev_delta[im], 1.0, mis(prev[im], pdf_tab[tx] / n_e if have_tab else 0.0))
            L[im] += thr[im] * envf[tx] * w[:, None]
        alive[im] = False
        idx, t, k = idx[~miss], t[~miss], k[~miss]
        lit = kind_of[k] == AREA                                   # ---- a light: its emission before the max_depth test
        if lit.any():
            il, tl, kl = idx[lit], t[lit], k[lit]
            cos_o = -(nrm[kl] * d[il]).sum(-1)
            front = cos_o > 0
            unweighted = np.full(il.size, depth == 0 or not emitter_sample) | prev_delta[il]
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
                rec["rough_bsdf_hits_light"][il[front & prev_rough_t[il]]] = True
            idx, t, k = idx[~lit], t[~lit], k[~lit]
        hc = colored_of[k]                                         # the record: a ray that lands on a coloured object, shaded or not
        if hc.any():
            if depth == 0:
                which = [next(j for j, ob in enumerate(objects) if ob["first_tri"] <= kk < ob["first_tri"] + ob["n_tri"]) for kk in k[hc]]
                rec["colored_camera"][idx[hc], which] = True
            else:
                rec["colored_indirect"][idx[hc]] = True
        if depth + 1 >= max_depth:
            alive[:] = False
            break
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
            rec["fallback"][idx[sm]] |= cause.any(-1)
        col = np.ones((idx.size, 3))                               # the colour rule: 1 off the coloured objects
        cl = colored_of[k]
        if cl.any():
            cu, cv = ps.barycentrics(P[k[cl]], o[idx[cl]], d[idx[cl]])
            col[cl] = vertex_color(tint[k[cl]], cu, cv)
        prev_rough_t[idx] = False
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
            av, rv, mv = cm[:, :3] * col[sel], cm[:, 3], cm[:, 4]   # albedo = a (.) c
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
            ids, ng, ns, p, rho = idx[sel], n[sel], nsh[sel], p_all[sel], par[k[sel]] * col[sel]   # reflectance = p (.) c
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
    return (L.reshape(H, W, 3) if lanes is None else L), rec


def replay_mean(H, W, spp, seeds, max_depth, V, T, env, tab, objects, chunk=8, emitter_sample=True):
    """`path_rough_fp64.replay_mean` over `replay_color` -> [len(seeds), H, W, 3]."""
    maps = (np.zeros((H, W, 3), np.float32), np.ones((H, W, 1), np.float32), np.zeros((H, W, 1), np.float32))
    out = np.zeros((len(seeds), H, W, 3))
    pix, smp = np.meshgrid(np.arange(H * W), np.arange(spp), indexing="ij")
    for c0 in range(0, len(seeds), chunk):
        sd = np.asarray(seeds[c0:c0 + chunk])
        lanes = (np.tile(pix.reshape(-1), sd.size), np.repeat(sd, pix.size), np.tile(smp.reshape(-1), sd.size))
        L, _ = replay_color(None, V, T, *maps, env, tab, H, W, max_depth, 0, objects, lanes=lanes, emitter_sample=emitter_sample)
        out[c0:c0 + sd.size] = L.reshape(sd.size, H, W, spp, 3).mean(3)
    return out


# ---- the shared test scenes ----------------------------------------------------------------------------------------------------------
COLOR_SPHERE = ((0.08, 0.12, -1.10), 0.09)                         # `path_rough_fp64`'s rough sphere's place
COLOR_CUBE = ((0.13, -0.12, -1.36), 0.16, (0.0, 0.5, 0.0))         # its rough cube's
PLAIN_CUBE = pl.DIFFUSE_CUBE
CLEAR_SPHERE = pr.CLEAR_SPHERE
PBR_BASE = {"type": "pbr", "albedo": (0.9, 0.8, 0.7), "roughness": 0.4, "metallic": 0.2}
DIFFUSE_BASE = {"type": "diffuse", "reflectance": (0.9, 0.85, 0.8)}


def vertex_colors(V, seed):
    """Colours that vary per vertex, with corners at 0 and at 1 among them: fp32 values in [0, 1]."""
    rng = np.random.default_rng(seed)
    C = rng.random((len(V), 3))
    C[0], C[1] = 0.0, 1.0
    return C.astype(np.float32).astype(np.float64)


def table_scene(uniform=False, flagged=True):
    """The GPU parity scene's table, in front of a depth mesh at z <= -1.6: a vertex-coloured smooth diffuse icosphere, a
    vertex-coloured flat PBR cube, an uncoloured diffuse cube and a clear-glass icosphere.  `uniform`: every colour (1, 1, 1);
    `flagged=False`: the same table without colours."""
    Vs, Ts, Ns = ps.icosphere(*COLOR_SPHERE, 1)
    Vc, Tc = po.cube(*COLOR_CUBE)
    Vd, Td = po.cube(*PLAIN_CUBE)
    Vg, Tg, Ng = ps.icosphere(*CLEAR_SPHERE, 1)
    out = [{"vertices": Vs, "triangles": Ts, "bsdf": DIFFUSE_BASE, "normals": Ns},
           {"vertices": Vc, "triangles": Tc, "bsdf": PBR_BASE},
           {"vertices": Vd, "triangles": Td, "bsdf": po.DIFFUSE_08},
           {"vertices": Vg, "triangles": Tg, "bsdf": po.GLASS, "normals": Ng}]
    if flagged:
        out[0]["colors"] = np.ones_like(Vs) if uniform else vertex_colors(Vs, 21)
        out[1]["colors"] = np.ones_like(Vc) if uniform else vertex_colors(Vc, 22)
    return out


def corner_colors(ob):
    """The object's "colors" as the library stores them: one per triangle corner, rounded to fp32; None without colours."""
    if ob.get("colors") is None:
        return None
    return np.asarray(ob["colors"], np.float64)[np.asarray(ob["triangles"], np.int64)].astype(np.float32).astype(np.float64)


def merged(V, T, objects):
    """`path_rough_fp64.merged` with each table entry carrying its "corner_colors"."""
    Vm, Tm, table = pr.merged(V, T, objects)
    for entry, ob in zip(table, objects):
        entry["corner_colors"] = corner_colors(ob)
    return Vm, Tm, table


# the closed form in expectation: `path_light_fp64.furnace_scene`'s box around a diffuse cube whose camera-facing face is perpendicular
# to the view axis and whose corner colours are an affine function of world position
FURNACE_CUBE = ((0.0, 0.0, -1.2), 0.5)
FURNACE_P = (0.9, 0.8, 0.7)
FURNACE_GRAD = ((0.5, 0.9, 0.0), (0.2, -0.7, 0.4), (0.0, 0.3, 0.9))   # d rho[c] / d (x, y, z)
FURNACE_AT_CENTRE = (0.5, 0.45, 0.4)


def furnace_color(x):
    """rho(x) [..., 3], affine in world position, inside [0, 1] on the cube."""
    return np.asarray(FURNACE_AT_CENTRE) + (np.asarray(x, np.float64) - np.asarray(FURNACE_CUBE[0])) @ np.asarray(FURNACE_GRAD).T


def furnace_scene():
    """-> the objects: the emitting box and the axis-aligned coloured diffuse cube."""
    Vb, Tb = pl.box(*pl.FURNACE_BOX, inward=True)
    Vi, Ti = po.cube(FURNACE_CUBE[0], FURNACE_CUBE[1], (0.0, 0.0, 0.0))
    Vi = Vi.astype(np.float32).astype(np.float64)
    cube = {"vertices": Vi, "triangles": Ti, "bsdf": {"type": "diffuse", "reflectance": FURNACE_P}, "colors": furnace_color(Vi)}
    return [{"vertices": Vb, "triangles": Tb, "bsdf": {"type": "area", "radiance": pl.FURNACE_L}}, cube]
