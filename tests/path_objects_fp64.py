"""fp64 restatement of the path render with inserted objects of every kind: the one walk the object tests
measure the kernels against.  `path_oi_fp64.replay_oi` stays beside it as the independent base statement (glass and diffuse, flat),
and on a flat glass-and-diffuse table the two return the same bits.

`replay_objects` walks one sample of every pixel (or the given lanes) as `path_fp64.replay` does; the depth mesh's vertices run the
same statements in the same order.  An object of the table is {"first_tri", "n_tri", "bsdf"} plus what `merged` adds.  The rules, in
the order the render gained them; each feature module holds its rule's samplers, constants and scenes, and a table without a feature
returns the bits of the walk without its rule:

  * Glass and diffuse (`path_oi_fp64`): "dielectric" is a delta vertex that shades from both sides, takes no emitter sample and
    spawns the next ray on the side it leaves on; "diffuse" is one-sided about the outward face normal ng, f cos = rho / pi
    max(ns . wi, 0), with an emitter sample (dims 2-5, needs ng . wl > 0) and a cosine sample (dims 7, 8); a sample below the face
    ends the path.

  * Smooth shading normals (`path_oi_smooth_fp64`): an object may carry "corner_normals" [n_tri,3,3]; at a hit on it the BSDF shades
    with ns, the normal interpolated by Moller-Trumbore's u, v with its three fallbacks to ng (`shading_normal`), and ng keeps the
    geometry.  A dielectric event about ns that disagrees with the geometry is redone about ng (`sample_dielectric_shading`).

  * PBR (`path_oi_pbr_fp64`): "pbr" runs the depth mesh's vertex on the object's constants (rounded to fp32) instead of a texel:
    one-sided about ng, BSDF about ns, never delta; a BSDF sample with ng . wi <= 0 ends the path; the next ray starts at p + eps ng.

  * Area lights (`path_light_fp64`): "area" emits.  The emitters are the envmap where it has tables, then the lights in table order,
    n_e in all; an emitter sample picks one by sample reuse of dim 2 (`choose`, in fp32) and a light's point by `sample_light`, with
    a shadow ray that reaches dist (1 - 1e-3).  A traced ray that lands on a light's front adds thr p w BEFORE the max_depth test,
    w = 1 at depth 0 or after a delta vertex, else mis(prev_pdf, t^2 / (A (ng . wo) n_e)); front or back, the path ends.  An escaped
    ray's weight takes env_pdf / n_e.

  * Rough glass (`path_rough_fp64`): "roughdielectric" shades from both sides and is never delta (`rough_sample`, `rough_eval`); its
    emitter sample is drawn from p + eps ng, is taken on either side of the face, and its shadow ray starts on wl's side.

  * Vertex colours (`path_color_fp64`): a diffuse or pbr object may carry "corner_colors" [n_tri,3,3]; reflectance = p (.) c,
    albedo = a (.) c with c = `vertex_color` at the hit's u, v.  Neither sampler depends on the colour.

  * Textures (`path_texture_fp64`): a diffuse or pbr object may carry "corner_uv" [n_tri,3,2] with "texture" and (pbr) "orm_texture";
    the base colour multiplies c, and an orm fetch (o, g, b) gives roughness = clip(r g, 0.07, 1), metallic = clip(m b, 0, 1).

No library code: the default intersection is `path_fp64.brute`.  `closest(o, d)` -> (t, index) may be bound to the library's fp32
traversal, and `occluded(o, d)` -> bool to its any-hit routine.

The record holds `n_e` and, per pixel (or lane): `transmitted`, `diffuse_object`, `blocked_by_object`; `smooth_transmitted`,
`smooth_diffuse`, `redo`, `fallback`, `fallback_cause` [N,3]; `pbr_vertex`, `pbr_smooth_vertex`, `pbr_below_ng` (a BSDF sample ended
by ng . wi <= 0; `pbr_below_ng_carrying`: one whose weight about ns was not zero already), `pbr_emitter_below_ng` (an emitter sample
the BSDF about ns would have carried, refused by ng . wl <= 0); `light_sample_arrives`, `light_sample_blocked`,
`bsdf_hits_light_front` / `_back`, `light_through_glass`, `light_at_depth0`, `env_sample` (an envmap sample taken while lights
compete); `rough_reflected`, `rough_transmitted`, `rough_emitter_reflection_side`, `rough_emitter_blocked_inside`,
`rough_bsdf_hits_light`, `rough_killed_by_normals`; `colored_camera` [N,8] / `textured_camera` [N,8] (the camera ray's first hit lies
on coloured / textured object k), `colored_indirect` / `textured_indirect` (a later ray lands on one, shaded or not),
`fetch_wraps_columns` / `fetch_wraps_rows`, `orm_roughness_floor` (a pbr vertex whose r g lies at or below the 0.07 floor)."""
import math

import numpy as np

import path_light_fp64 as pl
import path_oi_fp64 as po
import path_oi_pbr_fp64 as pp
import path_oi_smooth_fp64 as ps
from path_color_fp64 import corner_colors, vertex_color
from path_fp64 import FOV, brute, env_texel, mis, pcg, rng_u, texel
from path_rough_fp64 import AREA, DIELECTRIC, DIFFUSE, PBR, ROUGH, SCENE, f32, rough_eval, rough_params, rough_sample
from path_texture_fp64 import ROUGHNESS_FLOOR, corner_uv, texture_fetch, texture_st

FLAGS = ("transmitted", "diffuse_object", "blocked_by_object", "smooth_transmitted", "smooth_diffuse", "redo", "fallback", "pbr_vertex",
         "pbr_smooth_vertex", "pbr_below_ng", "pbr_below_ng_carrying", "pbr_emitter_below_ng", "light_sample_arrives", "light_sample_blocked",
         "bsdf_hits_light_front", "bsdf_hits_light_back", "light_through_glass", "light_at_depth0", "env_sample", "rough_reflected",
         "rough_transmitted", "rough_emitter_reflection_side", "rough_emitter_blocked_inside", "rough_bsdf_hits_light",
         "rough_killed_by_normals", "colored_indirect", "textured_indirect", "fetch_wraps_columns", "fetch_wraps_rows", "orm_roughness_floor")


def replay_objects(o64, V, T, a, r, m, env, tab, H, W, max_depth, seed, objects=(), sample=0, closest=None, occluded=None, lanes=None,
                   emitter_sample=True):
    """-> (L [H,W,3], record).  `closest(o, d)` -> (t, index): the intersection routine (default `brute`); a shadow ray is occluded
    where its closest hit lies nearer than its reach.  `occluded(o, d)` -> bool answers the shadow rays instead; it knows no reach, so
    it serves the envmap's rays alone and a table with an area light is refused with it.  `lanes` = (pixel [N], seed [N], sample [N]):
    these samples in one walk instead of one sample of every pixel -> L [N,3] (the record's entries are per lane then).
    `emitter_sample=False`: the same estimator's other half alone, no emitter sample at any vertex and every MIS weight 1."""
    He, We = env.shape[:2]
    envf = env.reshape(-1, 3).astype(np.float64)
    pdf_tab = tab["pdf"].reshape(-1).astype(np.float64)
    row_cdf, col_cdf = tab["row_cdf"], tab["col_cdf"]
    have_tab = bool(tab["row_cdf"][-1] > 0)
    P = V[T]
    if closest is None:
        closest = lambda o, d: brute(P, o, d)
    kind_of = np.zeros(T.shape[0], np.int64)
    obj_of = np.full(T.shape[0], -1, np.int64)                     # the object a triangle belongs to
    par = np.zeros((T.shape[0], 3))
    mat = np.zeros((T.shape[0], 5))
    smooth_of = np.zeros(T.shape[0], bool)
    corner = np.zeros((T.shape[0], 3, 3))
    area_of = np.zeros(T.shape[0])
    colored_of = np.zeros(T.shape[0], bool)
    tint = np.ones((T.shape[0], 3, 3))
    textured_of, orm_of = np.zeros(T.shape[0], bool), np.zeros(T.shape[0], bool)
    st_of = np.zeros((T.shape[0], 3, 2))
    lights = []                                                    # per light: (P, A, cdf, radiance)
    for j, ob in enumerate(objects):
        sl = slice(ob["first_tri"], ob["first_tri"] + ob["n_tri"])
        b = ob["bsdf"]
        obj_of[sl] = j
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
        if ob.get("corner_uv") is not None:
            assert b["type"] in ("diffuse", "pbr"), "an image textures a diffuse or a pbr object"
            assert ob.get("texture") is not None or ob.get("orm_texture") is not None, "a textured object needs an image"
            assert ob.get("orm_texture") is None or b["type"] == "pbr", "an orm image belongs to a pbr object"
            textured_of[sl], st_of[sl], orm_of[sl] = True, np.asarray(ob["corner_uv"], np.float64), ob.get("orm_texture") is not None
    if occluded is None:
        shadowed = lambda o_, d_, reach: closest(o_, d_)[0] < reach
    elif lights:
        raise ValueError("occluded= answers shadow rays of unbounded reach only; a light's shadow ray ends before the light: use closest=")
    else:
        shadowed = lambda o_, d_, reach: occluded(o_, d_)
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
    rec = {"H": H, "W": W, "n_e": n_e, **{key: np.zeros(N, bool) for key in FLAGS}, "fallback_cause": np.zeros((N, 3), bool),
           "colored_camera": np.zeros((N, 8), bool), "textured_camera": np.zeros((N, 8), bool)}

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

    def emitter_term(ids, b, depth, po_, ng, eval_f, two_sided=None, refused=None):
        """The emitter sample of a non-delta vertex added to L; eval_f(wl) -> (f with its cosine, pdf_b).  `two_sided` = (p, eps, wo): a
        rough vertex, whose sample needs no ng . wl > 0 and whose shadow ray starts on wl's side of the face.  `refused`: the record
        key of the samples that ng . wl <= 0 alone refuses."""
        if n_e == 0 or not emitter_sample:
            return
        wl, Le, pe, reach, lit = emitter(ids, b, depth, po_)
        fb, pb = eval_f(wl)
        gl = (ng * wl).sum(-1)
        ok = (pe > 0) & (fb > 0).any(-1)
        org = po_
        if two_sided is None:
            if refused is not None:
                rec[refused][ids[ok & ~(gl > 0)]] = True
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
        for flag, name in ((colored_of[k], "colored"), (textured_of[k], "textured")):   # a ray that lands on a flagged object, shaded or not
            if flag.any():
                if depth == 0:
                    rec[name + "_camera"][idx[flag], obj_of[k[flag]]] = True
                else:
                    rec[name + "_indirect"][idx[flag]] = True
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
        sm = smooth_of[k]                                          # the shading normal: interpolated on a smooth object, else ng
        nsh = n.copy()
        if sm.any():
            bu, bv = ps.barycentrics(P[k[sm]], o[idx[sm]], d[idx[sm]])
            nsh[sm], cause = ps.shading_normal(corner[k[sm]], bu, bv, n[sm], wo[sm])
            rec["fallback_cause"][idx[sm]] |= cause
            rec["fallback"][idx[sm]] |= cause.any(-1)
        col = np.ones((idx.size, 3))                               # the colour rule: 1 off the coloured objects
        cl = colored_of[k]
        if cl.any():
            cu, cv = ps.barycentrics(P[k[cl]], o[idx[cl]], d[idx[cl]])
            col[cl] = vertex_color(tint[k[cl]], cu, cv)
        orm = np.ones((idx.size, 3))                               # the texture rule: 1 off the textured objects
        for j in np.unique(obj_of[k][textured_of[k]]):
            tx = textured_of[k] & (obj_of[k] == j)
            tu, tv = ps.barycentrics(P[k[tx]], o[idx[tx]], d[idx[tx]])
            s_, t_ = texture_st(st_of[k[tx]], tu, tv)
            for key in ("texture", "orm_texture"):
                if objects[j].get(key) is None:
                    continue
                c, wx, wy = texture_fetch(np.asarray(objects[j][key], np.float64), s_, t_)
                rec["fetch_wraps_columns"][idx[tx]] |= wx
                rec["fetch_wraps_rows"][idx[tx]] |= wy
                if key == "texture":
                    col[tx] = col[tx] * c                          # p (.) c_vertex (.) c_base
                else:
                    orm[tx] = c
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
        sel = kind == PBR
        if sel.any():                                              # ---- a PBR object: the depth mesh's vertex on the object's constants
            ids, ng, ns, wos, p = idx[sel], n[sel], nsh[sel], wo[sel], p_all[sel]
            cm = mat[k[sel]]
            av = cm[:, :3] * col[sel]                              # albedo = a (.) c_vertex (.) c_base
            has_orm = orm_of[k[sel]]
            rv = np.where(has_orm, np.clip(cm[:, 3] * orm[sel][:, 1], ROUGHNESS_FLOOR, 1.0), cm[:, 3])
            mv = np.where(has_orm, np.clip(cm[:, 4] * orm[sel][:, 2], 0.0, 1.0), cm[:, 4])
            rec["orm_roughness_floor"][ids[has_orm & (cm[:, 3] * orm[sel][:, 1] <= ROUGHNESS_FLOOR)]] = True
            po_ = p + eps_all[sel][:, None] * ng
            b = base[ids]
            rec["pbr_vertex"][ids] = True
            rec["pbr_smooth_vertex"][ids[sm[sel]]] = True
            emitter_term(ids, b, depth, po_, ng, lambda wl: o64.eval_brdf(wl, wos, ns, av, rv, mv), refused="pbr_emitter_below_ng")
            s1, s2a, s2b = (rng_u(b, depth, c) for c in (6, 7, 8))
            wi, pdf, wgt = o64.sample_brdf(s1, np.stack([s2a, s2b], -1), wos, ns, av, rv, mv)
            below = ~((ng * wi).sum(-1) > 0)                       # a sample that leaves below the face ends the path
            rec["pbr_below_ng"][ids[below]] = True
            rec["pbr_below_ng_carrying"][ids[below & (wgt > 0).any(-1)]] = True
            thr[ids] *= wgt
            alive[ids[~(thr[ids] > 0).any(-1) | below]] = False
            prev[ids] = pdf
            prev_delta[ids] = False
            o[ids], d[ids] = po_, wi
        sel = kind == DIFFUSE
        if sel.any():                                              # ---- a diffuse object: f cos = rho / pi max(ns . wi, 0)
            ids, ng, ns, p, rho = idx[sel], n[sel], nsh[sel], p_all[sel], par[k[sel]] * col[sel]   # reflectance = p (.) c
            po_ = p + eps_all[sel][:, None] * ng
            b = base[ids]
            rec["diffuse_object"][ids] = True
            rec["smooth_diffuse"][ids[sm[sel]]] = True

            def lambert(wl):
                c = np.maximum((ns * wl).sum(-1), 0.0)
                return rho * (c / np.pi)[:, None], c / np.pi

            emitter_term(ids, b, depth, po_, ng, lambert)
            wi, pdf = po.sample_diffuse(ns, rng_u(b, depth, 7), rng_u(b, depth, 8))
            below = ~((ng * wi).sum(-1) > 0)                       # sampled below the face: the path ends
            thr[ids] *= np.where(below[:, None], 0.0, rho)
            alive[ids[~(thr[ids] > 0).any(-1)]] = False
            prev[ids] = pdf
            prev_delta[ids] = False
            o[ids], d[ids] = po_, wi
        sel = kind == DIELECTRIC
        if sel.any():                                              # ---- glass: a delta vertex, no emitter sample
            ids, ng, ns, p, pr = idx[sel], n[sel], nsh[sel], p_all[sel], par[k[sel]]
            wi, wgt, prob, trans, redo = ps.sample_dielectric_shading(pr[:, 0], pr[:, 1], ng, ns, wo[sel], rng_u(base[ids], depth, 6))
            side = np.where((ng * wi).sum(-1) > 0, 1.0, -1.0)      # spawn on the side the new ray leaves on
            thr[ids] *= wgt[:, None]
            prev[ids] = prob
            prev_delta[ids] = True
            o[ids], d[ids] = p + (side * eps_all[sel])[:, None] * ng, wi
            rec["transmitted"][ids[trans]] = True
            rec["smooth_transmitted"][ids[trans & sm[sel]]] = True
            rec["redo"][ids[redo]] = True
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
    """The spp-sample estimate of every pixel for each seed, over a depth mesh that no ray meets (no maps, no oracle) ->
    [len(seeds), H, W, 3]; `chunk` seeds per walk."""
    maps = (np.zeros((H, W, 3), np.float32), np.ones((H, W, 1), np.float32), np.zeros((H, W, 1), np.float32))
    out = np.zeros((len(seeds), H, W, 3))
    pix, smp = np.meshgrid(np.arange(H * W), np.arange(spp), indexing="ij")
    for c0 in range(0, len(seeds), chunk):
        sd = np.asarray(seeds[c0:c0 + chunk])
        lanes = (np.tile(pix.reshape(-1), sd.size), np.repeat(sd, pix.size), np.tile(smp.reshape(-1), sd.size))
        L, _ = replay_objects(None, V, T, *maps, env, tab, H, W, max_depth, 0, objects, lanes=lanes, emitter_sample=emitter_sample)
        out[c0:c0 + sd.size] = L.reshape(sd.size, H, W, spp, 3).mean(3)
    return out


def merged(V, T, objects):
    """`path_oi_fp64.merged` with each table entry carrying what the library holds of its object: "corner_normals", "corner_colors",
    "corner_uv" and the images rounded to fp32; None where the object has none."""
    Vm, Tm, table = po.merged(V, T, objects)
    for entry, ob in zip(table, objects):
        entry.update(corner_normals=ps.corner_normals(ob), corner_colors=corner_colors(ob), corner_uv=corner_uv(ob))
        for key in ("texture", "orm_texture"):
            entry[key] = None if ob.get(key) is None else np.asarray(ob[key], np.float32).astype(np.float64)
    return Vm, Tm, table
