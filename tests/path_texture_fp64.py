"""fp64 restatement of the path render with UV-textured inserted objects ("Textured inserted objects"):
`path_color_fp64.replay_color` with the texture rule.

  * An object of type "diffuse" or "pbr" may carry "uv" [Nv,2] with "texture" [h,w,3] (base colour, linear, in [0, 1], row 0 the top
    row) and, a pbr one, "orm_texture" [h,w,3]; the table entry holds the coordinates as the library does, one pair per triangle
    corner, rounded to fp32 ("corner_uv"), and the images rounded to fp32.
  * At a hit on such an object u, v are Moller-Trumbore's (`path_oi_smooth_fp64.barycentrics`), (s, t) = st0 + u (st1 - st0) +
    v (st2 - st0), and an image of W x H texels is read with bilinear filtering and repeat wrapping: fs = s - floor(s),
    x = fs W - 1/2, x0 = floor(x), fx = x - x0, columns x0 and x0 + 1 wrapped into [0, W); t = 0 is the image's bottom,
    y = (1 - ft) H - 1/2, the rows likewise; c = clip(top + fy (bot - top), 0, 1) with top, bot the two rows blended by fx.  A
    coordinate that is not finite reads (0, 0, 0).
  * diffuse: reflectance = p (.) c_vertex (.) c_base; pbr: albedo = a (.) c_vertex (.) c_base and, with an orm image whose fetch is
    (o, g, b), roughness = clip(r g, 0.07, 1), metallic = clip(m b, 0, 1).  A base-colour image changes no path; an orm image does.

Every other statement is `replay_color`'s: with every image (1, 1, 1), or without a textured object, the two functions return the same
bits.  No library code.

The record gains `textured_camera` [N,8] (the camera ray's first hit lies on textured object k), `textured_indirect` (a later vertex
ray lands on a textured object, whether max_depth lets it shade there or not), `fetch_wraps_columns` / `fetch_wraps_rows` (a fetch at a
shaded vertex paired column W - 1 with column 0, or row H - 1 with row 0) and `orm_roughness_floor` (a pbr vertex whose r g lies at or
below the 0.07 floor)."""
import math

import numpy as np

import path_color_fp64 as pc
import path_light_fp64 as pl
import path_oi_fp64 as po
import path_oi_pbr_fp64 as pp
import path_oi_smooth_fp64 as ps
import path_rough_fp64 as pr
from path_color_fp64 import vertex_color
from path_fp64 import FOV, brute, env_texel, mis, pcg, rng_u, texel
from path_rough_fp64 import AREA, DIELECTRIC, DIFFUSE, PBR, ROUGH, SCENE, f32, rough_eval, rough_params, rough_sample

ROUGHNESS_FLOOR = 0.07


def texture_st(cs, u, v, dtype=np.float64):
    """(s, t) = st0 + u (st1 - st0) + v (st2 - st0) for corner coordinates cs [N,3,2] and barycentrics u, v [N] -> s [N], t [N]."""
    cs, u, v = np.asarray(cs, dtype), np.asarray(u, dtype), np.asarray(v, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        st = cs[:, 0] + u[:, None] * (cs[:, 1] - cs[:, 0]) + v[:, None] * (cs[:, 2] - cs[:, 0])
    return st[:, 0], st[:, 1]


def _axis(f, n, dtype):
    """One axis of the fetch: position f in [0, 1] among n texel centres -> (i0, i1 wrapped into [0, n), the weight of i1, wrapped)."""
    x = f * dtype(n) - dtype(0.5)
    x0 = np.floor(x)
    k = np.clip(x0.astype(np.int64), -1, n - 1)
    return k % n, (k + 1) % n, x - x0, (k < 0) | (k + 1 >= n)


def texture_fetch(img, s, t, dtype=np.float64):
    """The bilinear, repeat-wrapped read of img [h,w,3] (row 0 the top row) at (s, t) [N] -> (c [N,3] in [0, 1], the fetch paired
    column w - 1 with column 0 [N], row h - 1 with row 0 [N]).  `dtype=np.float32`: the same statements in fp32, each rounded once
    (the transcription the library's error is measured against)."""
    img = np.asarray(img, dtype)
    h, w = img.shape[:2]
    s, t = np.asarray(s, dtype), np.asarray(t, dtype)
    ok = np.isfinite(s) & np.isfinite(t)
    s, t = np.where(ok, s, dtype(0)), np.where(ok, t, dtype(0))
    fs, ft = s - np.floor(s), t - np.floor(t)
    fs, ft = np.where(fs < 1, fs, dtype(0)), np.where(ft < 1, ft, dtype(0))
    x0, x1, fx, wx = _axis(fs, w, dtype)
    y0, y1, fy, wy = _axis(dtype(1) - ft, h, dtype)
    fx, fy = fx[:, None], fy[:, None]
    top = img[y0, x0] + fx * (img[y0, x1] - img[y0, x0])
    bot = img[y1, x0] + fx * (img[y1, x1] - img[y1, x0])
    c = np.clip(top + fy * (bot - top), 0, 1)
    return np.where(ok[:, None], c, dtype(0)).astype(dtype), wx & ok, wy & ok


# ---- the walk ----------------------------------------------------------------------------------------------------------------------------
def replay_texture(o64, V, T, a, r, m, env, tab, H, W, max_depth, seed, objects=(), sample=0, closest=None, lanes=None, emitter_sample=True):
    """`path_color_fp64.replay_color`, statement for statement, where a diffuse or pbr object may also carry "corner_uv" [n_tri,3,2] with
    "texture" and (pbr) "orm_texture" [h,w,3] -> (L, record).  `emitter_sample=False`: no emitter sample at any vertex and every MIS
    weight 1."""
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
    tex_of = np.full(T.shape[0], -1, np.int64)                     # the textured object a triangle belongs to
    st_of = np.zeros((T.shape[0], 3, 2))
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
        if ob.get("corner_uv") is not None:
            assert b["type"] in ("diffuse", "pbr"), "an image textures a diffuse or a pbr object"
            assert ob.get("texture") is not None or ob.get("orm_texture") is not None, "a textured object needs an image"
            assert ob.get("orm_texture") is None or b["type"] == "pbr", "an orm image belongs to a pbr object"
            tex_of[sl], st_of[sl] = next(j for j, x in enumerate(objects) if x is ob), np.asarray(ob["corner_uv"], np.float64)
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
           "rough_bsdf_hits_light": z(), "rough_killed_by_normals": z(), "colored_camera": np.zeros((N, 8), bool), "colored_indirect": z(),
           "textured_camera": np.zeros((N, 8), bool), "textured_indirect": z(), "fetch_wraps_columns": z(), "fetch_wraps_rows": z(),
           "orm_roughness_floor": z()}

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
        ht = tex_of[k] >= 0                                         # the record: a ray that lands on a textured object, shaded or not
        if ht.any():
            if depth == 0:
                rec["textured_camera"][idx[ht], tex_of[k[ht]]] = True
            else:
                rec["textured_indirect"][idx[ht]] = True
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
        orm = np.ones((idx.size, 3))                               # the texture rule: 1 off the textured objects
        for j in np.unique(tex_of[k][tex_of[k] >= 0]):
            tx = tex_of[k] == j
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
            av = cm[:, :3] * col[sel]                              # albedo = a (.) c_vertex (.) c_base
            has_orm = np.array([tex_of[kk] >= 0 and objects[tex_of[kk]].get("orm_texture") is not None for kk in k[sel]], bool)
            rv = np.where(has_orm, np.clip(cm[:, 3] * orm[sel][:, 1], ROUGHNESS_FLOOR, 1.0), cm[:, 3])
            mv = np.where(has_orm, np.clip(cm[:, 4] * orm[sel][:, 2], 0.0, 1.0), cm[:, 4])
            rec["orm_roughness_floor"][idx[sel][has_orm & (cm[:, 3] * orm[sel][:, 1] <= ROUGHNESS_FLOOR)]] = True
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
    """`path_color_fp64.replay_mean` over `replay_texture` -> [len(seeds), H, W, 3]."""
    maps = (np.zeros((H, W, 3), np.float32), np.ones((H, W, 1), np.float32), np.zeros((H, W, 1), np.float32))
    out = np.zeros((len(seeds), H, W, 3))
    pix, smp = np.meshgrid(np.arange(H * W), np.arange(spp), indexing="ij")
    for c0 in range(0, len(seeds), chunk):
        sd = np.asarray(seeds[c0:c0 + chunk])
        lanes = (np.tile(pix.reshape(-1), sd.size), np.repeat(sd, pix.size), np.tile(smp.reshape(-1), sd.size))
        L, _ = replay_texture(None, V, T, *maps, env, tab, H, W, max_depth, 0, objects, lanes=lanes, emitter_sample=emitter_sample)
        out[c0:c0 + sd.size] = L.reshape(sd.size, H, W, spp, 3).mean(3)
    return out


# ---- the shared test scenes ----------------------------------------------------------------------------------------------------------
TEX_SPHERE = pc.COLOR_SPHERE                                        # `path_color_fp64`'s coloured sphere's place
TEX_CUBE = pc.COLOR_CUBE                                            # its coloured cube's
BOTH_CUBE = ((0.27, 0.07, -1.25), 0.1, (0.3, 0.2, 0.0))            # a vertex-coloured and textured diffuse cube, right of the sphere
PLAIN_CUBE = pc.PLAIN_CUBE
CLEAR_SPHERE = pc.CLEAR_SPHERE
PBR_BASE = {"type": "pbr", "albedo": (0.9, 0.8, 0.7), "roughness": 0.5, "metallic": 0.6}
DIFFUSE_BASE = pc.DIFFUSE_BASE


def image(h, w, seed, lo=0.0):
    """A random image [h,w,3] of fp32 values in [lo, 1], with a texel at lo and one at 1 among them."""
    A = lo + (1 - lo) * np.random.default_rng(seed).random((h, w, 3))
    A[0, 0], A[-1, -1] = lo, 1.0
    return A.astype(np.float32).astype(np.float64)


def orm_image():
    """3 x 2 (w x h) texels: g drives the roughness of PBR_BASE (0.5) to the 0.07 floor in four of them, b scales the metallic."""
    A = image(2, 3, 33, 0.2)
    A[0, :, 1] = (0.0, 0.1, 0.05)
    A[1, 1, 1] = 0.0
    return A.astype(np.float32).astype(np.float64)


def sphere_uv(V, centre):
    """Latitude-longitude coordinates of a sphere's vertices scaled by 2.5 and shifted by -1.3: both seams and negative values occur."""
    n = (V - np.asarray(centre)) / np.linalg.norm(V - np.asarray(centre), axis=-1, keepdims=True)
    st = np.stack([np.arctan2(n[:, 0], n[:, 2]) / (2 * np.pi) + 0.5, np.arccos(np.clip(n[:, 1], -1, 1)) / np.pi], -1)
    return (2.5 * st - 1.3).astype(np.float32).astype(np.float64)


def cube_uv(V, seed, scale=1.7):
    """Per-vertex coordinates of a cube that cross the seams: random in [-scale, scale]."""
    return ((np.random.default_rng(seed).random((len(V), 2)) * 2 - 1) * scale).astype(np.float32).astype(np.float64)


def table_scene(uniform=False, flagged=True):
    """The GPU parity scene's table, in front of a depth mesh at z <= -1.6: a smooth diffuse icosphere with a 5 x 4 texture, a flat PBR
    cube with a 2 x 3 base image and a 3 x 2 orm image, a vertex-coloured and textured diffuse cube, an untextured diffuse cube and a
    clear-glass icosphere.  `uniform`: every image (1, 1, 1); `flagged=False`: the same table without textures (the colours stay)."""
    Vs, Ts, Ns = ps.icosphere(*TEX_SPHERE, 1)
    Vc, Tc = po.cube(*TEX_CUBE)
    Vb, Tb = po.cube(*BOTH_CUBE)
    Vd, Td = po.cube(*PLAIN_CUBE)
    Vg, Tg, Ng = ps.icosphere(*CLEAR_SPHERE, 1)
    out = [{"vertices": Vs, "triangles": Ts, "bsdf": DIFFUSE_BASE, "normals": Ns},
           {"vertices": Vc, "triangles": Tc, "bsdf": PBR_BASE},
           {"vertices": Vb, "triangles": Tb, "bsdf": po.DIFFUSE_08, "colors": pc.vertex_colors(Vb, 23)},
           {"vertices": Vd, "triangles": Td, "bsdf": po.DIFFUSE_08},
           {"vertices": Vg, "triangles": Tg, "bsdf": po.GLASS, "normals": Ng}]
    if flagged:
        one = lambda h, w: np.ones((h, w, 3))
        out[0].update(uv=sphere_uv(Vs, TEX_SPHERE[0]), texture=one(4, 5) if uniform else image(4, 5, 31))
        out[1].update(uv=cube_uv(Vc, 41), texture=one(3, 2) if uniform else image(3, 2, 32), orm_texture=one(2, 3) if uniform else orm_image())
        out[2].update(uv=cube_uv(Vb, 42), texture=one(2, 2) if uniform else image(2, 2, 34))
    return out


def corner_uv(ob):
    """The object's "uv" as the library stores it: one pair per triangle corner, rounded to fp32; None without coordinates."""
    if ob.get("uv") is None:
        return None
    return np.asarray(ob["uv"], np.float64)[np.asarray(ob["triangles"], np.int64)].astype(np.float32).astype(np.float64)


def merged(V, T, objects):
    """`path_color_fp64.merged` with each table entry carrying its "corner_uv" and its images, rounded to fp32."""
    Vm, Tm, table = pc.merged(V, T, objects)
    for entry, ob in zip(table, objects):
        entry["corner_uv"] = corner_uv(ob)
        for key in ("texture", "orm_texture"):
            entry[key] = None if ob.get(key) is None else np.asarray(ob[key], np.float32).astype(np.float64)
    return Vm, Tm, table


# the closed form in expectation: `path_light_fp64.furnace_scene`'s box around a camera-facing diffuse quad at constant depth whose
# (s, t) are affine in position and stay inside the texel centres' hull, and whose 5 x 4 texels are affine in their indices: there the
# bilinear fetch is the affine function itself
FURNACE_QUAD = ((0.0, 0.0, -1.2), 0.25)                             # centre, half side
FURNACE_P = (0.9, 0.8, 0.7)
FURNACE_WH = (5, 4)


def furnace_st(x):
    """(s, t) [..., 2] of a point of the quad: affine in x, y, inside [0.5 / w, 1 - 0.5 / w] x [0.5 / h, 1 - 0.5 / h] on the quad."""
    w, h = FURNACE_WH
    c, half = np.asarray(FURNACE_QUAD[0]), FURNACE_QUAD[1]
    q = (np.asarray(x, np.float64)[..., :2] - c[:2]) / (2 * half) + 0.5      # [0, 1]^2 over the quad
    return np.stack([0.5 / w + q[..., 0] * (1 - 1.0 / w), 0.5 / h + q[..., 1] * (1 - 1.0 / h)], -1)


def furnace_texels():
    """[h,w,3], affine in the column i and in the row j counted from the bottom: T = A + B i + C j per channel, inside [0, 1]."""
    w, h = FURNACE_WH
    i, j = np.meshgrid(np.arange(w), (h - 1) - np.arange(h))       # row 0 is the top row
    A, B, C = np.array([0.1, 0.8, 0.3]), np.array([0.2, -0.15, 0.05]), np.array([0.02, -0.05, 0.15])
    return (A + B * i[..., None] + C * j[..., None]).astype(np.float32).astype(np.float64)


def furnace_value(s, t):
    """T(s, t) [..., 3]: the affine function the texels sample, x = s w - 1/2 columns from the left, y = t h - 1/2 rows from the bottom."""
    w, h = FURNACE_WH
    tx = furnace_texels()
    A, B, C = tx[h - 1, 0], tx[h - 1, 1] - tx[h - 1, 0], tx[h - 2, 0] - tx[h - 1, 0]
    return A + B * (np.asarray(s)[..., None] * w - 0.5) + C * (np.asarray(t)[..., None] * h - 0.5)


def furnace_scene():
    """-> the objects: the emitting box and the textured diffuse quad facing the camera."""
    Vb, Tb = pl.box(*pl.FURNACE_BOX, inward=True)
    (cx, cy, cz), half = FURNACE_QUAD
    Vq = np.array([[cx - half, cy - half, cz], [cx + half, cy - half, cz], [cx + half, cy + half, cz], [cx - half, cy + half, cz]])
    Vq = Vq.astype(np.float32).astype(np.float64)
    Tq = np.array([[0, 1, 2], [0, 2, 3]], np.int32)                # outward normal +z: towards the camera
    quad = {"vertices": Vq, "triangles": Tq, "bsdf": {"type": "diffuse", "reflectance": FURNACE_P}, "uv": furnace_st(Vq),
            "texture": furnace_texels()}
    return [{"vertices": Vb, "triangles": Tb, "bsdf": {"type": "area", "radiance": pl.FURNACE_L}}, quad]
