"""fp64 restatement of the path render with rough dielectric inserted objects ("Rough dielectric objects"):
`path_light_fp64.replay_lights` with a fifth object kind, {"type": "roughdielectric", "int_ior", "ext_ior", "alpha"}, rough glass
(Walter et al. 2007 with GGX, the visible normals of Heitz 2018, the separable Smith G).

  * At a vertex n is the outward normal the BSDF shades with (the face normal ng, or the interpolated ns after its three fallbacks),
    s = sign(n . wo), N = s n, eta_it = int_ior / ext_ior entering (s > 0), its inverse leaving, eta_ti = 1 / eta_it.
  * D(h) is GGX about N with 1 - NoH^2 = |N x h|^2; G1(v, h) = 2 / (1 + sqrt(1 + alpha^2 tan^2 theta_v)) where (v . h)(v . N) > 0,
    else 0; D_v(h) = G1(wo) max(wo . h, 0) D(h) / (wo . N); F is the exact Fresnel reflectance at |wo . h|, and 1 - F is formed
    without the difference, as 2 eta ci ct (1 / (ci + eta ct)^2 + 1 / (ct + eta ci)^2): near total internal reflection the literal
    1 - F keeps no digit.
  * Sample (dims 6, 7, 8): h from D_v (dims 7, 8, in the frame of Duff et al. about N); u6 <= F reflects, wi = 2 (wo . h) h - wo,
    pdf = F D_v / (4 wo . h), weight G1(wi), valid where wi . N > 0; else wi = (eta_ti (wo . h) - cos_t) h - eta_ti wo,
    pdf = (1 - F) D_v eta_it^2 |wi . h| / ((wo . h) + eta_it (wi . h))^2, weight G1(wi) eta_ti^2, valid where wi . N < 0.  The vertex
    is never delta.
  * Evaluate (an emitter sample wl; f with its cosine): wl . N > 0: h = normalize(wo + wl), f = F D G / (4 wo . N); else
    h = +-normalize(wo + eta_it wl) with h . N > 0, f = (1 - F) D G |wo . h| |wl . h| / (wo . N ((wo . h) + eta_it (wl . h))^2).
    The pdf is the sampler's for the same pair.
  * A direction w (wi or wl) with (ng . w)(n . w) <= 0 carries nothing.
  * The vertex shades from both sides; its emitter sample is drawn from p + eps ng like every other vertex's, is taken on either side
    of the face, and its shadow ray starts at p + eps ng or p - eps ng, on wl's side.

Every other statement is `path_light_fp64.replay_lights`'s (without a rough object the two functions return the same bits).  The
parameters are rounded to fp32, as the library holds them.  `dtype=np.float32` in `rough_sample` / `rough_eval` is the transcription
whose own rounding sets the host tests' tolerance.  No library code.

The record gains, per pixel: `rough_reflected`, `rough_transmitted` (BSDF samples that carry on), `rough_emitter_reflection_side` (an
emitter sample that arrives with wl on wo's side of the face), `rough_emitter_blocked_inside` (an emitter sample whose shadow ray
starts inside the object, ng . wl < 0, and is stopped), `rough_bsdf_hits_light` (a light's front reached by a ray that a rough vertex
transmitted), `rough_killed_by_normals` (a BSDF or emitter sample dropped by the ng / ns rule)."""
import math

import numpy as np

import path_light_fp64 as pl
import path_oi_fp64 as po
import path_oi_pbr_fp64 as pp
import path_oi_smooth_fp64 as ps
from path_fp64 import FOV, brute, env_texel, mis, pcg, rng_u, texel

SCENE, DIELECTRIC, DIFFUSE, PBR, AREA, ROUGH = pl.SCENE, pl.DIELECTRIC, pl.DIFFUSE, pl.PBR, pl.AREA, 5
f32 = pl.f32


# ---- the BSDF --------------------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a * b).sum(-1)


def _side(p, ng, ns, wo, dt):
    """-> (n: ns after the third fallback, N, eta_it, cos_o)."""
    one = dt(1.0)
    n = np.where((_dot(ns, wo) * _dot(ng, wo) > 0)[:, None], ns, ng)
    no = _dot(n, wo)
    eta = dt(p[0]) / dt(p[1])
    return n, np.where(no > 0, one, -one)[:, None] * n, np.where(no > 0, eta, one / eta), np.abs(no)


def _fresnel(cos_i, eta_it, dt):
    one = dt(1.0)
    eta_ti = one / eta_it
    ct2 = one - (eta_ti * eta_ti) * (one - cos_i * cos_i)
    tir = ~(ct2 > 0)
    ct = np.sqrt(np.where(tir, dt(0.0), ct2))
    with np.errstate(divide="ignore", invalid="ignore"):
        a_s = (cos_i - eta_it * ct) / (cos_i + eta_it * ct)
        a_p = (ct - eta_it * cos_i) / (ct + eta_it * cos_i)
        ka, kb = cos_i + eta_it * ct, ct + eta_it * cos_i
        tr = dt(2.0) * eta_it * cos_i * ct * (one / (ka * ka) + one / (kb * kb))       # 1 - F, in the form that does not cancel near TIR
    return np.where(tir, one, dt(0.5) * (a_s * a_s + a_p * a_p)), ct, np.where(tir, dt(0.0), tr)


def _D(alpha, N, h, dt):
    cr = np.cross(N, h)
    a2 = alpha * alpha
    den = a2 + _dot(cr, cr) * (dt(1.0) - a2)
    return a2 * dt(1.0 / math.pi) / (den * den)


def _G1(alpha, vn, vh, dt):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        c2 = vn * vn
        t2 = np.maximum(dt(1.0) - c2, dt(0.0)) / c2
        g = dt(2.0) / (dt(1.0) + np.sqrt(dt(1.0) + (alpha * alpha) * t2))
    return np.where(vn * vh > 0, g, dt(0.0))


def rough_sample(p, ng, ns, wo, u, dtype=np.float64):
    """p = (int_ior, ext_ior, alpha); ng, ns, wo [N,3]; u [N,3] = dims 6, 7, 8 -> {"wi", "weight" [N], "pdf" [N], "transmitted" [N],
    "reflect" [N]: u6 <= F, "F", "killed" [N]: dropped by the ng / ns rule alone, "decisions" [N,4]: the quantities whose signs or
    order decide a branch (F - u6, wi . N, ng . wi, n . wi), for a comparison across precisions}."""
    dt = dtype
    ng, ns, wo, u = (np.asarray(x, dt) for x in (ng, ns, wo, u))
    alpha, one, zero = dt(p[2]), dt(1.0), dt(0.0)
    n, N, eta_it, cos_o = _side(p, ng, ns, wo, dt)
    eta_ti = one / eta_it
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        sg = np.copysign(one, N[:, 2])
        a = -one / (sg + N[:, 2])
        b = N[:, 0] * N[:, 1] * a
        S = np.stack([one + sg * N[:, 0] * N[:, 0] * a, sg * b, -sg * N[:, 0]], -1)
        T = np.stack([b, sg + N[:, 1] * N[:, 1] * a, -N[:, 1]], -1)
        V = np.stack([alpha * _dot(S, wo), alpha * _dot(T, wo), cos_o], -1)
        V = V / np.sqrt(_dot(V, V))[:, None]
        lensq = V[:, 0] * V[:, 0] + V[:, 1] * V[:, 1]
        il1 = np.where(lensq > 0, one / np.sqrt(np.where(lensq > 0, lensq, one)), zero)
        T1 = np.stack([np.where(lensq > 0, -V[:, 1] * il1, one), np.where(lensq > 0, V[:, 0] * il1, zero), np.zeros_like(lensq)], -1)
        T2 = np.stack([-V[:, 2] * T1[:, 1], V[:, 2] * T1[:, 0], V[:, 0] * T1[:, 1] - V[:, 1] * T1[:, 0]], -1)
        r, ph = np.sqrt(np.maximum(u[:, 1], zero)), dt(2.0 * math.pi) * u[:, 2]
        t1, sm = r * np.cos(ph), dt(0.5) * (one + V[:, 2])
        t2 = (one - sm) * np.sqrt(np.maximum(one - t1 * t1, zero)) + sm * (r * np.sin(ph))
        t3 = np.sqrt(np.maximum(one - t1 * t1 - t2 * t2, zero))
        m = np.stack([alpha * (t1 * T1[:, 0] + t2 * T2[:, 0] + t3 * V[:, 0]), alpha * (t1 * T1[:, 1] + t2 * T2[:, 1] + t3 * V[:, 1]),
                      np.maximum(t2 * T2[:, 2] + t3 * V[:, 2], zero)], -1)
        ml2 = _dot(m, m)
        h = (m[:, 0:1] * S + m[:, 1:2] * T + m[:, 2:3] * N) / np.sqrt(ml2)[:, None]
        woh = _dot(wo, h)
        alive = (cos_o > 0) & (ml2 > 0) & (woh > 0)
        F, ct, Tr = _fresnel(woh, eta_it, dt)
        Dv = _G1(alpha, cos_o, woh, dt) * woh * _D(alpha, N, h, dt) / cos_o
        reflect = u[:, 0] <= F
        wi_r = (dt(2.0) * woh)[:, None] * h - wo
        wi_t = (eta_ti * woh - ct)[:, None] * h - eta_ti[:, None] * wo
        wi = np.where(reflect[:, None], wi_r, wi_t)
        win, wih = _dot(wi, N), _dot(wi, h)
        q = woh + eta_it * wih
        pdf = np.where(reflect, F * Dv / (dt(4.0) * woh), Tr * Dv * (eta_it * eta_it) * np.abs(wih) / (q * q))
        g1 = _G1(alpha, win, wih, dt)
        w = np.where(reflect, np.where(win > 0, g1, zero), np.where(win < 0, g1 * (eta_ti * eta_ti), zero))
        gi, ni = _dot(ng, wi), _dot(n, wi)
        agree = gi * ni > 0
        killed = alive & (w > 0) & (pdf > 0) & ~agree
        w = np.where(alive & agree & (pdf > 0), w, zero)
    dead = ~alive
    wi, pdf = np.where(dead[:, None], zero, wi), np.where(dead, zero, pdf)
    return {"wi": wi, "weight": w, "pdf": pdf, "transmitted": alive & ~reflect, "reflect": reflect, "F": F, "killed": killed,
            "decisions": np.stack([F - u[:, 0], win, gi, ni], -1), "alive": alive}


def rough_eval(p, ng, ns, wo, wl, dtype=np.float64, cosine=True):
    """-> {"f" [N] (with its cosine; `cosine=False`: divided by |wl . N|), "pdf" [N], "killed" [N], "decisions" [N,3]: wl . N, ng . wl,
    n . wl, "cond" [N]: the least of cos_t^2 (a transmission), (wo . h)^2 and (wl . N)^2, the differences and divisors whose smallness
    amplifies rounding}."""
    dt = dtype
    ng, ns, wo, wl = (np.asarray(x, dt) for x in (ng, ns, wo, wl))
    alpha, one, zero = dt(p[2]), dt(1.0), dt(0.0)
    n, N, eta_it, cos_o = _side(p, ng, ns, wo, dt)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        cos_l = _dot(wl, N)
        gl, nl = _dot(ng, wl), _dot(n, wl)
        agree = gl * nl > 0
        reflect = cos_l > 0
        kl = np.where(reflect, one, eta_it)
        h = wo + kl[:, None] * wl
        l2 = _dot(h, h)
        h = h * (np.where(_dot(h, N) > 0, one, -one) / np.sqrt(l2))[:, None]
        woh, wlh = _dot(wo, h), _dot(wl, h)
        alive = (cos_o > 0) & agree & (l2 > 0) & (woh > 0) & (reflect | (wlh < 0))     # a refraction leaves on the far side of the microfacet
        F, ct, Tr = _fresnel(woh, eta_it, dt)
        D, G1o, G1l = _D(alpha, N, h, dt), _G1(alpha, cos_o, woh, dt), _G1(alpha, cos_l, wlh, dt)
        Dv = G1o * woh * D / cos_o
        q = woh + eta_it * wlh
        f = np.where(reflect, F * D * (G1o * G1l) / (dt(4.0) * cos_o), Tr * D * (G1o * G1l) * (woh * np.abs(wlh)) / (cos_o * (q * q)))
        pdf = np.where(reflect, F * Dv / (dt(4.0) * woh), Tr * Dv * (eta_it * eta_it) * np.abs(wlh) / (q * q))
        ok = alive & (pdf > 0)
        f, pdf = np.where(ok, f, zero), np.where(ok, pdf, zero)
        if not cosine:
            f = np.where(ok, f / np.abs(cos_l), zero)
        cond = np.minimum(np.where(reflect, one, ct * ct), np.minimum(woh * woh, cos_l * cos_l))
    return {"f": f, "pdf": pdf, "killed": (cos_o > 0) & ~agree, "decisions": np.stack([cos_l, gl, nl], -1), "cond": cond}


def rough_params(bsdf):
    return f32([bsdf.get("int_ior", 1.49), bsdf.get("ext_ior", 1.000277), bsdf.get("alpha", 0.1)])


# ---- the walk ----------------------------------------------------------------------------------------------------------------------------
def replay_rough(o64, V, T, a, r, m, env, tab, H, W, max_depth, seed, objects=(), sample=0, closest=None, lanes=None, emitter_sample=True):
    """`path_light_fp64.replay_lights` where an object's bsdf may be of type "roughdielectric" -> (L, record).  `emitter_sample=False`:
    the same estimator's other half alone, no emitter sample at any vertex and every MIS weight 1 (its expectation is the same)."""
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
           "rough_bsdf_hits_light": z(), "rough_killed_by_normals": z()}

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
    """`path_light_fp64.replay_mean` over `replay_rough` -> [len(seeds), H, W, 3]."""
    maps = (np.zeros((H, W, 3), np.float32), np.ones((H, W, 1), np.float32), np.zeros((H, W, 1), np.float32))
    out = np.zeros((len(seeds), H, W, 3))
    pix, smp = np.meshgrid(np.arange(H * W), np.arange(spp), indexing="ij")
    for c0 in range(0, len(seeds), chunk):
        sd = np.asarray(seeds[c0:c0 + chunk])
        lanes = (np.tile(pix.reshape(-1), sd.size), np.repeat(sd, pix.size), np.tile(smp.reshape(-1), sd.size))
        L, _ = replay_rough(None, V, T, *maps, env, tab, H, W, max_depth, 0, objects, lanes=lanes, emitter_sample=emitter_sample)
        out[c0:c0 + sd.size] = L.reshape(sd.size, H, W, spp, 3).mean(3)
    return out


# ---- the shared test scenes ----------------------------------------------------------------------------------------------------------
FROSTED_02 = {"type": "roughdielectric", "int_ior": 1.49, "ext_ior": 1.000277, "alpha": 0.2}
FROSTED_005 = {"type": "roughdielectric", "int_ior": 1.49, "ext_ior": 1.000277, "alpha": 0.05}
ROUGH_SPHERE = ((0.08, 0.12, -1.10), 0.09)                         # `path_light_fp64`'s glass sphere, frosted
ROUGH_CUBE = ((0.13, -0.12, -1.36), 0.16, (0.0, 0.5, 0.0))         # its PBR cube's place, a little larger: the lamp's housing
INNER_QUAD_HALF = 0.03
CLEAR_SPHERE = ((-0.13, 0.12, -1.20), 0.07)
merged = ps.merged
RECORD_KEYS = ("rough_reflected", "rough_transmitted", "rough_emitter_reflection_side", "rough_emitter_blocked_inside", "rough_bsdf_hits_light",
               "rough_killed_by_normals")


def inner_quad(centre, half):
    """A small emitter quad at `centre` facing the camera (+z) -> (V, T)."""
    c = np.asarray(centre, np.float64)
    return pl.quad([c + (-half, -half, 0.0), c + (half, -half, 0.0), c + (half, half, 0.0), c + (-half, half, 0.0)])


def table_scene():
    """The GPU parity scene's table, in front of a depth mesh at z <= -1.6: a smooth-flagged rough-glass icosphere (alpha 0.2), a flat
    rough-glass cube (alpha 0.05) that encloses a small emitter quad, a diffuse cube and a clear-glass icosphere."""
    Vs, Ts, Ns = ps.icosphere(*ROUGH_SPHERE, 1)
    Vc, Tc = po.cube(*ROUGH_CUBE)
    Vq, Tq = inner_quad(ROUGH_CUBE[0], INNER_QUAD_HALF)
    Vd, Td = po.cube(*pl.DIFFUSE_CUBE)
    Vg, Tg, Ng = ps.icosphere(*CLEAR_SPHERE, 1)
    return [{"vertices": Vs, "triangles": Ts, "bsdf": FROSTED_02, "normals": Ns},
            {"vertices": Vc, "triangles": Tc, "bsdf": FROSTED_005},
            {"vertices": Vq, "triangles": Tq, "bsdf": pl.QUAD_LIGHT},
            {"vertices": Vd, "triangles": Td, "bsdf": po.DIFFUSE_08},
            {"vertices": Vg, "triangles": Tg, "bsdf": po.GLASS, "normals": Ng}]


FURNACE_C = 0.7
FURNACE_SPHERE = ((0.02, -0.01, -1.2), 0.2)
FURNACE_LAMP = {"type": "area", "radiance": (9.0, 8.0, 6.0)}


def furnace_scene(lamp):
    """A closed rough-glass icosphere (flat faces, alpha 0.2) before a depth mesh no ray meets; `lamp`: with a small two-sided lamp
    (two emitter quads back to back) at its centre."""
    Vi, Ti, _ = ps.icosphere(*FURNACE_SPHERE, 1)
    out = [{"vertices": Vi, "triangles": Ti, "bsdf": FROSTED_02}]
    if lamp:
        Vq, Tq = inner_quad(FURNACE_SPHERE[0], 0.05)
        out.append({"vertices": Vq, "triangles": Tq, "bsdf": FURNACE_LAMP})
        out.append({"vertices": Vq - (0.0, 0.0, 1e-3), "triangles": Tq[:, ::-1].copy(), "bsdf": FURNACE_LAMP})
    return out
