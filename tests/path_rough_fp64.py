"""The rough-glass rule of the fp64 restatement of the path render ("Rough dielectric objects"); the walk that
applies it, and the order of the rules, is `path_objects_fp64.replay_objects`.  A fifth object kind, {"type": "roughdielectric",
"int_ior", "ext_ior", "alpha"}, rough glass (Walter et al. 2007 with GGX, the visible normals of Heitz 2018, the separable Smith G).

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

The parameters are rounded to fp32, as the library holds them.  `dtype=np.float32` in `rough_sample` / `rough_eval` is the
transcription whose own rounding sets the host tests' tolerance.  No library code.

The record gains, per pixel: `rough_reflected`, `rough_transmitted` (BSDF samples that carry on), `rough_emitter_reflection_side` (an
emitter sample that arrives with wl on wo's side of the face), `rough_emitter_blocked_inside` (an emitter sample whose shadow ray
starts inside the object, ng . wl < 0, and is stopped), `rough_bsdf_hits_light` (a light's front reached by a ray that a rough vertex
transmitted), `rough_killed_by_normals` (a BSDF or emitter sample dropped by the ng / ns rule)."""
import math

import numpy as np

import path_light_fp64 as pl
import path_oi_fp64 as po
import path_oi_smooth_fp64 as ps

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


# ---- the shared test scenes ----------------------------------------------------------------------------------------------------------
FROSTED_02 = {"type": "roughdielectric", "int_ior": 1.49, "ext_ior": 1.000277, "alpha": 0.2}
FROSTED_005 = {"type": "roughdielectric", "int_ior": 1.49, "ext_ior": 1.000277, "alpha": 0.05}
ROUGH_SPHERE = ((0.08, 0.12, -1.10), 0.09)                         # `path_light_fp64`'s glass sphere, frosted
ROUGH_CUBE = ((0.13, -0.12, -1.36), 0.16, (0.0, 0.5, 0.0))         # its PBR cube's place, a little larger: the lamp's housing
INNER_QUAD_HALF = 0.03
CLEAR_SPHERE = ((-0.13, 0.12, -1.20), 0.07)
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
