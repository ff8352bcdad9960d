"""The area-light rule of the fp64 restatement of the path render ("Emissive inserted objects"); the walk that
applies it, and the order of the rules, is `path_objects_fp64.replay_objects`.  A fourth object kind, {"type": "area", "radiance":
scalar or 3 values}, an area light.

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

Radiance and area are rounded to fp32, as the library holds them.

The record gains, per pixel: `light_sample_arrives`, `light_sample_blocked` (a light sample whose shadow ray an object or the mesh
stops), `bsdf_hits_light_front` / `bsdf_hits_light_back` (a ray sampled at a non-delta vertex), `light_through_glass` (a front hit
after a delta vertex), `light_at_depth0`, `env_sample` (an envmap emitter sample taken while lights compete)."""
import math

import numpy as np

import path_oi_fp64 as po
import path_oi_pbr_fp64 as pp
import path_oi_smooth_fp64 as ps
from path_fp64 import FOV, brute

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
