"""The smooth-normal rule of the fp64 restatement of the path render ("Smooth inserted objects"); the walk
that applies it, and the order of the rules, is `path_objects_fp64.replay_objects`.  An object of the table may carry "corner_normals"
[n_tri,3,3] (one normal per corner of each of its triangles, in input order); at a hit on it the BSDF shades with the normal
interpolated at the hit point and the face normal keeps the geometry.

The record gains, per pixel: `smooth_transmitted` (a transmitted vertex on a smooth dielectric), `smooth_diffuse` (a vertex on a
smooth diffuse object), `redo` (a dielectric event about ns disagreed with the geometry and was redone about ng) and `fallback`
(one of the three fallbacks to the face normal fired), the last also split by cause in `fallback_cause` [N,3]."""
import numpy as np

import path_oi_fp64 as po

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
