"""The colour rule of the fp64 restatement of the path render ("Vertex-coloured inserted objects"); the walk
that applies it, and the order of the rules, is `path_objects_fp64.replay_objects`.

  * An object of type "diffuse" or "pbr" may carry "colors" [Nv,3], linear RGB in [0, 1]; the table entry holds them as the library
    does, one triple per triangle corner, rounded to fp32 ("corner_colors").
  * At a hit on such an object u, v are Moller-Trumbore's (`path_oi_smooth_fp64.barycentrics`, the ones the smooth normal uses) and
    c = clip(c0 + u (c1 - c0) + v (c2 - c0), 0, 1) per channel.
  * diffuse: reflectance = p (.) c; pbr: albedo = a (.) c, roughness and metallic the record's.  Nothing else changes: neither
    sampler depends on the colour, so the object walks the paths of its uncoloured twin.

With every corner colour (1, 1, 1) the walk returns the bits of the table without colours.  No library code.

The record gains `colored_camera` [N,8] (the camera ray's first hit lies on coloured object k) and `colored_indirect` (a later vertex
ray lands on a coloured object, whether max_depth lets it shade there or not)."""
import numpy as np

import path_light_fp64 as pl
import path_oi_fp64 as po
import path_oi_smooth_fp64 as ps
import path_rough_fp64 as pr


def vertex_color(cc, u, v):
    """c = clip(c0 + u (c1 - c0) + v (c2 - c0), 0, 1) for corner colours cc [N,3,3] and barycentrics u, v [N] -> [N,3]; a u, v that is
    not a number gives 0, as the library's clamp does."""
    with np.errstate(invalid="ignore", over="ignore"):
        c = cc[:, 0] + u[:, None] * (cc[:, 1] - cc[:, 0]) + v[:, None] * (cc[:, 2] - cc[:, 0])
    return np.clip(np.where(np.isnan(c), 0.0, c), 0.0, 1.0)


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
