"""The PBR rule of the fp64 restatement of the path render ("PBR inserted objects"); the walk that applies it,
and the order of the rules, is `path_objects_fp64.replay_objects`.  A third object kind, {"type": "pbr", "albedo", "roughness",
"metallic"}, whose vertices are the depth mesh's vertices under "Shading normals" on the constants of the object instead of on a texel:

  * one-sided about the outward face normal ng (ng . wo <= 0 ends the path with nothing added); no texel is read;
  * ns = ng on a flat object, the interpolated corner normal with its three fallbacks on a smooth one;
  * emitter sample (dims 2-5): needs pdf_e > 0 and ng . wl > 0; f and pdf_b from the fp64 BSDF about ns; a shadow ray where some
    f[c] > 0; the power heuristic;
  * BSDF sample (dims 6, 7, 8) about ns: the reference's lobe choice and weight (the oracle's sample_brdf); never a delta event; a
    sample with ng . wi <= 0 ends the path, on a flat object too; the next ray starts at p + eps ng.

The object's constants are rounded to fp32, as the library's record holds them.

The record gains, per pixel: `pbr_vertex` (a vertex on a PBR object), `pbr_smooth_vertex` (on a smooth one), `pbr_below_ng` (a BSDF
sample ended by ng . wi <= 0; `pbr_below_ng_carrying`: one whose weight about ns was not zero already, which only a smooth object
has), `pbr_emitter_below_ng` (an emitter sample the BSDF about ns would have carried, refused by
ng . wl <= 0); `blocked_by_object` and `fallback` as before."""
import numpy as np

import path_oi_fp64 as po
import path_oi_smooth_fp64 as ps

SCENE, DIELECTRIC, DIFFUSE, PBR = po.SCENE, po.DIELECTRIC, po.DIFFUSE, 3

PBR_DEFAULTS = {"albedo": 0.8, "roughness": 0.5, "metallic": 0.0}


def pbr_constants(bsdf):
    """(a [3], r, m) of a "pbr" dict in fp64, rounded to fp32 first: the values the library's record holds."""
    f32 = lambda x: np.asarray(x, np.float64).astype(np.float32).astype(np.float64)
    a = np.broadcast_to(f32(bsdf.get("albedo", PBR_DEFAULTS["albedo"])), (3,))
    return a, float(f32(bsdf.get("roughness", PBR_DEFAULTS["roughness"]))), float(f32(bsdf.get("metallic", PBR_DEFAULTS["metallic"])))


# ---- the shared test scenes ----------------------------------------------------------------------------------------------------------
METAL = {"type": "pbr", "albedo": (0.95, 0.64, 0.54), "roughness": 0.07, "metallic": 1.0}     # copper-coloured, at the roughness floor
PLASTIC = {"type": "pbr", "albedo": 0.5, "roughness": 0.6, "metallic": 0.0}
METAL_CENTRE, METAL_RADIUS = (0.096, 0.017, -1.30), 0.103
GLASS_CENTRE, GLASS_RADIUS = (-0.083, 0.07, -1.123), 0.104
PBR_CUBE = ((-0.01, 0.17, -1.40), 0.11, (0.5, -0.4, 0.3))
DIFFUSE_CUBE = ((-0.04, -0.15, -1.32), 0.12, (-0.3, 0.7, 0.2))


def table_scene():
    """All four object code paths in one table, in front of a depth mesh at z <= -1.6: a smooth metal icosphere and a smooth glass
    icosphere of level 1 (80 triangles each: at their silhouettes the interpolated normal turns away from the viewer while the face
    still looks at it, and a mirror reflection about it can leave below the face), a flat PBR cube and a flat diffuse cube."""
    Vm, Tm, Nm = ps.icosphere(METAL_CENTRE, METAL_RADIUS, 1)
    Vc, Tc = po.cube(*PBR_CUBE)
    Vg, Tg, Ng = ps.icosphere(GLASS_CENTRE, GLASS_RADIUS, 1)
    Vd, Td = po.cube(*DIFFUSE_CUBE)
    return [{"vertices": Vm, "triangles": Tm, "bsdf": METAL, "normals": Nm},
            {"vertices": Vc, "triangles": Tc, "bsdf": PLASTIC},
            {"vertices": Vg, "triangles": Tg, "bsdf": po.GLASS, "normals": Ng},
            {"vertices": Vd, "triangles": Td, "bsdf": po.DIFFUSE_08}]


def quad(z=-1.5):
    """The unit square of two triangles across the whole view at depth z, wound so that e1 x e2 points at the camera -> (V [4,3],
    T [2,3]): as a depth mesh the builder keeps the winding, as an inserted object it faces the camera.  Its edges are (1, 0, 0),
    (1, 1, 0) and (0, 1, 0): e1 x e2 = (0, 0, 1) without rounding, in any precision."""
    V = np.array([[-0.5, -0.5, z], [0.5, -0.5, z], [0.5, 0.5, z], [-0.5, 0.5, z]], np.float64)
    return V, np.array([[0, 1, 2], [0, 2, 3]], np.int32)


FAR_TRIANGLE = (np.array([[50.0, 50.0, -1.0], [50.001, 50.0, -1.0], [50.0, 50.001, -1.0]]), np.array([[0, 1, 2]], np.int32))   # out of view
