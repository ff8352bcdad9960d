"""What the path render traces, built on the host: an inserted object's BSDF and per-corner data checked and laid out as the library
takes them (`object_bsdf`, `merge_scene`, `merge_objects`), the light tables of a merged mesh, the BVH and the envmap's sampling tables
(DESIGN.md section 1.4)."""
import ctypes
import time
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence

import numpy as np

from .path_abi import (BSDF_AREA, BSDF_DIELECTRIC, BSDF_DIFFUSE, BSDF_PBR, BSDF_ROUGH_DIELECTRIC, MAX_OBJECTS, MEDIUM_MAX_G, NODE_BYTES, OBJECT_COLORED,
                       OBJECT_MEDIUM, OBJECT_PHOTO, OBJECT_SMOOTH, OBJECT_TEXTURED, PBR_DEFAULTS, PBR_MIN_ROUGHNESS, ROUGH_MIN_ALPHA, ROUGH_MIN_CONTRAST, TEXTURE_MAX_SIDE,
                       TEXTURE_MAX_UV, TRI_BYTES, PathLights, PathObject, PathObjectMedium, PathObjectPbr, PathObjectTex, PathXform, _ptr, _ref, _table_ptrs,
                       _uncolored, check, load, symbol)


def build_bvh(vertices: np.ndarray, triangles: np.ndarray, n_scene_tri: Optional[int] = None) -> Dict[str, object]:
    """Host BVH of a triangle mesh: {"nodes" uint8 [n_nodes*64], "tris" uint8 [T*48], "n_nodes", "depth", "n_leaves", "build_s"}.
    `n_scene_tri`: triangles from this index on belong to inserted meshes and keep their winding (`matpbr_path_bvh_build_objects`);
    None = every triangle is the depth mesh's (`matpbr_path_bvh_build`)."""
    lib = load()
    V = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    T = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
    cap = ctypes.c_long(0)
    check(lib.matpbr_path_bvh_size(T.shape[0], _ref(cap)), "matpbr_path_bvh_size")
    nodes = np.zeros(cap.value * NODE_BYTES, dtype=np.uint8)
    tris = np.zeros(max(T.shape[0], 1) * TRI_BYTES, dtype=np.uint8)
    n_nodes, depth, n_leaves = ctypes.c_long(0), ctypes.c_int(0), ctypes.c_long(0)
    t0 = time.perf_counter()
    outs = (_ref(n_nodes), _ref(depth), _ref(n_leaves))
    name, own = ("matpbr_path_bvh_build", ()) if n_scene_tri is None else ("matpbr_path_bvh_build_objects", (int(n_scene_tri),))
    code = getattr(lib, name)(_ptr(V), V.shape[0], _ptr(T), T.shape[0], *own, _ptr(nodes), cap.value, _ptr(tris), *outs)
    build_s = time.perf_counter() - t0
    check(code, name)
    return {"nodes": nodes[: n_nodes.value * NODE_BYTES].copy(), "tris": tris, "n_nodes": n_nodes.value, "depth": depth.value,
            "n_leaves": n_leaves.value, "build_s": build_s}


def build_bvh_grafted(vertices: np.ndarray, triangles: np.ndarray, n_scene_tri: int, reach: Optional[float] = None,
                      n_scene_vert: Optional[int] = None) -> Dict[str, object]:
    """The grafted host BVH of a merged mesh ("Moving inserted objects"; `matpbr_path_bvh_build_grafted`): node 0's
    slot 0 is the depth mesh's subtree (triangles below `n_scene_tri`), slot 1 the inserted triangles' -> `build_bvh`'s dict plus
    {"rest_tris" uint8 [n_object_tri*48]: the object triangles' records, the rest pose; "node_level" int32 [n_object_nodes];
    "first_object_node", "n_object_nodes", "object_depth", "pad": 1e-6 of "reach", the largest coordinate magnitude of the mesh and of
    `reach`, which announces the farthest pose a later move will ask for}.  `n_scene_vert`: the depth mesh's vertex count (the merged
    mesh lists its vertices first; the scene side is padded by their scale); None: the vertices the scene's triangles name, which is
    the same count unless the depth mesh ends in vertices no triangle uses."""
    lib = load()
    V = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    T = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
    n_scene, n_obj = int(n_scene_tri), T.shape[0] - int(n_scene_tri)
    if n_scene < 1 or n_obj < 1:
        raise ValueError(f"a grafted BVH needs the scene's triangles and inserted ones behind them: {T.shape[0]} triangles, n_scene_tri {n_scene_tri}")
    nv_scene = int(T[:n_scene].max()) + 1 if n_scene_vert is None else int(n_scene_vert)
    far = 0.0 if reach is None else float(reach)
    if not (np.isfinite(far) and far >= 0):
        raise ValueError(f"reach must be finite and >= 0, got {reach}")
    cap = 1 + max(1, n_scene) + max(1, n_obj)
    nodes = np.zeros(cap * NODE_BYTES, dtype=np.uint8)
    tris, rest = np.zeros(T.shape[0] * TRI_BYTES, dtype=np.uint8), np.zeros(n_obj * TRI_BYTES, dtype=np.uint8)
    level = np.zeros(cap, dtype=np.int32)
    n_nodes, depth, n_leaves, first, obj_depth, pad = (ctypes.c_long(0), ctypes.c_int(0), ctypes.c_long(0), ctypes.c_long(0), ctypes.c_int(0),
                                                       ctypes.c_float(0))
    t0 = time.perf_counter()
    code = symbol("matpbr_path_bvh_build_grafted", lib)(_ptr(V), V.shape[0], nv_scene, _ptr(T), T.shape[0], n_scene, far, _ptr(nodes), cap, _ptr(tris), _ptr(rest),
                                                        _ptr(level), _ref(n_nodes), _ref(depth), _ref(n_leaves), _ref(first), _ref(obj_depth), _ref(pad))
    build_s = time.perf_counter() - t0
    check(code, "matpbr_path_bvh_build_grafted")
    n_object_nodes = n_nodes.value - first.value
    return {"nodes": nodes[: n_nodes.value * NODE_BYTES].copy(), "tris": tris, "n_nodes": n_nodes.value, "depth": depth.value,
            "n_leaves": n_leaves.value, "build_s": build_s, "rest_tris": rest, "node_level": level[:n_object_nodes].copy(),
            "first_object_node": first.value, "n_object_nodes": n_object_nodes, "object_depth": obj_depth.value, "pad": pad.value,
            "reach": max(far, float(np.abs(V).max()))}


XFORM_KEYS = ("scale", "rotate", "translate", "pivot")


def rotation(axis, deg: float) -> np.ndarray:
    """The rotation by `deg` degrees about `axis` (any length but zero), 3 x 3 float64 (Rodrigues); ValueError when bad."""
    try:
        a, ang = np.asarray(axis, dtype=np.float64), float(deg)
    except (TypeError, ValueError):
        raise ValueError(f"a rotation needs an axis of 3 numbers and an angle in degrees, got {axis!r} and {deg!r}") from None
    if a.shape != (3,) or not np.isfinite(a).all() or not np.isfinite(ang):
        raise ValueError(f"a rotation needs a finite axis of 3 numbers and a finite angle, got {axis!r} and {deg!r}")
    ln = float(np.linalg.norm(a))
    if not ln > 0:
        raise ValueError("a rotation's axis must not be zero")
    x, y, z = a / ln
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    th = np.radians(ang)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def similarity(transform: Optional[dict], pivot=None) -> tuple:
    """A placement {"scale": s (1), "rotate": 3 x 3 or {"axis", "deg"} (none), "translate" (0), "pivot" (`pivot`, else 0)} ->
    (R [3,3], s, t [3], c [3]) in float64, p' = R (s (p - c)) + c + t; None is the identity about `pivot`.  ValueError for an unknown key,
    a value of the wrong shape, a non-finite one, a scale that is not positive or a zero axis.  Whether R is a rotation is the library's
    to say (`check_xforms`)."""
    tr = {} if transform is None else transform
    if not isinstance(tr, dict):
        raise ValueError(f"a transform must be a dict with keys of {XFORM_KEYS}, got {type(tr).__name__}")
    extra = sorted(set(tr) - set(XFORM_KEYS))
    if extra:
        raise ValueError(f"transform: unknown key {extra[0]!r} (known: {', '.join(repr(k) for k in XFORM_KEYS)})")
    rot = tr.get("rotate")
    if rot is None:
        R = np.eye(3)
    elif isinstance(rot, dict):
        extra = sorted(set(rot) - {"axis", "deg"})
        if extra or "axis" not in rot or "deg" not in rot:
            raise ValueError(f"transform: 'rotate' must be a 3 x 3 matrix or {{'axis': [x, y, z], 'deg': a}}, got {rot!r}")
        R = rotation(rot["axis"], rot["deg"])
    else:
        try:
            R = np.array(rot, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"transform: 'rotate' must be a 3 x 3 matrix or {{'axis': [x, y, z], 'deg': a}}, got {rot!r}") from None
        if R.shape != (3, 3):
            raise ValueError(f"transform: 'rotate' must be 3 x 3, got shape {R.shape}")
    try:
        s = float(tr.get("scale", 1.0))
        t = np.array(tr.get("translate", (0.0, 0.0, 0.0)), dtype=np.float64)
        c = np.array(tr.get("pivot") if tr.get("pivot") is not None else (pivot if pivot is not None else (0.0, 0.0, 0.0)), dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"transform: 'scale' must be a number, 'translate' and 'pivot' 3 numbers, got {tr!r}") from None
    if t.shape != (3,) or c.shape != (3,):
        raise ValueError(f"transform: 'translate' and 'pivot' must be 3 numbers, got shapes {t.shape} and {c.shape}")
    if not (np.isfinite(R).all() and np.isfinite(s) and np.isfinite(t).all() and np.isfinite(c).all()):
        raise ValueError(f"transform: every value must be finite, got {tr!r}")
    if not s > 0:
        raise ValueError(f"transform: 'scale' must be positive, got {s}")
    return R, s, t, c


def apply_similarity(sim: tuple, points: np.ndarray, vectors: bool = False) -> np.ndarray:
    """p' = R (s (p - c)) + c + t of points [..., 3] in float64; `vectors`: R p alone (normals)."""
    R, s, t, c = sim
    P = np.asarray(points, dtype=np.float64)
    return P @ R.T if vectors else (s * (P - c)) @ R.T + (c + t)


def xform_records(sims: Sequence[tuple]):
    """The similarities as the library takes them: a PathXform array (fp32)."""
    return (PathXform * len(sims))(*(PathXform((ctypes.c_float * 9)(*R.reshape(-1)), s, (ctypes.c_float * 3)(*t), (ctypes.c_float * 3)(*c))
                                     for R, s, t, c in sims))


def check_xforms(records) -> None:
    """ValueError unless the library takes every record (`matpbr_path_xform_check_host`): finite, scale > 0, R's rows orthonormal to
    1e-5, det R > 0.  Names the first record it refuses."""
    fn = symbol("matpbr_path_xform_check_host")
    for k in range(len(records)):
        if fn(ctypes.cast(ctypes.byref(records[k]), ctypes.c_void_p), 1) != 0:
            x = records[k]
            raise ValueError(f"transform of object {k}: every value must be finite, the scale positive and 'rotate' a rotation (rows orthonormal "
                             f"to 1e-5, no mirror), got R = {[round(v, 6) for v in x.R]}, scale = {x.s}")


def pose_extent(sim: tuple, lo: np.ndarray, hi: np.ndarray) -> float:
    """The largest coordinate magnitude of the box [lo, hi] under a similarity: that of its eight corners, which bounds the magnitude of
    everything inside the box (a coordinate is linear, so its extremes over the moved box lie at corners)."""
    corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])], dtype=np.float64)
    return float(np.abs(apply_similarity(sim, corners)).max())


def env_tables(env: np.ndarray) -> Dict[str, object]:
    """Emitter-sampling tables of an envmap [He,We,3] (fp64 on the host, stored fp32): row_cdf [He+1], col_cdf [He,We+1], pdf [He,We]."""
    E = np.ascontiguousarray(env, dtype=np.float32)
    He, We = E.shape[:2]
    row, col, pdf = np.empty(He + 1, np.float32), np.empty((He, We + 1), np.float32), np.empty((He, We), np.float32)
    total = ctypes.c_double(0.0)
    check(load().matpbr_path_env_tables(_ptr(E), He, We, _ptr(row), _ptr(col), _ptr(pdf), _ref(total)),
          "matpbr_path_env_tables")
    return {"row_cdf": row, "col_cdf": col, "pdf": pdf, "total": total.value}


MEDIUM_KEYS = ("sigma_a", "scatter", "g", "color", "at")


def object_medium(bsdf: dict) -> Optional[tuple]:
    """The "medium" of a glass object's bsdf dict ("Media inside glass") -> (sigma_a0, sigma_a1, sigma_a2, sigma_s,
    g) in float64, None without the key.  Either {"sigma_a": scalar or 3 values (0), "scatter": sigma_s (0), "g": g (0)}, every coefficient
    per scene unit, finite and >= 0, |g| <= 0.99; or {"color": scalar or 3 values in (0, 1], "at": d > 0, "scatter", "g"}: the colour white
    light has after the distance d inside the object, sigma_a = -ln(color) / d.  ValueError for another bsdf type than 'dielectric' and
    'roughdielectric', for both forms at once, for an unknown sub-key or a value out of range."""
    med = bsdf.get("medium") if isinstance(bsdf, dict) else None
    if med is None:
        return None
    if bsdf.get("type") not in ("dielectric", "roughdielectric"):
        raise ValueError(f"medium: a medium fills a 'dielectric' or a 'roughdielectric' object; a {bsdf.get('type')!r} object takes none (drop 'medium')")
    if not isinstance(med, dict):
        raise ValueError(f"medium must be a dict with keys of {MEDIUM_KEYS}, got {type(med).__name__}")
    extra = sorted(set(med) - set(MEDIUM_KEYS))
    if extra:
        raise ValueError(f"medium: unknown key {extra[0]!r} (known: {', '.join(repr(k) for k in MEDIUM_KEYS)})")
    friendly, plain = "color" in med or "at" in med, "sigma_a" in med
    if friendly and plain:
        raise ValueError("medium: give either 'sigma_a' or 'color' with 'at', not both")
    try:
        if friendly:
            if "color" not in med or "at" not in med:
                raise ValueError("medium: 'color' and 'at' go together: the colour of white light after the distance 'at' inside the object")
            col, at = np.asarray(med["color"], dtype=np.float64), float(med["at"])
            if col.shape not in ((), (1,), (3,)) or not ((col > 0) & (col <= 1)).all():
                raise ValueError(f"medium: color must be a scalar or 3 values in (0, 1], got {med['color']!r}")
            if not (np.isfinite(at) and at > 0):
                raise ValueError(f"medium: 'at' must be finite and > 0, got {med['at']!r}")
            sa = -np.log(np.broadcast_to(col, (3,))) / at + 0.0          # + 0.0: a white channel gives +0, not -0
        else:
            sa = np.asarray(med.get("sigma_a", 0.0), dtype=np.float64)
            if sa.shape not in ((), (1,), (3,)):
                raise ValueError(f"medium: sigma_a must be a scalar or 3 values, got shape {sa.shape}")
            sa = np.broadcast_to(sa, (3,))
        ss, g = float(med.get("scatter", 0.0)), float(med.get("g", 0.0))
    except TypeError:
        raise ValueError(f"medium: every value must be a number or 3 numbers, got {med!r}") from None
    with np.errstate(over="ignore"):
        ok = np.isfinite(np.asarray([*sa, ss], np.float32)).all()    # the bounds as the library sees them: the record is fp32
    if not (ok and (sa >= 0).all() and ss >= 0):
        raise ValueError(f"medium: sigma_a and scatter must be finite and >= 0, got {sa.tolist()} and {ss}")
    if not abs(np.float32(g)) <= np.float32(MEDIUM_MAX_G):
        raise ValueError(f"medium: g must lie in [-{MEDIUM_MAX_G}, {MEDIUM_MAX_G}], got {g}")
    return (*(float(x) for x in sa), ss, g)


PHOTO_TYPES = ("diffuse", "pbr", "roughdielectric")


def object_photo(ob: dict) -> bool:
    """The "photo" key of an inserted object ("Reflected in inserted objects") -> whether the see-through chain
    passes the object's vertices; False without the key.  ValueError for a value that is not a bool, and for True on an object whose
    bsdf type is 'area' (it has no BSDF) or 'dielectric' (the see-through rule holds for it already)."""
    photo = ob.get("photo") if isinstance(ob, dict) else None
    if photo is None:
        return False
    if not isinstance(photo, (bool, np.bool_)):
        raise ValueError(f"photo must be true or false, got {photo!r}")
    kind = ob["bsdf"].get("type") if isinstance(ob.get("bsdf"), dict) else None
    if photo and kind not in PHOTO_TYPES:
        why = "has no BSDF" if kind == "area" else "is see-through already (see_through shows the photograph behind it)" if kind == "dielectric" else "takes none"
        raise ValueError(f"photo: the photograph is reflected in a 'diffuse', a 'pbr' or a 'roughdielectric' object; a {kind!r} object {why} (drop 'photo')")
    return bool(photo)


def object_bsdf(bsdf: dict) -> tuple:
    """{"type": "dielectric", "int_ior", "ext_ior"} | {"type": "diffuse", "reflectance"} -> (kind, (p0, p1, p2));
    {"type": "pbr", "albedo": scalar or 3 values (0.8), "roughness" (0.5), "metallic" (0)} -> (BSDF_PBR, (a0, a1, a2, r, m));
    {"type": "area", "radiance": scalar or 3 values, finite and >= 0 (1)} -> (BSDF_AREA, (r, g, b)): an area light.
    {"type": "roughdielectric", "int_ior" (1.49), "ext_ior" (1.000277), "alpha" (0.1): the GGX width in [0.02, 1]} ->
    (BSDF_ROUGH_DIELECTRIC, (int_ior, ext_ior, alpha)): rough glass; the indices' ratio stays at least 0.01 away from 1.
    A dielectric or roughdielectric dict may carry "medium" (`object_medium` returns its record; the kind returned here stays bare); on
    another type it is refused.  ValueError when bad."""
    kind = bsdf.get("type") if isinstance(bsdf, dict) else None
    object_medium(bsdf)
    if kind == "roughdielectric":
        try:
            p = (float(bsdf.get("int_ior", 1.49)), float(bsdf.get("ext_ior", 1.000277)), float(bsdf.get("alpha", 0.1)))
        except (TypeError, ValueError):
            raise ValueError(f"roughdielectric: int_ior, ext_ior and alpha must be numbers, got {bsdf!r}") from None
        q = np.asarray(p, np.float32)                    # the bounds as the library sees them: the table is fp32
        if not (q[0] > 0 and q[1] > 0 and np.isfinite(q[:2]).all()):
            raise ValueError(f"roughdielectric: int_ior and ext_ior must be positive and finite, got {p[0]}, {p[1]}")
        with np.errstate(over="ignore", under="ignore", divide="ignore"):
            eta = q[0] / q[1]
            inv = np.float32(1) / eta
        if not (eta > 0 and np.isfinite(eta) and np.isfinite(inv) and abs(eta - np.float32(1)) >= np.float32(ROUGH_MIN_CONTRAST)):
            raise ValueError(f"roughdielectric: int_ior / ext_ior must differ from 1 by at least {ROUGH_MIN_CONTRAST}, got {p[0]} / {p[1]}")
        if not np.float32(ROUGH_MIN_ALPHA) <= q[2] <= 1:
            raise ValueError(f"roughdielectric: alpha must lie in [{ROUGH_MIN_ALPHA}, 1], got {p[2]}")
        return BSDF_ROUGH_DIELECTRIC, p
    if kind == "dielectric":
        p = (float(bsdf.get("int_ior", 1.49)), float(bsdf.get("ext_ior", 1.000277)), 0.0)
        if not (p[0] > 0 and p[1] > 0 and np.isfinite(p[:2]).all()):
            raise ValueError(f"dielectric: int_ior and ext_ior must be positive, got {p[0]}, {p[1]}")
        return BSDF_DIELECTRIC, p
    if kind == "diffuse":
        rho = np.broadcast_to(np.asarray(bsdf.get("reflectance", 0.5), dtype=np.float64), (3,))
        if not ((rho >= 0) & (rho <= 1)).all():
            raise ValueError(f"diffuse: reflectance must lie in [0, 1], got {rho.tolist()}")
        return BSDF_DIFFUSE, tuple(float(x) for x in rho)
    if kind == "pbr":
        alb = np.asarray(bsdf.get("albedo", PBR_DEFAULTS["albedo"]), dtype=np.float64)
        if alb.shape not in ((), (1,), (3,)):
            raise ValueError(f"pbr: albedo must be a scalar or 3 values, got shape {alb.shape}")
        alb = np.broadcast_to(alb, (3,))
        if not ((alb >= 0) & (alb <= 1)).all():
            raise ValueError(f"pbr: albedo must lie in [0, 1], got {alb.tolist()}")
        rough, metal = float(bsdf.get("roughness", PBR_DEFAULTS["roughness"])), float(bsdf.get("metallic", PBR_DEFAULTS["metallic"]))
        # the bounds as the library sees them: the record is fp32 (0.07 is not a float; its nearest one lies above it)
        if not np.float32(PBR_MIN_ROUGHNESS) <= np.float32(rough) <= 1:
            raise ValueError(f"pbr: roughness must lie in [{PBR_MIN_ROUGHNESS}, 1], got {rough}")
        if not 0 <= metal <= 1:
            raise ValueError(f"pbr: metallic must lie in [0, 1], got {metal}")
        return BSDF_PBR, (*(float(x) for x in alb), rough, metal)
    if kind == "area":
        try:
            rad = np.asarray(bsdf.get("radiance", 1.0), dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"area: radiance must be a number or 3 numbers, got {bsdf.get('radiance')!r}") from None
        if rad.shape not in ((), (1,), (3,)):
            raise ValueError(f"area: radiance must be a scalar or 3 values, got shape {rad.shape}")
        rad = np.broadcast_to(rad, (3,))
        if not (np.isfinite(rad).all() and (rad >= 0).all() and np.isfinite(rad.astype(np.float32)).all()):
            raise ValueError(f"area: radiance must be finite and >= 0, got {rad.tolist()}")
        return BSDF_AREA, tuple(float(x) for x in rad)
    raise ValueError(f"object bsdf type must be 'dielectric', 'diffuse', 'pbr', 'area' or 'roughdielectric', got {kind!r}")


def _corner_normals(k: int, ob: dict, Vo: np.ndarray, To: np.ndarray) -> np.ndarray:
    """Object k's "normals" [Nv,3], normalised in fp64 and expanded to one record per triangle corner [Nt,3,3]; ValueError when bad."""
    No = np.asarray(ob["normals"], dtype=np.float64)
    if No.shape != Vo.shape:
        raise ValueError(f"object {k}: normals must be [Nv,3] = {Vo.shape}, one per vertex, got {No.shape}")
    if not np.isfinite(No).all():
        raise ValueError(f"object {k}: normals must be finite")
    ln = np.linalg.norm(No, axis=-1)
    used = np.zeros(Vo.shape[0], bool)
    used[To.reshape(-1)] = True
    if (used & ~(ln > 0)).any():
        raise ValueError(f"object {k}: the normal of vertex {int(np.nonzero(used & ~(ln > 0))[0][0])}, which a triangle uses, has zero length")
    return (No / np.where(ln > 0, ln, 1.0)[:, None])[To]


def light_tables(V: np.ndarray, T: np.ndarray, table: Sequence[PathObject], records: Optional[Sequence[PathObjectPbr]] = None,
                 symbol=symbol) -> Optional[dict]:
    """The light tables of a merged mesh (`merge_objects`' V, T, table and PBR records), built by the library on the host ->
    {"header": PathLights, "tris" float32 [n_light_tri, 3, 4] = (v0, 0) (e1, 0) (e2, 0) of every light triangle in input order,
    "cdf" float32 [n_light_tri]: per light the cumulative area / its area, the last entry exactly 1}; None when no object is of kind
    BSDF_AREA.  PathError where the library refuses the table (a light of total area 0 among the reasons).  `symbol`: the lookup of
    the library's function (`PathTracer` passes its module's own, the one its other lookups go through)."""
    if not any(t.kind & ~OBJECT_SMOOTH == BSDF_AREA for t in table):
        return None
    table = _uncolored(table)
    Vv = np.ascontiguousarray(V, dtype=np.float64).reshape(-1, 3)
    Tt = np.ascontiguousarray(T, dtype=np.int32).reshape(-1, 3)
    tab, rec = _table_ptrs(table, records)
    fn = symbol("matpbr_path_light_tables")
    head, n = PathLights(), ctypes.c_long(0)
    hp, np_ = _ref(head), _ref(n)
    check(fn(_ptr(Vv), Vv.shape[0], _ptr(Tt), Tt.shape[0], tab, len(table), rec, hp, None, None, 0, np_), "matpbr_path_light_tables")
    tris, cdf = np.zeros((n.value, 3, 4), np.float32), np.zeros(n.value, np.float32)
    check(fn(_ptr(Vv), Vv.shape[0], _ptr(Tt), Tt.shape[0], tab, len(table), rec, hp, _ptr(tris), _ptr(cdf), n.value, np_), "matpbr_path_light_tables")
    return {"header": head, "tris": tris, "cdf": cdf}


def _corner_colors(k: int, ob: dict, kind: int, Vo: np.ndarray, To: np.ndarray) -> np.ndarray:
    """Object k's "colors" [Nv,3] (linear RGB, finite, in [0, 1]) expanded to one record per triangle corner [Nt,3,3]; ValueError when bad."""
    if kind not in (BSDF_DIFFUSE, BSDF_PBR):
        raise ValueError(f"object {k}: vertex colours tint a 'diffuse' or a 'pbr' object; a {ob['bsdf'].get('type')!r} object takes none (drop 'colors')")
    Co = np.asarray(ob["colors"], dtype=np.float64)
    if Co.shape != Vo.shape:
        raise ValueError(f"object {k}: colors must be [Nv,3] = {Vo.shape}, one per vertex, got {Co.shape}")
    bad = ~(np.isfinite(Co) & (Co >= 0) & (Co <= 1)).all(-1)
    if bad.any():
        v = int(np.nonzero(bad)[0][0])
        raise ValueError(f"object {k}: the colour of vertex {v} must be finite and lie in [0, 1], got {Co[v].tolist()}")
    return Co[To]


def _corner_uv(k: int, ob: dict, Vo: np.ndarray, To: np.ndarray) -> np.ndarray:
    """Object k's "uv" [Nv,2] (finite, |.| <= TEXTURE_MAX_UV) expanded to one record per triangle corner [Nt,3,2]; ValueError when bad."""
    Uo = np.asarray(ob["uv"], dtype=np.float64)
    if Uo.shape != (Vo.shape[0], 2):
        raise ValueError(f"object {k}: uv must be [Nv,2] = {(Vo.shape[0], 2)}, one (s, t) per vertex, got {Uo.shape}")
    bad = ~(np.isfinite(Uo) & (np.abs(Uo) <= TEXTURE_MAX_UV)).all(-1)
    if bad.any():
        v = int(np.nonzero(bad)[0][0])
        raise ValueError(f"object {k}: the texture coordinate of vertex {v} must be finite with |s|, |t| <= {TEXTURE_MAX_UV:g}, got {Uo[v].tolist()}")
    return Uo[To]


def _texture_image(k: int, key: str, img) -> np.ndarray:
    """Object k's image ob[key] [h,w,3] (linear, finite, in [0, 1]) as texels [h w, 4] float32 = (r, g, b, 0), row 0 the top row;
    ValueError naming the texel when bad."""
    A = np.asarray(img, dtype=np.float64)
    if A.ndim != 3 or A.shape[2] != 3 or not (1 <= A.shape[0] <= TEXTURE_MAX_SIDE and 1 <= A.shape[1] <= TEXTURE_MAX_SIDE):
        raise ValueError(f"object {k}: {key} must be [h,w,3] with h, w in [1, {TEXTURE_MAX_SIDE}], got {A.shape}")
    bad = ~(np.isfinite(A) & (A >= 0) & (A <= 1)).all(-1)
    if bad.any():
        i, j = (int(x[0]) for x in np.nonzero(bad))
        raise ValueError(f"object {k}: {key}: texel (row {i}, column {j}) must be finite and lie in [0, 1], got {A[i, j].tolist()}")
    out = np.zeros((A.shape[0] * A.shape[1], 4), np.float32)
    out[:, :3] = A.reshape(-1, 3)
    return out


def _object_textures(k: int, ob: dict, kind: int, first: int):
    """Object k's images -> (its PathObjectTex with the images placed from texel `first` on, [texel arrays]); ValueError where the
    object may carry none, or carries "uv" and images the wrong way round."""
    have = [key for key in ("texture", "orm_texture") if ob.get(key) is not None]
    if not have and ob.get("uv") is None:
        return PathObjectTex(), []
    if kind not in (BSDF_DIFFUSE, BSDF_PBR):
        raise ValueError(f"object {k}: an image textures a 'diffuse' or a 'pbr' object; a {ob['bsdf'].get('type')!r} object takes none "
                         f"(drop 'uv', 'texture' and 'orm_texture')")
    if not have:
        raise ValueError(f"object {k}: 'uv' without an image: give 'texture' (or 'orm_texture' on a pbr object), or drop 'uv'")
    if ob.get("uv") is None:
        raise ValueError(f"object {k}: {have[0]!r} without 'uv': an image needs one (s, t) per vertex")
    if "orm_texture" in have and kind != BSDF_PBR:
        raise ValueError(f"object {k}: 'orm_texture' holds roughness and metallic, which a 'diffuse' object does not have (a 'pbr' one does)")
    rec, texels = PathObjectTex(), []
    for key, name in (("texture", "base"), ("orm_texture", "orm")):
        if key in have:
            tx = _texture_image(k, key, ob[key])
            h, w = np.asarray(ob[key]).shape[:2]
            setattr(rec, name + "_first", first)
            setattr(rec, name + "_w", w)
            setattr(rec, name + "_h", h)
            texels.append(tx)
            first += tx.shape[0]
    return rec, texels


COUNT_KEYS = ("n_smooth_objects", "n_pbr_objects", "n_lights", "n_rough_objects", "n_colored_objects", "n_textured_objects")


@dataclass
class MergedScene:
    """The depth mesh with the inserted meshes appended, as `merge_scene` lays it out for the library."""
    V: np.ndarray                       # [Nv,3] float64
    T: np.ndarray                       # [Nt,3] int32; object k's triangles follow the scene's in the order given
    table: List[PathObject]             # object k's kind (with its OBJECT_ flags), its range of T, its parameters
    obj_nrm: Optional[np.ndarray]       # corner normals [Nt - scene's Nt, 3, 3] float32 (zero for a flat object); None: no object is smooth
    records: List[PathObjectPbr]        # one per object (zero unless its kind is BSDF_PBR)
    lights: Optional[dict]              # `light_tables` of the merged mesh; None: no object is an area light, or they were not asked for
    obj_col: Optional[np.ndarray]       # corner colours [Nt - scene's Nt, 3, 3] float32 (zero without "colors"); None: no object is coloured
    textures: Optional[tuple]           # (obj_uv [Nt - scene's Nt, 3, 2] float32, [PathObjectTex] one per object, texels [n, 4] float32); None: no object is textured
    counts: Dict[str, int]              # the objects of each kind, under `PathTracer.stats`' keys (COUNT_KEYS)
    media: Optional[List[PathObjectMedium]] = None   # one per object (zero unless it holds a medium); None: no object holds one


def merge_scene(vertices: np.ndarray, triangles: np.ndarray, objects: Sequence[dict], lights: bool = False, symbol=symbol) -> MergedScene:
    """The depth mesh with `objects` appended, every object checked (ValueError when bad; `merge_objects` says what an object may
    carry).  `lights`: build the light tables (`symbol`: `light_tables`')."""
    V = [np.asarray(vertices, dtype=np.float64).reshape(-1, 3)]
    T = [np.asarray(triangles, dtype=np.int32).reshape(-1, 3)]
    if len(objects) > MAX_OBJECTS:
        raise ValueError(f"at most {MAX_OBJECTS} inserted objects, got {len(objects)}")
    table: List[PathObject] = []
    corner: Dict[str, List[np.ndarray]] = {"normals": [], "colors": [], "uv": []}   # per object [Nt,3,c]: zero where it carries none (the kernel never reads those)
    tex: List[PathObjectTex] = []
    texels: List[np.ndarray] = []
    records: List[PathObjectPbr] = []
    media: List[PathObjectMedium] = []
    counts = dict.fromkeys(COUNT_KEYS, 0)
    nv, nt = V[0].shape[0], T[0].shape[0]
    for k, ob in enumerate(objects):
        bare, p = object_bsdf(ob.get("bsdf"))
        med = object_medium(ob.get("bsdf"))
        try:
            photo = object_photo(ob)
        except ValueError as e:
            raise ValueError(f"object {k}: {e}") from None
        media.append(PathObjectMedium((ctypes.c_float * 3)(*med[:3]), med[3], med[4]) if med is not None else PathObjectMedium())
        records.append(PathObjectPbr((ctypes.c_float * 3)(*p[:3]), p[3], p[4]) if bare == BSDF_PBR else PathObjectPbr())
        if bare == BSDF_PBR:
            p = (0.0, 0.0, 0.0)
        Vo = np.asarray(ob["vertices"], dtype=np.float64)
        To = np.asarray(ob["triangles"])
        if Vo.ndim != 2 or Vo.shape[1] != 3 or To.ndim != 2 or To.shape[1] != 3 or To.shape[0] == 0:
            raise ValueError(f"object {k}: vertices must be [Nv,3] and triangles [Nt,3] (Nt > 0), got {Vo.shape} and {To.shape}")
        if not np.isfinite(Vo).all():
            raise ValueError(f"object {k}: vertices must be finite")
        if not np.issubdtype(To.dtype, np.integer) or To.min() < 0 or To.max() >= Vo.shape[0]:
            raise ValueError(f"object {k}: triangle indices must be integers in [0, {Vo.shape[0]})")
        if ob.get("normals") is not None and bare == BSDF_AREA:
            raise ValueError(f"object {k}: an area light has no shading normals: it emits from its faces (drop 'normals')")
        smooth, colored = ob.get("normals") is not None, ob.get("colors") is not None
        corner["normals"].append(_corner_normals(k, ob, Vo, To) if smooth else np.zeros((To.shape[0], 3, 3)))
        corner["colors"].append(_corner_colors(k, ob, bare, Vo, To) if colored else np.zeros((To.shape[0], 3, 3)))
        rec, images = _object_textures(k, ob, bare, sum(x.shape[0] for x in texels))
        tex.append(rec)
        texels += images
        corner["uv"].append(_corner_uv(k, ob, Vo, To) if images else np.zeros((To.shape[0], 3, 2)))
        kind = bare | (OBJECT_SMOOTH if smooth else 0) | (OBJECT_COLORED if colored else 0) | (OBJECT_TEXTURED if images else 0) | \
            (OBJECT_MEDIUM if med is not None else 0) | (OBJECT_PHOTO if photo else 0)
        for key, one in zip(COUNT_KEYS, (smooth, bare == BSDF_PBR, bare == BSDF_AREA, bare == BSDF_ROUGH_DIELECTRIC, colored, bool(images))):
            counts[key] += one
        V.append(Vo)
        T.append((To.astype(np.int64) + nv).astype(np.int32))
        table.append(PathObject(kind, nt, To.shape[0], (ctypes.c_float * 3)(*p)))
        nv, nt = nv + Vo.shape[0], nt + To.shape[0]
    Vm, Tm = np.concatenate(V), np.concatenate(T)
    joined = lambda key, count: np.ascontiguousarray(np.concatenate(corner[key]), dtype=np.float32) if counts[count] else None
    return MergedScene(Vm, Tm, table, joined("normals", "n_smooth_objects"), records, light_tables(Vm, Tm, table, records, symbol) if lights else None,
                       joined("colors", "n_colored_objects"),
                       (joined("uv", "n_textured_objects"), tex, np.ascontiguousarray(np.concatenate(texels))) if texels else None, counts,
                       media if any(t.kind & OBJECT_MEDIUM for t in table) else None)


def merge_objects(vertices: np.ndarray, triangles: np.ndarray, objects: Sequence[dict], normals: bool = False, pbr: bool = False,
                  lights: bool = False, colors: bool = False, textures: bool = False):
    """The depth mesh with the inserted meshes appended -> (V [Nv,3] float64, T [Nt,3] int32, [PathObject]).  Object k's triangles
    follow the scene's in the order given; its ids are its range of T.  An object may carry "normals" [Nv,3] (per vertex, outward, any
    length): it is smooth ("Smooth inserted objects"), its kind carries OBJECT_SMOOTH, and with `normals=True`
    a fourth value follows, the corner normals [Nt - scene's Nt, 3, 3] float32 of every inserted triangle (unit length, normalised in
    fp64; zero for the objects without normals, which the kernel never reads), or None when no object is smooth.  With `pbr=True`
    one more value follows, the [n_objects] PathObjectPbr records (zero for the objects of another kind, which the kernel never
    reads); a table entry of kind BSDF_PBR has p = 0.  With `lights=True` one more value follows, `light_tables` of the merged mesh
    (None when no object is an area light).  An area light ({"type": "area"}) has kind BSDF_AREA and p = its radiance; with "normals"
    it is refused.  A diffuse or pbr object may carry "colors" [Nv,3] (per vertex, linear RGB, finite, in [0, 1]; DESIGN.md section 1.4,
    "Vertex-coloured inserted objects"): its kind carries OBJECT_COLORED, and with `colors=True` one more value follows, last, the
    corner colours [Nt - scene's Nt, 3, 3] float32 of every inserted triangle (zero for the objects without colours, which the kernel
    never reads), or None when no object has "colors".  On a dielectric, area or roughdielectric object "colors" is refused.  A diffuse
    or pbr object may carry "uv" [Nv,2] (per vertex, finite, |.| <= 64) with "texture" [h,w,3] (base colour: linear, finite, in [0, 1],
    row 0 the top row) and, on a pbr object, "orm_texture" [h,w,3] (glTF's occlusion, roughness, metallic; DESIGN.md section 1.4,
    "Textured inserted objects"): its kind carries OBJECT_TEXTURED, and with `textures=True` one more value follows, last,
    (obj_uv [Nt - scene's Nt, 3, 2] float32, [PathObjectTex] one per object, texels [n, 4] float32), or None when no object is textured.
    "uv" without an image, an image without "uv", an image on another kind and "orm_texture" on a diffuse object are refused.
    The values are `merge_scene`'s record, projected onto what the five flags select."""
    s = merge_scene(vertices, triangles, objects, lights=lights)
    chosen = ((normals, s.obj_nrm), (pbr, s.records), (lights, s.lights), (colors, s.obj_col), (textures, s.textures))
    return (s.V, s.T, s.table, *(value for want, value in chosen if want))
