"""The path render's routines on the CPU, lane by lane: each function hands rows of inputs to the `*_host` entry of libmatpbr_path.so
that runs the code the kernel runs, and returns fresh arrays.  Only the tests call them: they are what the fp64 restatements and the
device are compared against."""
import ctypes
from typing import Dict, Optional, Sequence

import numpy as np

from .path_abi import (BSDF_PBR, BSDF_ROUGH_DIELECTRIC, PathObject, PathObjectTex, PathTransEdit, _aligned_texels, _ptr, _ref, _rows, _same_rows,
                       _table_ptrs, _tex_ptrs, _uncolored, check, symbol)
from .path_scene import object_bsdf


def _call(name: str, *args) -> None:
    """The library's `name` over `args`, an array standing for its address; PathError when it fails."""
    check(symbol(name)(*(_ptr(x) if isinstance(x, np.ndarray) else x for x in args)), name)


def _out(N: int, *cols: int) -> tuple:
    """Fresh float32 outputs of N rows: [N] for cols = 1, else [N, cols]."""
    return tuple(np.empty(N if c == 1 else (N, c), np.float32) for c in cols)


def _trace(name: str, bvh, origins, dirs, tmin, tmax, *own) -> tuple:
    o, d = _rows(origins, 3), _rows(dirs, 3)
    t, k = np.empty(o.shape[0], np.float32), np.empty(o.shape[0], np.int32)
    _call(name, bvh["nodes"], bvh["tris"], o, d, o.shape[0], tmin, tmax, t, k, *own)
    return t, k


def trace_host(bvh: Dict[str, object], origins: np.ndarray, dirs: np.ndarray, tmin: float = 0.0, tmax: float = 3.0e38):
    """Closest hit on the CPU with the kernel's routine -> (t [N] float32, tmax where missed; triangle index [N] int32, -1 = miss)."""
    return _trace("matpbr_path_trace_host", bvh, origins, dirs, tmin, tmax)


def trace_scene_host(bvh: Dict[str, object], origins: np.ndarray, dirs: np.ndarray, n_scene_tri: int, any: bool = False, tmin: float = 0.0,
                     tmax: float = 3.0e38):
    """`trace_host` over the triangles of id < `n_scene_tri` alone, the differential render's second walk: a triangle of a larger id is
    skipped before its test.  `any`: the shadow rays' traversal, which returns the first triangle it finds (t is then its distance,
    not the closest).  With `n_scene_tri` at the mesh's triangle count and `any` off it is `trace_host`, bit for bit."""
    return _trace("matpbr_path_trace_scene_host", bvh, origins, dirs, tmin, tmax, int(n_scene_tri), int(bool(any)))


def moved_light_areas(lights: dict, records) -> list:
    """A light's area under its object's similarity, (float)((double) area_rest s s), for every light of `light_tables`' dict at rest."""
    head = lights["header"]
    return [float(np.float32(float(head.area[l]) * float(records[head.object[l]].s) * float(records[head.object[l]].s))) for l in range(head.n_lights)]


def objects_move_host(bvh: Dict[str, object], table: Sequence[PathObject], n_scene_tri: int, records, rest_nrm: Optional[np.ndarray] = None,
                      lights: Optional[dict] = None) -> dict:
    """`PathTracer.move_objects` on the CPU with the routines the kernels run ("Moving inserted objects"):
    `build_bvh_grafted`'s dict, `merge_objects`' table, `xform_records`' poses, the rest corner normals and the rest `light_tables` ->
    {"nodes", "tris": moved copies (the dict is `bvh` with them, so `trace_host` takes it), "obj_nrm", "light_tris": moved copies or None,
    "area": the lights' areas}.  The rest pose is not written.  PathError where the library refuses."""
    out = dict(bvh)
    out["nodes"], out["tris"] = np.array(bvh["nodes"], copy=True), np.array(bvh["tris"], copy=True)
    n_obj = bvh["rest_tris"].size // 48
    nrm = None if rest_nrm is None else np.ascontiguousarray(rest_nrm, dtype=np.float32)
    out["obj_nrm"] = None if nrm is None else np.zeros_like(nrm)
    ltris, head, n_light = (None, None, 0) if lights is None else _light_args(lights)
    moved_l = None if lights is None else _aligned_texels(np.zeros((3 * n_light, 4), np.float32)).reshape(-1)   # 16-byte aligned records
    tab, _ = _table_ptrs(table)
    _call("matpbr_path_objects_move_host", out["nodes"], out["tris"], bvh["rest_tris"], int(n_scene_tri), n_obj, bvh["first_object_node"],
          bvh["n_object_nodes"], np.ascontiguousarray(bvh["node_level"], dtype=np.int32), bvh["object_depth"], tab, len(table),
          ctypes.cast(records, ctypes.c_void_p), float(bvh["pad"]), nrm, out["obj_nrm"], ltris, moved_l, n_light, head)
    out["light_tris"] = None if lights is None else moved_l.reshape(-1, 3, 4).copy()
    out["area"] = [] if lights is None else moved_light_areas(lights, records)
    return out


def through_chain_host(bvh: Dict[str, object], table: Sequence[PathObject], n_scene_tri: int, H: int, W: int, pixels, seeds, samples,
                       max_depth: int, obj_nrm: Optional[np.ndarray] = None, fov_x_deg: float = 35.0) -> dict:
    """The camera chain of `PathTracer.render_diff_through` on the CPU with the routines the kernel runs ("Seen
    through glass"): lane l is sample samples[l] of pixel pixels[l] (a flat index) under seeds[l], over the host BVH of the merged
    mesh and `merge_objects`' table (`obj_nrm`: its corner normals, where an object is smooth) -> {"depth" [N] int32: the depth at
    which the chain lands on the depth mesh's front, -1 where the sample is not see-through; "texel" [N] int32: the texel the landing
    point projects to; "thr" [N,3]: the chain's throughput; "o", "d" [N,3]: the ray that lands}."""
    pix = np.ascontiguousarray(pixels, dtype=np.int32).reshape(-1)
    sd = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint32), pix.shape))
    smp = np.ascontiguousarray(np.broadcast_to(np.asarray(samples, dtype=np.int32), pix.shape))
    tab, _ = _table_ptrs(table)
    nrm = None if obj_nrm is None else np.ascontiguousarray(obj_nrm, dtype=np.float32)
    N = pix.size
    depth, texel = np.empty(N, np.int32), np.empty(N, np.int32)
    thr, o, d = _out(N, 3, 3, 3)
    _call("matpbr_path_through_chain_host", bvh["nodes"], bvh["tris"], int(H), int(W), float(fov_x_deg), int(max_depth), tab, len(table), nrm,
          int(n_scene_tri), pix, sd, smp, N, depth, texel, thr, o, d)
    return {"depth": depth, "texel": texel, "thr": thr, "o": o, "d": d}


def reflect_chain_host(bvh: Dict[str, object], table: Sequence[PathObject], n_scene_tri: int, H: int, W: int, pixels, seeds, samples,
                       max_depth: int, obj_nrm: Optional[np.ndarray] = None, records=None, fov_x_deg: float = 35.0) -> dict:
    """`through_chain_host` for the chain that also passes the objects carrying OBJECT_PHOTO ("Reflected in
    inserted objects"; `matpbr_path_reflect_chain_host`): the same lanes and outputs, `thr` now with the flagged vertices' BSDF weights.
    `records`: `merge_objects`' PathObjectPbr records, needed where a flagged object is of kind BSDF_PBR.  On a table without the flag it
    gives `through_chain_host`'s bits."""
    pix = np.ascontiguousarray(pixels, dtype=np.int32).reshape(-1)
    sd = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, dtype=np.uint32), pix.shape))
    smp = np.ascontiguousarray(np.broadcast_to(np.asarray(samples, dtype=np.int32), pix.shape))
    tab, rec = _table_ptrs(table, records)
    nrm = None if obj_nrm is None else np.ascontiguousarray(obj_nrm, dtype=np.float32)
    N = pix.size
    depth, texel = np.empty(N, np.int32), np.empty(N, np.int32)
    thr, o, d = _out(N, 3, 3, 3)
    _call("matpbr_path_reflect_chain_host", bvh["nodes"], bvh["tris"], int(H), int(W), float(fov_x_deg), int(max_depth), tab, len(table), nrm,
          int(n_scene_tri), rec, pix, sd, smp, N, depth, texel, thr, o, d)
    return {"depth": depth, "texel": texel, "thr": thr, "o": o, "d": d}


def env_sample_host(tables: Dict[str, object], u: np.ndarray):
    """The render's emitter sampler on the CPU: u [N,4] -> (dir [N,3], pdf [N], texel [N] = row*We + col)."""
    U = _rows(u, 4)
    He, We = tables["pdf"].shape
    d, p = _out(U.shape[0], 3, 1)
    k = np.empty(U.shape[0], np.int32)
    _call("matpbr_path_env_sample_host", tables["row_cdf"], tables["col_cdf"], tables["pdf"], He, We, U, U.shape[0], d, p, k)
    return d, p, k


def _light_args(lights: dict) -> tuple:
    """A 16-byte aligned copy of the records and the pointers of the two CPU entry points' first arguments."""
    n = lights["cdf"].shape[0]
    raw = np.zeros(n * 12 + 4, np.float32)
    off = (-raw.ctypes.data % 16) // 4
    tris = raw[off:off + n * 12]
    tris[:] = np.asarray(lights["tris"], np.float32).reshape(-1)
    return tris, _ref(lights["header"]), n


def light_sample_host(lights: dict, have_env: bool, po: np.ndarray, u: np.ndarray):
    """The kernel's emitter choice and light sampler on the CPU: `light_tables`' dict, whether the envmap is emitter 0, spawn points po
    [N,3] and u [N,4] = dims 2-5 -> {"emitter" [N] (the index among the n_e emitters), "u_re" [N], "record" [N] (the light triangle;
    -1 for the envmap), "y" [N,3], "wl" [N,3], "dist" [N], "pdf" [N] (0 where the light faces away or dist = 0)}."""
    P, U = _rows(po, 3), _rows(u, 4)
    N = _same_rows("po and u must have the same rows", P, U)
    tris, hp, n = _light_args(lights)
    cdf = np.ascontiguousarray(lights["cdf"], dtype=np.float32)
    o = {"emitter": np.empty(N, np.int32), "u_re": np.empty(N, np.float32), "record": np.empty(N, np.int32), "y": np.empty((N, 3), np.float32),
         "wl": np.empty((N, 3), np.float32), "dist": np.empty(N, np.float32), "pdf": np.empty(N, np.float32)}
    _call("matpbr_path_light_sample_host", hp, tris, cdf, n, int(bool(have_env)), P, U, N, *o.values())
    return o


def light_pdf_host(lights: dict, have_env: bool, light: np.ndarray, record: np.ndarray, o: np.ndarray, d: np.ndarray):
    """The hit side's pdf on the CPU with the kernel's routine: rays o, d [N,3] (unit length) that land on light triangle record [N] of
    light [N] -> (t [N], pdf [N] = t^2 / (A (n_l . -d) n_e), 0 on the back)."""
    O, D = _rows(o, 3), _rows(d, 3)
    Lg, Rc = np.ascontiguousarray(light, dtype=np.int32).reshape(-1), np.ascontiguousarray(record, dtype=np.int32).reshape(-1)
    N = _same_rows("light, record, o and d must have the same rows", O, D, Lg, Rc)
    tris, hp, n = _light_args(lights)
    t, pdf = _out(N, 1, 1)
    _call("matpbr_path_light_pdf_host", hp, tris, n, int(bool(have_env)), Lg, Rc, O, D, N, t, pdf)
    return t, pdf


def object_lookup_host(table: Sequence[PathObject], records, ids: np.ndarray):
    """The kernel's table lookup on the CPU: `merge_objects`' table and PBR records, triangle ids [N] -> (kind [N] int32, 0 where the
    id lies in no range, the smooth flag kept; a [N,3], r [N], m [N]: a PBR object's record, 0 for every other id)."""
    I = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
    tab, rec = _table_ptrs(table, records)
    kind = np.empty(I.size, np.int32)
    a, r, m = _out(I.size, 3, 1, 1)
    _call("matpbr_path_object_lookup_host", tab, len(table), rec, I, I.size, kind, a, r, m)
    return kind, a, r, m


def _sampled_object(bsdf: dict) -> PathObject:
    """`object_bsdf` for the object samplers' host twins, which know the dielectric and the diffuse BSDF (a PBR object is sampled by the
    depth mesh's device routines, which have no host twin)."""
    kind, p = object_bsdf(bsdf)
    if kind == BSDF_PBR:
        raise ValueError("the object samplers on the CPU know 'dielectric' and 'diffuse'; a 'pbr' object samples with MatDiffBSDF's device code")
    if kind == BSDF_ROUGH_DIELECTRIC:
        raise ValueError("the object samplers on the CPU know 'dielectric' and 'diffuse'; a 'roughdielectric' object samples with rough_sample_host")
    return PathObject(kind, 0, 0, (ctypes.c_float * 3)(*p))


def _rough_object(bsdf: dict) -> PathObject:
    kind, p = object_bsdf(bsdf)
    if kind != BSDF_ROUGH_DIELECTRIC:
        raise ValueError(f"rough_sample_host and rough_eval_host take a 'roughdielectric' bsdf, got {bsdf.get('type')!r}")
    return PathObject(kind, 0, 0, (ctypes.c_float * 3)(*p))


def _normal_rows(x, N: int) -> np.ndarray:
    return np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float32).reshape(-1, 3), (N, 3)))


def _sample(name: str, ob: PathObject, normals, wo, u) -> tuple:
    """An object sampler `name` over wo, u [N,3] -> (wi [N,3], weight [N,3], pdf [N], flags [N]).  `normals`: the normal arguments, each
    [3] or [N,3], between the object and wo."""
    WO, U = _rows(wo, 3), _rows(u, 3)
    N = _same_rows(f"wo and u must have the same rows, got {WO.shape[0]} and {U.shape[0]}", WO, U)
    wi, w, pdf = _out(N, 3, 3, 1)
    flags = np.empty(N, np.int32)
    _call(name, _ref(ob), *(normals(N)), WO, U, N, wi, w, pdf, flags)
    return wi, w, pdf, flags


def object_sample_host(bsdf: dict, n: np.ndarray, wo: np.ndarray, u: np.ndarray):
    """The kernel's BSDF sampler of an inserted object on the CPU: outward face normal n [3], wo [N,3], u [N,3] (dims 6, 7, 8) ->
    (wi [N,3], weight [N,3], pdf [N], flags [N]: bit 0 delta, bit 1 transmitted)."""
    return _sample("matpbr_path_object_sample_host", _sampled_object(bsdf), lambda N: (np.ascontiguousarray(n, dtype=np.float32).reshape(3),), wo, u)


def object_sample_shading_host(bsdf: dict, ng: np.ndarray, ns: np.ndarray, wo: np.ndarray, u: np.ndarray):
    """`object_sample_host` at vertices with a face normal ng [N,3] (or [3]) and a shading normal ns [N,3] (or [3]), as the kernel
    samples a smooth object: the third fallback, the sample about ns, the dielectric's redo about ng, weight 0 below ng ->
    (wi [N,3], weight [N,3], pdf [N], flags [N])."""
    return _sample("matpbr_path_object_sample_shading_host", _sampled_object(bsdf), lambda N: (_normal_rows(ng, N), _normal_rows(ns, N)), wo, u)


def rough_sample_host(bsdf: dict, ng: np.ndarray, ns: np.ndarray, wo: np.ndarray, u: np.ndarray):
    """The kernel's sampler of a rough dielectric object on the CPU: face normal ng [N,3] (or [3]), shading normal ns [N,3] (or [3];
    ng on a flat object), wo [N,3], u [N,3] (dims 6, 7, 8) -> (wi [N,3], weight [N,3], pdf [N], flags [N]: bit 1 transmitted)."""
    return _sample("matpbr_path_rough_sample_host", _rough_object(bsdf), lambda N: (_normal_rows(ng, N), _normal_rows(ns, N)), wo, u)


def rough_eval_host(bsdf: dict, ng: np.ndarray, ns: np.ndarray, wo: np.ndarray, wl: np.ndarray):
    """The kernel's evaluation of a rough dielectric object on the CPU, as an emitter sample takes it: directions wl [N,3] ->
    (f [N,3], with its cosine; pdf [N], the density `rough_sample_host` gives wl)."""
    ob = _rough_object(bsdf)
    WO, WL = _rows(wo, 3), _rows(wl, 3)
    N = _same_rows(f"wo and wl must have the same rows, got {WO.shape[0]} and {WL.shape[0]}", WO, WL)
    f, pdf = _out(N, 3, 1)
    _call("matpbr_path_rough_eval_host", _ref(ob), _normal_rows(ng, N), _normal_rows(ns, N), WO, WL, N, f, pdf)
    return f, pdf


def _at_hits(name: str, tri, corner, what: str, cols: int, o, d, *own, outs=(1, 1, 3)) -> tuple:
    """The entry `name` over triangle records tri [N,3,3] = (v0, e1, e2), per-corner data `what` [N,3,cols] and rays o, d [N,3], then N,
    its `own` arguments and fresh outputs of `outs` columns, which are returned."""
    TR = np.ascontiguousarray(tri, dtype=np.float32).reshape(-1, 3, 3)
    CN = np.ascontiguousarray(corner, dtype=np.float32).reshape(-1, 3, cols)
    O, D = _rows(o, 3), _rows(d, 3)
    N = _same_rows(f"tri, {what}, o and d must have the same rows", TR, CN, O, D)
    out = _out(N, *outs)
    _call(name, TR, CN, O, D, N, *own, *out)
    return out


def object_normal_host(tri: np.ndarray, nrm: np.ndarray, o: np.ndarray, d: np.ndarray):
    """The kernel's shading normal of a smooth object on the CPU: triangle records tri [N,3,3] = (v0, e1, e2), corner normals nrm
    [N,3,3], rays o, d [N,3] -> (u [N], v [N], ns [N,3]); ns after the first two fallbacks (not finite or zero, ns . ng <= 0)."""
    return _at_hits("matpbr_path_object_normal_host", tri, nrm, "nrm", 3, o, d)


def object_color_host(tri: np.ndarray, col: np.ndarray, o: np.ndarray, d: np.ndarray):
    """The kernel's colour of a vertex-coloured object on the CPU: triangle records tri [N,3,3] = (v0, e1, e2), corner colours col
    [N,3,3], rays o, d [N,3] -> (u [N], v [N], c [N,3] = clamp(c0 + u (c1 - c0) + v (c2 - c0), 0, 1))."""
    return _at_hits("matpbr_path_object_color_host", tri, col, "col", 3, o, d)


def object_texture_host(tri: np.ndarray, uv: np.ndarray, o: np.ndarray, d: np.ndarray, tex: PathObjectTex, texels: np.ndarray):
    """The kernel's texture lookups of a textured object on the CPU: triangle records tri [N,3,3] = (v0, e1, e2), corner coordinates
    uv [N,3,2], rays o, d [N,3], one record over texels [n,4] -> (u [N], v [N], st [N,2], base [N,3], orm [N,3]); (1, 1, 1) for an
    image the record does not have."""
    TX = _aligned_texels(texels)
    return _at_hits("matpbr_path_object_texture_host", tri, uv, "uv", 2, o, d, _ref(tex), TX, TX.shape[0], outs=(1, 1, 2, 3, 3))


def trans_edit(ior: float = 1.2, spec_trans: float = 0.4, refract_distance: float = 100.0) -> PathTransEdit:
    """The scalars of a transparency edit, checked as the library checks them; ValueError when bad."""
    ior, spec_trans, refract_distance = float(ior), float(spec_trans), float(refract_distance)
    if not (ior > 0 and np.isfinite(ior)):
        raise ValueError(f"ior must be positive and finite, got {ior}")
    if not 0.0 <= spec_trans <= 1.0:
        raise ValueError(f"spec_trans must lie in [0, 1], got {spec_trans}")
    if not (refract_distance >= 0 and np.isfinite(refract_distance)):
        raise ValueError(f"refract_distance must be non-negative and finite, got {refract_distance}")
    return PathTransEdit(ior, spec_trans, refract_distance, 0.0)


def trans_eval_host(n: np.ndarray, wo: np.ndarray, wi: np.ndarray, a: np.ndarray, r: np.ndarray, m: np.ndarray, bg: np.ndarray,
                    ior: float = 1.2, spec_trans: float = 0.4):
    """The kernel's masked-branch BSDF (TransBSDF.eval_brdf where the mask is set) on the CPU: n, wo, wi, a, bg [N,3], r, m [N] ->
    (f [N,3] with its cosine, pdf [N])."""
    ed = trans_edit(ior, spec_trans)
    nn, WO, WI, A, BG, R, M = _rows(n, 3), _rows(wo, 3), _rows(wi, 3), _rows(a, 3), _rows(bg, 3), _rows(r, 1), _rows(m, 1)
    N = _same_rows("n, wo, wi, a, r, m and bg must have the same rows", nn, WO, WI, A, BG, R, M)
    f, pdf = _out(N, 3, 1)
    _call("matpbr_path_trans_eval_host", _ref(ed), nn, WO, WI, A, R, M, BG, N, f, pdf)
    return f, pdf


def trans_lookup_host(p: np.ndarray, n: np.ndarray, wo: np.ndarray, H: int, W: int, ior: float = 1.2, refract_distance: float = 100.0,
                      fov_x_deg: float = 35.0):
    """The kernel's texel lookups of a transparency edit on the CPU: hit points p, face normals n, wo [N,3] -> (texel [N] of the
    point itself, texel [N] the background is read at; row * W + col)."""
    ed = trans_edit(ior, 0.0, refract_distance)
    P, nn, WO = _rows(p, 3), _rows(n, 3), _rows(wo, 3)
    N = _same_rows("p, n and wo must have the same rows", P, nn, WO)
    tp, tq = np.empty(N, np.int32), np.empty(N, np.int32)
    _call("matpbr_path_trans_lookup_host", _ref(ed), P, nn, WO, N, int(H), int(W), float(fov_x_deg), tp, tq)
    return tp, tq


def eval_normal_grad_host(n: np.ndarray, wo: np.ndarray, wi: np.ndarray, a: np.ndarray, r: np.ndarray, m: np.ndarray, g: np.ndarray):
    """d (g . f) / d n of the BSDF value on the CPU, composed and gated by the routine the backward kernel runs: n, wo, wi, a, g [N,3],
    r, m [N] -> d_n [N,3] = gl wi + gv wo + gh h, with respect to n's components as free variables."""
    nn, WO, WI, A, G, R, M = _rows(n, 3), _rows(wo, 3), _rows(wi, 3), _rows(a, 3), _rows(g, 3), _rows(r, 1), _rows(m, 1)
    N = _same_rows("n, wo, wi, a, r, m and g must have the same rows", nn, WO, WI, A, G, R, M)
    d_n, = _out(N, 3)
    _call("matpbr_path_eval_normal_grad_host", nn, WO, WI, A, R, M, G, N, d_n)
    return d_n


def _host_image(x, shape, what: str) -> np.ndarray:
    """A fresh (so aligned) contiguous float32 copy of `x`, which must have `shape`."""
    a = np.asarray(x)
    if tuple(a.shape) != tuple(shape):
        raise ValueError(f"{what} must be {list(shape)}, got {list(a.shape)}")
    return np.array(a, dtype=np.float32, order="C", copy=True)


def _copy32(x) -> Optional[np.ndarray]:
    return None if x is None else np.array(x, dtype=np.float32, order="C", copy=True)


def _size(H: int, W: int) -> tuple:
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"H and W must be positive, got {H} x {W}")
    return H, W


def _first_hit_host(name: str, bvh: Dict[str, object], H: int, W: int, fov_x_deg: float, table, channels: int, *own) -> np.ndarray:
    """out [H,W,channels] of the first-hit entry `name` on the CPU: it takes the BVH, the camera, the table and its count, its `own`
    arguments, then out."""
    out = np.empty((H, W, channels), np.float32)
    _call(name, bvh["nodes"], bvh["tris"], H, W, float(fov_x_deg), _table_ptrs(table)[0], len(table) if table else 0, *own, out)
    return out


def features_host(bvh: Dict[str, object], H: int, W: int, fov_x_deg: float = 35.0, objects: Optional[Sequence[PathObject]] = None,
                  obj_nrm: Optional[np.ndarray] = None, n_scene_tri: int = 0, normal: Optional[np.ndarray] = None) -> np.ndarray:
    """`PathTracer.features` on the CPU with the routine the kernel runs -> geom [H,W,8].  `bvh`: what `build_bvh` returned;
    `objects`, `obj_nrm`, `n_scene_tri`: `merge_objects`' table, its corner normals and the depth mesh's triangle count; `normal`
    [H,W,3]: the shading-normal map."""
    H, W = _size(H, W)
    nm = None if normal is None else _host_image(normal, (H, W, 3), "normal")
    return _first_hit_host("matpbr_path_features_host", bvh, H, W, fov_x_deg, _uncolored(objects), 8, _copy32(obj_nrm), int(n_scene_tri), nm)


def feature_colors_host(bvh: Dict[str, object], H: int, W: int, fov_x_deg: float = 35.0, objects: Optional[Sequence[PathObject]] = None,
                        obj_col: Optional[np.ndarray] = None, n_scene_tri: int = 0) -> np.ndarray:
    """`PathTracer.feature_colors` on the CPU with the routine the kernel runs -> [H,W,3]: the interpolated colour where the camera
    ray through the pixel centre first hits a vertex-coloured object, (1, 1, 1) elsewhere.  `objects`, `obj_col`, `n_scene_tri`:
    `merge_objects`' table, its corner colours and the depth mesh's triangle count."""
    H, W = _size(H, W)
    return _first_hit_host("matpbr_path_feature_colors_host", bvh, H, W, fov_x_deg, objects, 3, int(n_scene_tri), _copy32(obj_col))


def feature_tints_host(bvh: Dict[str, object], H: int, W: int, fov_x_deg: float = 35.0, objects: Optional[Sequence[PathObject]] = None,
                       obj_col: Optional[np.ndarray] = None, textures=None, n_scene_tri: int = 0) -> np.ndarray:
    """`PathTracer.feature_tints` on the CPU with the routine the kernel runs -> [H,W,3]: the interpolated colour times the base-colour
    fetch where the camera ray through the pixel centre first hits a coloured or textured object, (1, 1, 1) elsewhere.  `objects`,
    `obj_col`, `textures`, `n_scene_tri`: `merge_objects`' table, its corner colours, its (obj_uv, records, texels) and the depth
    mesh's triangle count."""
    H, W = _size(H, W)
    uv, records, texels = (None, None, None) if textures is None else (_copy32(textures[0]), textures[1], _aligned_texels(textures[2]))
    return _first_hit_host("matpbr_path_feature_tints_host", bvh, H, W, fov_x_deg, objects, 3, int(n_scene_tri), _copy32(obj_col), uv,
                           *_tex_ptrs(objects, records, texels))
