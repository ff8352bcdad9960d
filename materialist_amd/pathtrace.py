"""Path-traced re-render of the depth mesh: the ctypes binding of libmatpbr_path.so (include/matpbr_path.h) and `PathTracer`.

The deterministic render is direct light, unshadowed, under SH25.  The reference's *final* images come from
Mitsuba's `path` integrator, `max_depth` 4, on the `.ply` mesh under the texel envmap (render_final.py:35-96, inverse_img_w_mi.py:
49-52).  `PathTracer` is that render on the GPU: shadows, inter-reflection, the envmap's texels as the light.
`PathTracer.render_bwd` is its backward pass (the fixed-seed estimator's derivative with the sampling detached) and `PathRenderFn`
puts both behind autograd.  `PathTracer.features` and `PathTracer.denoise` are the opt-in denoiser (DESIGN.md section 1.4,
"Denoiser"): first-hit features and a variance-guided a-trous filter over two half renders, forward only.  `PathTracer.render_diff`
and `composite` are the differential render ("Differential render"): what inserted objects add to and take
from a photograph of the scene, forward only; `PathTracer.denoise_diff` is its own a-trous filter over two halves of it ("Denoiser
for the differential render"); `PathTracer.render_diff_through` is the differential render with the photograph shown, refracted,
behind inserted clear glass ("Seen through glass").  There is no fallback: a missing or failing library raises.
"""
from __future__ import annotations

import ctypes
import threading
import time
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import build as _build

_P = ctypes.c_void_p
_lib = None
_lock = threading.Lock()

NODE_BYTES = 64
TRI_BYTES = 48
MAX_BVH_DEPTH = 40
MAX_OBJECTS = 8
BSDF_DIELECTRIC, BSDF_DIFFUSE = 1, 2
BSDF_PBR = 3                   # MATPBR_PATH_BSDF_PBR: MatDiffBSDF on the constants of a PathObjectPbr record
PBR_MIN_ROUGHNESS = 0.07       # the floor the project's roughness maps are clamped to (matpbr_shade.hpp, armhead.py)
PBR_DEFAULTS = {"albedo": 0.8, "roughness": 0.5, "metallic": 0.0}
BSDF_AREA = 4                  # MATPBR_PATH_BSDF_AREA: an area light, p = radiance ("Emissive inserted objects")
BSDF_ROUGH_DIELECTRIC = 5      # MATPBR_PATH_BSDF_ROUGH_DIELECTRIC: rough glass, p = (int_ior, ext_ior, alpha) ("Rough dielectric objects")
ROUGH_MIN_ALPHA = 0.02         # the GGX width's floor: the peak of D is 1 / (pi alpha^2)
ROUGH_MIN_CONTRAST = 0.01      # |int_ior / ext_ior - 1| at least this: at a ratio of 1 the refraction Jacobian has no finite value
OBJECT_SMOOTH = 0x100          # MATPBR_PATH_OBJECT_SMOOTH, OR-ed into PathObject.kind
OBJECT_COLORED = 0x200         # MATPBR_PATH_OBJECT_COLORED, OR-ed into the kind of a diffuse or pbr object ("Vertex-coloured inserted objects")
OBJECT_TEXTURED = 0x400        # MATPBR_PATH_OBJECT_TEXTURED, OR-ed into the kind of a diffuse or pbr object ("Textured inserted objects")
OBJECT_FLAGS = OBJECT_SMOOTH | OBJECT_COLORED | OBJECT_TEXTURED
TEXTURE_MAX_SIDE = 8192        # w, h of an image
TEXTURE_MAX_UV = 64.0          # |s|, |t| of a corner: a coordinate's fractional part keeps 17 bits or more


class PathObject(ctypes.Structure):
    """MatpbrPathObject (include/matpbr_path.h): the BSDF of one range of triangle ids."""
    _fields_ = [("kind", ctypes.c_int32), ("first_tri", ctypes.c_int32), ("n_tri", ctypes.c_int32), ("p", ctypes.c_float * 3)]


class PathObjectPbr(ctypes.Structure):
    """MatpbrPathObjectPbr (include/matpbr_path.h): albedo, roughness and metallic of one object of kind BSDF_PBR."""
    _fields_ = [("a", ctypes.c_float * 3), ("r", ctypes.c_float), ("m", ctypes.c_float), ("reserved", ctypes.c_float * 3)]


class PathObjectTex(ctypes.Structure):
    """MatpbrPathObjectTex (include/matpbr_path.h): where the base-colour and the orm image of one textured object lie among the texels
    (w = 0: no such image)."""
    _fields_ = [("base_first", ctypes.c_int32), ("base_w", ctypes.c_int32), ("base_h", ctypes.c_int32), ("orm_first", ctypes.c_int32),
                ("orm_w", ctypes.c_int32), ("orm_h", ctypes.c_int32), ("reserved", ctypes.c_int32 * 2)]


class PathLights(ctypes.Structure):
    """MatpbrPathLights (include/matpbr_path.h): the per-light header of a table with objects of kind BSDF_AREA."""
    _fields_ = [("n_lights", ctypes.c_int32), ("object", ctypes.c_int32 * MAX_OBJECTS), ("first", ctypes.c_int32 * MAX_OBJECTS),
                ("n_tri", ctypes.c_int32 * MAX_OBJECTS), ("area", ctypes.c_float * MAX_OBJECTS)]


class PathTransEdit(ctypes.Structure):
    """MatpbrPathTransEdit (include/matpbr_path.h): the scalars of a transparency edit."""
    _fields_ = [("ior", ctypes.c_float), ("spec_trans", ctypes.c_float), ("refract_distance", ctypes.c_float), ("reserved", ctypes.c_float)]


class PathDenoise(ctypes.Structure):
    """MatpbrPathDenoise (include/matpbr_path.h): the levels and the four sigmas of the a-trous filter."""
    _fields_ = [("levels", ctypes.c_int32), ("sigma_n", ctypes.c_float), ("sigma_x", ctypes.c_float), ("sigma_a", ctypes.c_float),
                ("sigma_c", ctypes.c_float)]


# the 18 common arguments of a render or a backward pass (`PathTracer._frame`); a render then takes out, rays, stream, a backward pass
# d_out, d_a, d_r, d_m, d_env, workspace, workspace_bytes, rays, stream; an entry point's own arguments follow
_FRAME = [_P] * 5 + [ctypes.c_int, ctypes.c_int, ctypes.c_float] + [_P] * 4 + [ctypes.c_int] * 4 + [ctypes.c_uint32, ctypes.c_int]
_RENDER = _FRAME + [_P] * 3
_RENDER_BWD = _FRAME + [_P] * 6 + [ctypes.c_size_t, _P, _P]
SIGNATURES = {
    "matpbr_path_version": (ctypes.c_int, []),
    "matpbr_path_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "matpbr_path_bvh_size": (ctypes.c_int, [ctypes.c_long, _P]),
    "matpbr_path_bvh_build": (ctypes.c_int, [_P, ctypes.c_long, _P, ctypes.c_long, _P, ctypes.c_long, _P, _P, _P, _P]),
    "matpbr_path_bvh_build_objects": (ctypes.c_int, [_P, ctypes.c_long, _P, ctypes.c_long, ctypes.c_long, _P, ctypes.c_long, _P, _P, _P, _P]),
    "matpbr_path_trace_host": (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_long, ctypes.c_float, ctypes.c_float, _P, _P]),
    "matpbr_path_env_tables": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, _P, _P, _P, _P]),
    "matpbr_path_env_sample_host": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, ctypes.c_long, _P, _P, _P]),
    "matpbr_path_render": (ctypes.c_int, _RENDER),
    "matpbr_path_render_objects": (ctypes.c_int, _RENDER + [_P, ctypes.c_int]),
    "matpbr_path_object_sample_host": (ctypes.c_int, [_P] * 4 + [ctypes.c_long] + [_P] * 4),
    "matpbr_path_render_objects_normals": (ctypes.c_int, _RENDER + [_P, ctypes.c_int, _P, ctypes.c_long]),
    "matpbr_path_object_normal_host": (ctypes.c_int, [_P] * 4 + [ctypes.c_long] + [_P] * 3),
    "matpbr_path_render_objects_pbr": (ctypes.c_int, _RENDER + [_P, ctypes.c_int, _P, ctypes.c_long, _P]),
    "matpbr_path_object_lookup_host": (ctypes.c_int, [_P, ctypes.c_int, _P, _P, ctypes.c_long, _P, _P, _P, _P]),
    "matpbr_path_light_tables": (ctypes.c_int, [_P, ctypes.c_long, _P, ctypes.c_long, _P, ctypes.c_int, _P, _P, _P, _P, ctypes.c_long, _P]),
    "matpbr_path_render_objects_lights": (ctypes.c_int, _RENDER + [_P, ctypes.c_int, _P, ctypes.c_long, _P, _P, _P, _P]),
    "matpbr_path_light_sample_host": (ctypes.c_int, [_P, _P, _P, ctypes.c_long, ctypes.c_int, _P, _P, ctypes.c_long] + [_P] * 7),
    "matpbr_path_light_pdf_host": (ctypes.c_int, [_P, _P, ctypes.c_long, ctypes.c_int, _P, _P, _P, _P, ctypes.c_long, _P, _P]),
    "matpbr_path_render_objects_rough": (ctypes.c_int, _RENDER + [_P, ctypes.c_int, _P, ctypes.c_long, _P, _P, _P, _P]),
    "matpbr_path_rough_sample_host": (ctypes.c_int, [_P] * 5 + [ctypes.c_long] + [_P] * 4),
    "matpbr_path_rough_eval_host": (ctypes.c_int, [_P] * 5 + [ctypes.c_long] + [_P] * 2),
    "matpbr_path_object_sample_shading_host": (ctypes.c_int, [_P] * 5 + [ctypes.c_long] + [_P] * 4),
    "matpbr_path_render_objects_colors": (ctypes.c_int, _RENDER + [_P, ctypes.c_int, _P, ctypes.c_long, _P, _P, _P, _P, _P]),
    "matpbr_path_object_color_host": (ctypes.c_int, [_P] * 4 + [ctypes.c_long] + [_P] * 3),
    "matpbr_path_feature_colors": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_float, _P, ctypes.c_int, ctypes.c_long, _P, _P, _P]),
    "matpbr_path_feature_colors_host": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_float, _P, ctypes.c_int, ctypes.c_long, _P, _P]),
    "matpbr_path_render_objects_textures": (ctypes.c_int, _RENDER + [_P, ctypes.c_int, _P, ctypes.c_long, _P, _P, _P, _P, _P, _P, _P, _P, ctypes.c_long]),
    "matpbr_path_object_texture_host": (ctypes.c_int, [_P] * 4 + [ctypes.c_long, _P, _P, ctypes.c_long] + [_P] * 5),
    "matpbr_path_feature_tints": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_float, _P, ctypes.c_int, ctypes.c_long, _P, _P, _P, _P,
                                                 ctypes.c_long, _P, _P]),
    "matpbr_path_feature_tints_host": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_float, _P, ctypes.c_int, ctypes.c_long, _P, _P, _P, _P,
                                                      ctypes.c_long, _P]),
    "matpbr_path_render_objects_diff": (ctypes.c_int, _FRAME + [_P, _P] + [_P, ctypes.c_int, _P, ctypes.c_long, _P, _P, _P, _P, _P, _P, _P, _P, ctypes.c_long] + [_P] * 4),
    "matpbr_path_render_objects_through": (ctypes.c_int, _FRAME + [_P, _P] + [_P, ctypes.c_int, _P, ctypes.c_long, _P, _P, _P, _P, _P, _P, _P, _P, ctypes.c_long] + [_P] * 6),
    "matpbr_path_through_chain_host": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_long, _P, _P, _P,
                                                      ctypes.c_long] + [_P] * 5),
    "matpbr_path_composite": (ctypes.c_int, [_P] * 4 + [ctypes.c_int, ctypes.c_int, ctypes.c_float, _P, _P]),
    "matpbr_path_composite_host": (ctypes.c_int, [_P] * 4 + [ctypes.c_int, ctypes.c_int, ctypes.c_float, _P]),
    "matpbr_path_trace_scene_host": (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_long, ctypes.c_float, ctypes.c_float, _P, _P, ctypes.c_long, ctypes.c_int]),
    "matpbr_path_render_trans": (ctypes.c_int, _RENDER + [_P, _P, _P]),
    "matpbr_path_trans_eval_host": (ctypes.c_int, [_P] * 8 + [ctypes.c_long, _P, _P]),
    "matpbr_path_trans_lookup_host": (ctypes.c_int, [_P] * 4 + [ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_float, _P, _P]),
    "matpbr_path_render_bwd_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 4),
    "matpbr_path_render_bwd": (ctypes.c_int, _RENDER_BWD),
    "matpbr_path_render_normals": (ctypes.c_int, _RENDER + [_P]),
    "matpbr_path_eval_normal_grad_host": (ctypes.c_int, [_P] * 7 + [ctypes.c_long, _P]),
    "matpbr_path_render_bwd_normals_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int] * 4),
    "matpbr_path_render_bwd_normals": (ctypes.c_int, _RENDER_BWD + [_P, _P]),
    "matpbr_path_features": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_float, _P, ctypes.c_int, _P, ctypes.c_long, _P, _P, _P]),
    "matpbr_path_features_host": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_float, _P, ctypes.c_int, _P, ctypes.c_long, _P, _P]),
    "matpbr_path_denoise_prepare": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, _P]),
    "matpbr_path_denoise_prepare_host": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P]),
    "matpbr_path_denoise_level": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, ctypes.c_int, _P, _P]),
    "matpbr_path_denoise_level_host": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, ctypes.c_int, _P]),
    "matpbr_path_denoise_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "matpbr_path_denoise": (ctypes.c_int, [_P] * 4 + [ctypes.c_int, ctypes.c_int, _P, _P, _P, ctypes.c_size_t, _P]),
    "matpbr_path_denoise_diff_prepare": (ctypes.c_int, [_P] * 7 + [ctypes.c_int, ctypes.c_int, ctypes.c_float, _P, _P, _P]),
    "matpbr_path_denoise_diff_prepare_host": (ctypes.c_int, [_P] * 7 + [ctypes.c_int, ctypes.c_int, ctypes.c_float, _P, _P]),
    "matpbr_path_denoise_diff_level": (ctypes.c_int, [_P] * 4 + [ctypes.c_int, ctypes.c_int, _P, ctypes.c_int, _P, _P]),
    "matpbr_path_denoise_diff_level_host": (ctypes.c_int, [_P] * 4 + [ctypes.c_int, ctypes.c_int, _P, ctypes.c_int, _P]),
    "matpbr_path_denoise_diff_finish": (ctypes.c_int, [_P] * 9 + [ctypes.c_int, ctypes.c_int, ctypes.c_float, _P, _P, _P, _P]),
    "matpbr_path_denoise_diff_finish_host": (ctypes.c_int, [_P] * 9 + [ctypes.c_int, ctypes.c_int, ctypes.c_float, _P, _P, _P]),
    "matpbr_path_denoise_diff_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "matpbr_path_denoise_diff": (ctypes.c_int, [_P] * 8 + [ctypes.c_int, ctypes.c_int, ctypes.c_float, _P, _P, _P, _P, _P, ctypes.c_size_t, _P]),
    "matpbr_path_denoise_diff_host": (ctypes.c_int, [_P] * 8 + [ctypes.c_int, ctypes.c_int, ctypes.c_float, _P, _P, _P, _P, _P, ctypes.c_size_t]),
}
VERSION = 3
MAX_BWD_ENV_TEXELS = 1024
# added at version 3 (smooth inserted objects): a version-3 library built before them loads, and `symbol` names what it lacks
SMOOTH_SYMBOLS = ("matpbr_path_render_objects_normals", "matpbr_path_object_normal_host", "matpbr_path_object_sample_shading_host")
# added at version 3 too (the denoiser)
DENOISE_SYMBOLS = ("matpbr_path_features", "matpbr_path_features_host", "matpbr_path_denoise_prepare", "matpbr_path_denoise_prepare_host",
                   "matpbr_path_denoise_level", "matpbr_path_denoise_level_host", "matpbr_path_denoise_workspace_bytes", "matpbr_path_denoise")
# added at version 3 as well (PBR inserted objects)
PBR_SYMBOLS = ("matpbr_path_render_objects_pbr", "matpbr_path_object_lookup_host")
# and (emissive inserted objects)
LIGHT_SYMBOLS = ("matpbr_path_light_tables", "matpbr_path_render_objects_lights", "matpbr_path_light_sample_host", "matpbr_path_light_pdf_host")
# and (rough dielectric inserted objects)
ROUGH_SYMBOLS = ("matpbr_path_render_objects_rough", "matpbr_path_rough_sample_host", "matpbr_path_rough_eval_host")
# and (vertex-coloured inserted objects)
COLOR_SYMBOLS = ("matpbr_path_render_objects_colors", "matpbr_path_object_color_host", "matpbr_path_feature_colors", "matpbr_path_feature_colors_host")
# and (textured inserted objects)
TEXTURE_SYMBOLS = ("matpbr_path_render_objects_textures", "matpbr_path_object_texture_host", "matpbr_path_feature_tints", "matpbr_path_feature_tints_host")
# and (the differential render)
DIFF_SYMBOLS = ("matpbr_path_render_objects_diff", "matpbr_path_composite", "matpbr_path_composite_host", "matpbr_path_trace_scene_host")
# and (the differential render's denoiser)
DIFF_DENOISE_SYMBOLS = ("matpbr_path_denoise_diff_prepare", "matpbr_path_denoise_diff_prepare_host", "matpbr_path_denoise_diff_level",
                        "matpbr_path_denoise_diff_level_host", "matpbr_path_denoise_diff_finish", "matpbr_path_denoise_diff_finish_host",
                        "matpbr_path_denoise_diff_workspace_bytes", "matpbr_path_denoise_diff", "matpbr_path_denoise_diff_host")
# and (the photograph seen through inserted glass)
THROUGH_SYMBOLS = ("matpbr_path_render_objects_through", "matpbr_path_through_chain_host")
LATE_SYMBOLS = (SMOOTH_SYMBOLS + DENOISE_SYMBOLS + PBR_SYMBOLS + LIGHT_SYMBOLS + ROUGH_SYMBOLS + COLOR_SYMBOLS + TEXTURE_SYMBOLS + DIFF_SYMBOLS +
                DIFF_DENOISE_SYMBOLS + THROUGH_SYMBOLS)
# the feature each of them came with, as `symbol` names it
_FEATURE = {name: what for names, what in ((SMOOTH_SYMBOLS, "smooth inserted objects"), (DENOISE_SYMBOLS, "the denoiser"),
                                           (PBR_SYMBOLS, "PBR inserted objects"), (LIGHT_SYMBOLS, "emissive inserted objects"),
                                           (ROUGH_SYMBOLS, "rough dielectric inserted objects"),
                                           (COLOR_SYMBOLS, "vertex-coloured inserted objects"),
                                           (TEXTURE_SYMBOLS, "textured inserted objects"),
                                           (DIFF_SYMBOLS, "the differential render"),
                                           (DIFF_DENOISE_SYMBOLS, "the differential render's denoiser"),
                                           (THROUGH_SYMBOLS, "the photograph seen through inserted glass")) for name in names}
# the object entry points, one per level of DESIGN.md section 1.4, "The object entries" -> how many of `PathTracer.object_args()` each takes
OBJECT_ENTRIES = {"matpbr_path_render_objects": 2, "matpbr_path_render_objects_normals": 4, "matpbr_path_render_objects_pbr": 5,
                  "matpbr_path_render_objects_lights": 8, "matpbr_path_render_objects_rough": 8, "matpbr_path_render_objects_colors": 9,
                  "matpbr_path_render_objects_textures": 13, "matpbr_path_render_objects_through": 13}
DENOISE_DEFAULTS = {"levels": 5, "sigma_n": 32.0, "sigma_x": 1.0, "sigma_a": 0.1, "sigma_c": 4.0}


class PathError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Load libmatpbr_path.so (building it first when it is missing or older than its sources) and bind every symbol."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        _build.build_path_library()
        lib = ctypes.CDLL(_build.PATH_LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            if name in LATE_SYMBOLS and not hasattr(lib, name):
                continue
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        if lib.matpbr_path_version() != VERSION:
            raise PathError(f"libmatpbr_path.so is version {lib.matpbr_path_version()}, this binding needs {VERSION}")
        _lib = lib
        return lib


def symbol(name: str, lib: Optional[ctypes.CDLL] = None):
    """The library's function `name`; PathError naming it when the loaded library was built before it existed."""
    lib = load() if lib is None else lib
    if not hasattr(lib, name):
        what = _FEATURE.get(name, "smooth inserted objects")
        raise PathError(f"libmatpbr_path.so has no {name}: it was built before {what}; rebuild it (build.build_path_library)")
    return getattr(lib, name)


def check(code: int, what: str) -> None:
    if code != 0:
        msg = load().matpbr_path_strerror(code)
        raise PathError(f"{what} failed: {msg.decode() if msg else code} ({code})")


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def _rows(x, cols: int) -> np.ndarray:
    """`x` as contiguous float32 rows: [N, cols], or [N] for cols = 1."""
    a = np.ascontiguousarray(x, dtype=np.float32)
    return a.reshape(-1) if cols == 1 else a.reshape(-1, cols)


def _same_rows(refusal: str, first: np.ndarray, *rest: np.ndarray) -> int:
    """The row count the arrays share; ValueError(refusal) when they do not."""
    if any(x.shape[0] != first.shape[0] for x in rest):
        raise ValueError(refusal)
    return first.shape[0]


def _table_ptrs(table, records=None) -> tuple:
    """(the PathObject table, its PathObjectPbr records) as the C ABI takes them: a pointer, or None for a missing or empty one.
    ValueError unless there is one record per object."""
    def ptr(kind, xs):
        if xs is None or not len(xs):
            return None
        return ctypes.cast(xs if isinstance(xs, ctypes.Array) else (kind * len(xs))(*xs), _P)

    if records is not None and len(records) and len(records) != len(table):
        raise ValueError(f"one record per object: {len(table)} objects, {len(records)} records")
    return ptr(PathObject, table), ptr(PathObjectPbr, records)


def _uncolored(table, flags: int = OBJECT_COLORED | OBJECT_TEXTURED):
    """`table` as the entry points from before the colour flag take it (the features, the light tables: they need the kind and the smooth
    flag only): the same table where no object carries OBJECT_COLORED or OBJECT_TEXTURED, else copies without them.  `flags`: the
    flags to hide (the colour guide takes the colour flag and not the texture flag)."""
    if table is None or not any(t.kind & flags for t in table):
        return table
    return [PathObject(t.kind & ~flags, t.first_tri, t.n_tri, t.p) for t in table]


def _tex_ptrs(table, tex, texels):
    """(the PathObjectTex records, the texel buffer's address, its length) as the C ABI takes them; None, None, 0 without textures.
    `texels`: a float32 [n,4] numpy array or torch tensor.  ValueError unless there is one record per object."""
    if tex is None or not len(tex):
        return None, None, 0
    if len(tex) != len(table):
        raise ValueError(f"one record per object: {len(table)} objects, {len(tex)} texture records")
    rec = ctypes.cast(tex if isinstance(tex, ctypes.Array) else (PathObjectTex * len(tex))(*tex), _P)
    return rec, (texels.data_ptr() if hasattr(texels, "data_ptr") else _ptr(texels)), int(texels.shape[0])


def build_bvh(vertices: np.ndarray, triangles: np.ndarray, n_scene_tri: Optional[int] = None) -> Dict[str, object]:
    """Host BVH of a triangle mesh: {"nodes" uint8 [n_nodes*64], "tris" uint8 [T*48], "n_nodes", "depth", "n_leaves", "build_s"}.
    `n_scene_tri`: triangles from this index on belong to inserted meshes and keep their winding (`matpbr_path_bvh_build_objects`);
    None = every triangle is the depth mesh's (`matpbr_path_bvh_build`)."""
    lib = load()
    V = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    T = np.ascontiguousarray(triangles, dtype=np.int32).reshape(-1, 3)
    cap = ctypes.c_long(0)
    check(lib.matpbr_path_bvh_size(T.shape[0], ctypes.cast(ctypes.byref(cap), _P)), "matpbr_path_bvh_size")
    nodes = np.zeros(cap.value * NODE_BYTES, dtype=np.uint8)
    tris = np.zeros(max(T.shape[0], 1) * TRI_BYTES, dtype=np.uint8)
    n_nodes, depth, n_leaves = ctypes.c_long(0), ctypes.c_int(0), ctypes.c_long(0)
    t0 = time.perf_counter()
    outs = (ctypes.cast(ctypes.byref(n_nodes), _P), ctypes.cast(ctypes.byref(depth), _P), ctypes.cast(ctypes.byref(n_leaves), _P))
    if n_scene_tri is None:
        code = lib.matpbr_path_bvh_build(_ptr(V), V.shape[0], _ptr(T), T.shape[0], _ptr(nodes), cap.value, _ptr(tris), *outs)
    else:
        code = lib.matpbr_path_bvh_build_objects(_ptr(V), V.shape[0], _ptr(T), T.shape[0], int(n_scene_tri), _ptr(nodes), cap.value, _ptr(tris),
                                                 *outs)
    build_s = time.perf_counter() - t0
    check(code, "matpbr_path_bvh_build" if n_scene_tri is None else "matpbr_path_bvh_build_objects")
    return {"nodes": nodes[: n_nodes.value * NODE_BYTES].copy(), "tris": tris, "n_nodes": n_nodes.value, "depth": depth.value,
            "n_leaves": n_leaves.value, "build_s": build_s}


def trace_host(bvh: Dict[str, object], origins: np.ndarray, dirs: np.ndarray, tmin: float = 0.0, tmax: float = 3.0e38):
    """Closest hit on the CPU with the kernel's routine -> (t [N] float32, tmax where missed; triangle index [N] int32, -1 = miss)."""
    o, d = _rows(origins, 3), _rows(dirs, 3)
    t = np.empty(o.shape[0], np.float32)
    k = np.empty(o.shape[0], np.int32)
    check(load().matpbr_path_trace_host(_ptr(bvh["nodes"]), _ptr(bvh["tris"]), _ptr(o), _ptr(d), o.shape[0], tmin, tmax, _ptr(t), _ptr(k)),
          "matpbr_path_trace_host")
    return t, k


def trace_scene_host(bvh: Dict[str, object], origins: np.ndarray, dirs: np.ndarray, n_scene_tri: int, any: bool = False, tmin: float = 0.0,
                     tmax: float = 3.0e38):
    """`trace_host` over the triangles of id < `n_scene_tri` alone, the differential render's second walk: a triangle of a larger id is
    skipped before its test.  `any`: the shadow rays' traversal, which returns the first triangle it finds (t is then its distance,
    not the closest).  With `n_scene_tri` at the mesh's triangle count and `any` off it is `trace_host`, bit for bit."""
    o, d = _rows(origins, 3), _rows(dirs, 3)
    t = np.empty(o.shape[0], np.float32)
    k = np.empty(o.shape[0], np.int32)
    check(symbol("matpbr_path_trace_scene_host")(_ptr(bvh["nodes"]), _ptr(bvh["tris"]), _ptr(o), _ptr(d), o.shape[0], tmin, tmax, _ptr(t), _ptr(k),
                                                 int(n_scene_tri), int(bool(any))), "matpbr_path_trace_scene_host")
    return t, k


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
    thr, o, d = np.empty((N, 3), np.float32), np.empty((N, 3), np.float32), np.empty((N, 3), np.float32)
    check(symbol("matpbr_path_through_chain_host")(_ptr(bvh["nodes"]), _ptr(bvh["tris"]), int(H), int(W), float(fov_x_deg), int(max_depth), tab,
                                                   len(table), _ptr(nrm) if nrm is not None else None, int(n_scene_tri), _ptr(pix), _ptr(sd),
                                                   _ptr(smp), N, _ptr(depth), _ptr(texel), _ptr(thr), _ptr(o), _ptr(d)),
          "matpbr_path_through_chain_host")
    return {"depth": depth, "texel": texel, "thr": thr, "o": o, "d": d}


def env_tables(env: np.ndarray) -> Dict[str, object]:
    """Emitter-sampling tables of an envmap [He,We,3] (fp64 on the host, stored fp32): row_cdf [He+1], col_cdf [He,We+1], pdf [He,We]."""
    E = np.ascontiguousarray(env, dtype=np.float32)
    He, We = E.shape[:2]
    row = np.empty(He + 1, np.float32)
    col = np.empty((He, We + 1), np.float32)
    pdf = np.empty((He, We), np.float32)
    total = ctypes.c_double(0.0)
    check(load().matpbr_path_env_tables(_ptr(E), He, We, _ptr(row), _ptr(col), _ptr(pdf), ctypes.cast(ctypes.byref(total), _P)),
          "matpbr_path_env_tables")
    return {"row_cdf": row, "col_cdf": col, "pdf": pdf, "total": total.value}


def env_sample_host(tables: Dict[str, object], u: np.ndarray):
    """The render's emitter sampler on the CPU: u [N,4] -> (dir [N,3], pdf [N], texel [N] = row*We + col)."""
    U = _rows(u, 4)
    He, We = tables["pdf"].shape
    d = np.empty((U.shape[0], 3), np.float32)
    p = np.empty(U.shape[0], np.float32)
    k = np.empty(U.shape[0], np.int32)
    check(load().matpbr_path_env_sample_host(_ptr(tables["row_cdf"]), _ptr(tables["col_cdf"]), _ptr(tables["pdf"]), He, We, _ptr(U), U.shape[0],
                                             _ptr(d), _ptr(p), _ptr(k)), "matpbr_path_env_sample_host")
    return d, p, k


def object_bsdf(bsdf: dict) -> tuple:
    """{"type": "dielectric", "int_ior", "ext_ior"} | {"type": "diffuse", "reflectance"} -> (kind, (p0, p1, p2));
    {"type": "pbr", "albedo": scalar or 3 values (0.8), "roughness" (0.5), "metallic" (0)} -> (BSDF_PBR, (a0, a1, a2, r, m));
    {"type": "area", "radiance": scalar or 3 values, finite and >= 0 (1)} -> (BSDF_AREA, (r, g, b)): an area light.
    {"type": "roughdielectric", "int_ior" (1.49), "ext_ior" (1.000277), "alpha" (0.1): the GGX width in [0.02, 1]} ->
    (BSDF_ROUGH_DIELECTRIC, (int_ior, ext_ior, alpha)): rough glass; the indices' ratio stays at least 0.01 away from 1.
    ValueError when bad."""
    kind = bsdf.get("type") if isinstance(bsdf, dict) else None
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


def light_tables(V: np.ndarray, T: np.ndarray, table: Sequence[PathObject], records: Optional[Sequence[PathObjectPbr]] = None) -> Optional[dict]:
    """The light tables of a merged mesh (`merge_objects`' V, T, table and PBR records), built by the library on the host ->
    {"header": PathLights, "tris" float32 [n_light_tri, 3, 4] = (v0, 0) (e1, 0) (e2, 0) of every light triangle in input order,
    "cdf" float32 [n_light_tri]: per light the cumulative area / its area, the last entry exactly 1}; None when no object is of kind
    BSDF_AREA.  PathError where the library refuses the table (a light of total area 0 among the reasons)."""
    if not any(t.kind & ~OBJECT_SMOOTH == BSDF_AREA for t in table):
        return None
    table = _uncolored(table)
    Vv = np.ascontiguousarray(V, dtype=np.float64).reshape(-1, 3)
    Tt = np.ascontiguousarray(T, dtype=np.int32).reshape(-1, 3)
    tab, rec = _table_ptrs(table, records)
    fn = symbol("matpbr_path_light_tables")
    head, n = PathLights(), ctypes.c_long(0)
    hp, np_ = ctypes.cast(ctypes.byref(head), _P), ctypes.cast(ctypes.byref(n), _P)
    check(fn(_ptr(Vv), Vv.shape[0], _ptr(Tt), Tt.shape[0], tab, len(table), rec, hp, None, None, 0, np_), "matpbr_path_light_tables")
    tris, cdf = np.zeros((n.value, 3, 4), np.float32), np.zeros(n.value, np.float32)
    check(fn(_ptr(Vv), Vv.shape[0], _ptr(Tt), Tt.shape[0], tab, len(table), rec, hp, _ptr(tris), _ptr(cdf), n.value, np_), "matpbr_path_light_tables")
    return {"header": head, "tris": tris, "cdf": cdf}


def _light_args(lights: dict) -> tuple:
    """A 16-byte aligned copy of the records and the pointers of the two CPU entry points' first arguments."""
    n = lights["cdf"].shape[0]
    raw = np.zeros(n * 12 + 4, np.float32)
    off = (-raw.ctypes.data % 16) // 4
    tris = raw[off:off + n * 12]
    tris[:] = np.asarray(lights["tris"], np.float32).reshape(-1)
    return tris, ctypes.cast(ctypes.byref(lights["header"]), _P), n


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
    check(symbol("matpbr_path_light_sample_host")(hp, _ptr(tris), _ptr(cdf), n, int(bool(have_env)), _ptr(P), _ptr(U), N,
                                                  *(_ptr(o[k]) for k in ("emitter", "u_re", "record", "y", "wl", "dist", "pdf"))),
          "matpbr_path_light_sample_host")
    return o


def light_pdf_host(lights: dict, have_env: bool, light: np.ndarray, record: np.ndarray, o: np.ndarray, d: np.ndarray):
    """The hit side's pdf on the CPU with the kernel's routine: rays o, d [N,3] (unit length) that land on light triangle record [N] of
    light [N] -> (t [N], pdf [N] = t^2 / (A (n_l . -d) n_e), 0 on the back)."""
    O, D = _rows(o, 3), _rows(d, 3)
    Lg, Rc = np.ascontiguousarray(light, dtype=np.int32).reshape(-1), np.ascontiguousarray(record, dtype=np.int32).reshape(-1)
    N = _same_rows("light, record, o and d must have the same rows", O, D, Lg, Rc)
    tris, hp, n = _light_args(lights)
    t, pdf = np.empty(N, np.float32), np.empty(N, np.float32)
    check(symbol("matpbr_path_light_pdf_host")(hp, _ptr(tris), n, int(bool(have_env)), _ptr(Lg), _ptr(Rc), _ptr(O), _ptr(D), N, _ptr(t), _ptr(pdf)),
          "matpbr_path_light_pdf_host")
    return t, pdf


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
    "uv" without an image, an image without "uv", an image on another kind and "orm_texture" on a diffuse object are refused."""
    V = [np.asarray(vertices, dtype=np.float64).reshape(-1, 3)]
    T = [np.asarray(triangles, dtype=np.int32).reshape(-1, 3)]
    if len(objects) > MAX_OBJECTS:
        raise ValueError(f"at most {MAX_OBJECTS} inserted objects, got {len(objects)}")
    table: List[PathObject] = []
    corner: List[np.ndarray] = []
    tint: List[np.ndarray] = []
    st: List[np.ndarray] = []
    tex: List[PathObjectTex] = []
    texels: List[np.ndarray] = []
    records: List[PathObjectPbr] = []
    nv, nt = V[0].shape[0], T[0].shape[0]
    for k, ob in enumerate(objects):
        kind, p = object_bsdf(ob.get("bsdf"))
        records.append(PathObjectPbr((ctypes.c_float * 3)(*p[:3]), p[3], p[4]) if kind == BSDF_PBR else PathObjectPbr())
        if kind == BSDF_PBR:
            p = (0.0, 0.0, 0.0)
        Vo = np.asarray(ob["vertices"], dtype=np.float64)
        To = np.asarray(ob["triangles"])
        if Vo.ndim != 2 or Vo.shape[1] != 3 or To.ndim != 2 or To.shape[1] != 3 or To.shape[0] == 0:
            raise ValueError(f"object {k}: vertices must be [Nv,3] and triangles [Nt,3] (Nt > 0), got {Vo.shape} and {To.shape}")
        if not np.isfinite(Vo).all():
            raise ValueError(f"object {k}: vertices must be finite")
        if not np.issubdtype(To.dtype, np.integer) or To.min() < 0 or To.max() >= Vo.shape[0]:
            raise ValueError(f"object {k}: triangle indices must be integers in [0, {Vo.shape[0]})")
        if ob.get("normals") is not None and kind == BSDF_AREA:
            raise ValueError(f"object {k}: an area light has no shading normals: it emits from its faces (drop 'normals')")
        if ob.get("normals") is not None:
            corner.append(_corner_normals(k, ob, Vo, To))
            kind |= OBJECT_SMOOTH
        else:
            corner.append(np.zeros((To.shape[0], 3, 3)))
        if ob.get("colors") is not None:
            tint.append(_corner_colors(k, ob, kind & ~OBJECT_SMOOTH, Vo, To))
            kind |= OBJECT_COLORED
        else:
            tint.append(np.zeros((To.shape[0], 3, 3)))
        rec, images = _object_textures(k, ob, kind & ~OBJECT_FLAGS, sum(x.shape[0] for x in texels))
        tex.append(rec)
        texels += images
        if images:
            st.append(_corner_uv(k, ob, Vo, To))
            kind |= OBJECT_TEXTURED
        else:
            st.append(np.zeros((To.shape[0], 3, 2)))
        V.append(Vo)
        T.append((To.astype(np.int64) + nv).astype(np.int32))
        table.append(PathObject(kind, nt, To.shape[0], (ctypes.c_float * 3)(*p)))
        nv, nt = nv + Vo.shape[0], nt + To.shape[0]
    out = (np.concatenate(V), np.concatenate(T), table)
    if normals:
        smooth = any(t.kind & OBJECT_SMOOTH for t in table)
        out += (np.ascontiguousarray(np.concatenate(corner), dtype=np.float32) if smooth else None,)
    out += (records,) if pbr else ()
    out += (light_tables(out[0], out[1], table, records),) if lights else ()
    if colors:
        out += (np.ascontiguousarray(np.concatenate(tint), dtype=np.float32) if any(t.kind & OBJECT_COLORED for t in table) else None,)
    if textures:
        out += ((np.ascontiguousarray(np.concatenate(st), dtype=np.float32), tex, np.ascontiguousarray(np.concatenate(texels))) if texels else None,)
    return out


def object_lookup_host(table: Sequence[PathObject], records: Optional[Sequence[PathObjectPbr]], ids: np.ndarray):
    """The kernel's table lookup on the CPU: `merge_objects`' table and PBR records, triangle ids [N] -> (kind [N] int32, 0 where the
    id lies in no range, the smooth flag kept; a [N,3], r [N], m [N]: a PBR object's record, 0 for every other id)."""
    I = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
    tab, rec = _table_ptrs(table, records)
    kind = np.empty(I.size, np.int32)
    a, r, m = np.empty((I.size, 3), np.float32), np.empty(I.size, np.float32), np.empty(I.size, np.float32)
    check(symbol("matpbr_path_object_lookup_host")(tab, len(table), rec, _ptr(I), I.size, _ptr(kind), _ptr(a), _ptr(r), _ptr(m)),
          "matpbr_path_object_lookup_host")
    return kind, a, r, m


def _sampled_bsdf(bsdf: dict) -> tuple:
    """`object_bsdf` for the object samplers' host twins, which know the dielectric and the diffuse BSDF (a PBR object is sampled by the
    depth mesh's device routines, which have no host twin)."""
    kind, p = object_bsdf(bsdf)
    if kind == BSDF_PBR:
        raise ValueError("the object samplers on the CPU know 'dielectric' and 'diffuse'; a 'pbr' object samples with MatDiffBSDF's device code")
    if kind == BSDF_ROUGH_DIELECTRIC:
        raise ValueError("the object samplers on the CPU know 'dielectric' and 'diffuse'; a 'roughdielectric' object samples with rough_sample_host")
    return kind, p


def object_sample_host(bsdf: dict, n: np.ndarray, wo: np.ndarray, u: np.ndarray):
    """The kernel's BSDF sampler of an inserted object on the CPU: outward face normal n [3], wo [N,3], u [N,3] (dims 6, 7, 8) ->
    (wi [N,3], weight [N,3], pdf [N], flags [N]: bit 0 delta, bit 1 transmitted)."""
    kind, p = _sampled_bsdf(bsdf)
    ob = PathObject(kind, 0, 0, (ctypes.c_float * 3)(*p))
    nn = np.ascontiguousarray(n, dtype=np.float32).reshape(3)
    WO, U = _rows(wo, 3), _rows(u, 3)
    N = _same_rows(f"wo and u must have the same rows, got {WO.shape[0]} and {U.shape[0]}", WO, U)
    wi, w = np.empty((N, 3), np.float32), np.empty((N, 3), np.float32)
    pdf, flags = np.empty(N, np.float32), np.empty(N, np.int32)
    check(load().matpbr_path_object_sample_host(ctypes.cast(ctypes.byref(ob), _P), _ptr(nn), _ptr(WO), _ptr(U), N, _ptr(wi), _ptr(w), _ptr(pdf),
                                                _ptr(flags)), "matpbr_path_object_sample_host")
    return wi, w, pdf, flags


def object_normal_host(tri: np.ndarray, nrm: np.ndarray, o: np.ndarray, d: np.ndarray):
    """The kernel's shading normal of a smooth object on the CPU: triangle records tri [N,3,3] = (v0, e1, e2), corner normals nrm
    [N,3,3], rays o, d [N,3] -> (u [N], v [N], ns [N,3]); ns after the first two fallbacks (not finite or zero, ns . ng <= 0)."""
    TR = np.ascontiguousarray(tri, dtype=np.float32).reshape(-1, 3, 3)
    NR = np.ascontiguousarray(nrm, dtype=np.float32).reshape(-1, 3, 3)
    O, D = _rows(o, 3), _rows(d, 3)
    N = _same_rows("tri, nrm, o and d must have the same rows", TR, NR, O, D)
    u, v, ns = np.empty(N, np.float32), np.empty(N, np.float32), np.empty((N, 3), np.float32)
    check(symbol("matpbr_path_object_normal_host")(_ptr(TR), _ptr(NR), _ptr(O), _ptr(D), N, _ptr(u), _ptr(v), _ptr(ns)),
          "matpbr_path_object_normal_host")
    return u, v, ns


def object_color_host(tri: np.ndarray, col: np.ndarray, o: np.ndarray, d: np.ndarray):
    """The kernel's colour of a vertex-coloured object on the CPU: triangle records tri [N,3,3] = (v0, e1, e2), corner colours col
    [N,3,3], rays o, d [N,3] -> (u [N], v [N], c [N,3] = clamp(c0 + u (c1 - c0) + v (c2 - c0), 0, 1))."""
    TR = np.ascontiguousarray(tri, dtype=np.float32).reshape(-1, 3, 3)
    CL = np.ascontiguousarray(col, dtype=np.float32).reshape(-1, 3, 3)
    O, D = _rows(o, 3), _rows(d, 3)
    N = _same_rows("tri, col, o and d must have the same rows", TR, CL, O, D)
    u, v, c = np.empty(N, np.float32), np.empty(N, np.float32), np.empty((N, 3), np.float32)
    check(symbol("matpbr_path_object_color_host")(_ptr(TR), _ptr(CL), _ptr(O), _ptr(D), N, _ptr(u), _ptr(v), _ptr(c)),
          "matpbr_path_object_color_host")
    return u, v, c


def object_texture_host(tri: np.ndarray, uv: np.ndarray, o: np.ndarray, d: np.ndarray, tex: PathObjectTex, texels: np.ndarray):
    """The kernel's texture lookups of a textured object on the CPU: triangle records tri [N,3,3] = (v0, e1, e2), corner coordinates
    uv [N,3,2], rays o, d [N,3], one record over texels [n,4] -> (u [N], v [N], st [N,2], base [N,3], orm [N,3]); (1, 1, 1) for an
    image the record does not have."""
    TR = np.ascontiguousarray(tri, dtype=np.float32).reshape(-1, 3, 3)
    UV = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 3, 2)
    O, D = _rows(o, 3), _rows(d, 3)
    N = _same_rows("tri, uv, o and d must have the same rows", TR, UV, O, D)
    TX = _aligned_texels(texels)
    u, v, st = np.empty(N, np.float32), np.empty(N, np.float32), np.empty((N, 2), np.float32)
    base, orm = np.empty((N, 3), np.float32), np.empty((N, 3), np.float32)
    check(symbol("matpbr_path_object_texture_host")(_ptr(TR), _ptr(UV), _ptr(O), _ptr(D), N, ctypes.cast(ctypes.byref(tex), _P), _ptr(TX),
                                                    TX.shape[0], _ptr(u), _ptr(v), _ptr(st), _ptr(base), _ptr(orm)),
          "matpbr_path_object_texture_host")
    return u, v, st, base, orm


def _aligned_texels(texels) -> np.ndarray:
    """`texels` as float32 [n,4] in memory whose address is a multiple of 16, as the library's float4 loads need it."""
    a = np.asarray(texels, dtype=np.float32).reshape(-1, 4)
    buf = np.empty(a.size + 4, np.float32)
    off = (-buf.ctypes.data % 16) // 4
    out = buf[off:off + a.size].reshape(-1, 4)
    out[...] = a
    return out


def object_sample_shading_host(bsdf: dict, ng: np.ndarray, ns: np.ndarray, wo: np.ndarray, u: np.ndarray):
    """`object_sample_host` at vertices with a face normal ng [N,3] (or [3]) and a shading normal ns [N,3] (or [3]), as the kernel
    samples a smooth object: the third fallback, the sample about ns, the dielectric's redo about ng, weight 0 below ng ->
    (wi [N,3], weight [N,3], pdf [N], flags [N])."""
    kind, p = _sampled_bsdf(bsdf)
    ob = PathObject(kind, 0, 0, (ctypes.c_float * 3)(*p))
    WO, U = _rows(wo, 3), _rows(u, 3)
    N = _same_rows(f"wo and u must have the same rows, got {WO.shape[0]} and {U.shape[0]}", WO, U)
    NG = np.ascontiguousarray(np.broadcast_to(np.asarray(ng, dtype=np.float32).reshape(-1, 3), (N, 3)))
    NS = np.ascontiguousarray(np.broadcast_to(np.asarray(ns, dtype=np.float32).reshape(-1, 3), (N, 3)))
    wi, w = np.empty((N, 3), np.float32), np.empty((N, 3), np.float32)
    pdf, flags = np.empty(N, np.float32), np.empty(N, np.int32)
    check(symbol("matpbr_path_object_sample_shading_host")(ctypes.cast(ctypes.byref(ob), _P), _ptr(NG), _ptr(NS), _ptr(WO), _ptr(U), N, _ptr(wi),
                                                           _ptr(w), _ptr(pdf), _ptr(flags)), "matpbr_path_object_sample_shading_host")
    return wi, w, pdf, flags


def _rough_object(bsdf: dict) -> PathObject:
    kind, p = object_bsdf(bsdf)
    if kind != BSDF_ROUGH_DIELECTRIC:
        raise ValueError(f"rough_sample_host and rough_eval_host take a 'roughdielectric' bsdf, got {bsdf.get('type')!r}")
    return PathObject(kind, 0, 0, (ctypes.c_float * 3)(*p))


def _normal_rows(x, N: int) -> np.ndarray:
    return np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float32).reshape(-1, 3), (N, 3)))


def rough_sample_host(bsdf: dict, ng: np.ndarray, ns: np.ndarray, wo: np.ndarray, u: np.ndarray):
    """The kernel's sampler of a rough dielectric object on the CPU: face normal ng [N,3] (or [3]), shading normal ns [N,3] (or [3];
    ng on a flat object), wo [N,3], u [N,3] (dims 6, 7, 8) -> (wi [N,3], weight [N,3], pdf [N], flags [N]: bit 1 transmitted)."""
    ob = _rough_object(bsdf)
    WO, U = _rows(wo, 3), _rows(u, 3)
    N = _same_rows(f"wo and u must have the same rows, got {WO.shape[0]} and {U.shape[0]}", WO, U)
    NG, NS = _normal_rows(ng, N), _normal_rows(ns, N)
    wi, w = np.empty((N, 3), np.float32), np.empty((N, 3), np.float32)
    pdf, flags = np.empty(N, np.float32), np.empty(N, np.int32)
    check(symbol("matpbr_path_rough_sample_host")(ctypes.cast(ctypes.byref(ob), _P), _ptr(NG), _ptr(NS), _ptr(WO), _ptr(U), N, _ptr(wi), _ptr(w),
                                                  _ptr(pdf), _ptr(flags)), "matpbr_path_rough_sample_host")
    return wi, w, pdf, flags


def rough_eval_host(bsdf: dict, ng: np.ndarray, ns: np.ndarray, wo: np.ndarray, wl: np.ndarray):
    """The kernel's evaluation of a rough dielectric object on the CPU, as an emitter sample takes it: directions wl [N,3] ->
    (f [N,3], with its cosine; pdf [N], the density `rough_sample_host` gives wl)."""
    ob = _rough_object(bsdf)
    WO, WL = _rows(wo, 3), _rows(wl, 3)
    N = _same_rows(f"wo and wl must have the same rows, got {WO.shape[0]} and {WL.shape[0]}", WO, WL)
    NG, NS = _normal_rows(ng, N), _normal_rows(ns, N)
    f, pdf = np.empty((N, 3), np.float32), np.empty(N, np.float32)
    check(symbol("matpbr_path_rough_eval_host")(ctypes.cast(ctypes.byref(ob), _P), _ptr(NG), _ptr(NS), _ptr(WO), _ptr(WL), N, _ptr(f), _ptr(pdf)),
          "matpbr_path_rough_eval_host")
    return f, pdf


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
    f, pdf = np.empty((N, 3), np.float32), np.empty(N, np.float32)
    check(load().matpbr_path_trans_eval_host(ctypes.cast(ctypes.byref(ed), _P), _ptr(nn), _ptr(WO), _ptr(WI), _ptr(A), _ptr(R), _ptr(M), _ptr(BG),
                                             N, _ptr(f), _ptr(pdf)), "matpbr_path_trans_eval_host")
    return f, pdf


def trans_lookup_host(p: np.ndarray, n: np.ndarray, wo: np.ndarray, H: int, W: int, ior: float = 1.2, refract_distance: float = 100.0,
                      fov_x_deg: float = 35.0):
    """The kernel's texel lookups of a transparency edit on the CPU: hit points p, face normals n, wo [N,3] -> (texel [N] of the
    point itself, texel [N] the background is read at; row * W + col)."""
    ed = trans_edit(ior, 0.0, refract_distance)
    P, nn, WO = _rows(p, 3), _rows(n, 3), _rows(wo, 3)
    N = _same_rows("p, n and wo must have the same rows", P, nn, WO)
    tp, tq = np.empty(N, np.int32), np.empty(N, np.int32)
    check(load().matpbr_path_trans_lookup_host(ctypes.cast(ctypes.byref(ed), _P), _ptr(P), _ptr(nn), _ptr(WO), N, int(H), int(W), float(fov_x_deg),
                                               _ptr(tp), _ptr(tq)), "matpbr_path_trans_lookup_host")
    return tp, tq


def eval_normal_grad_host(n: np.ndarray, wo: np.ndarray, wi: np.ndarray, a: np.ndarray, r: np.ndarray, m: np.ndarray, g: np.ndarray):
    """d (g . f) / d n of the BSDF value on the CPU, composed and gated by the routine the backward kernel runs: n, wo, wi, a, g [N,3],
    r, m [N] -> d_n [N,3] = gl wi + gv wo + gh h, with respect to n's components as free variables."""
    nn, WO, WI, A, G, R, M = _rows(n, 3), _rows(wo, 3), _rows(wi, 3), _rows(a, 3), _rows(g, 3), _rows(r, 1), _rows(m, 1)
    N = _same_rows("n, wo, wi, a, r, m and g must have the same rows", nn, WO, WI, A, G, R, M)
    d_n = np.empty((N, 3), np.float32)
    check(load().matpbr_path_eval_normal_grad_host(_ptr(nn), _ptr(WO), _ptr(WI), _ptr(A), _ptr(R), _ptr(M), _ptr(G), N, _ptr(d_n)),
          "matpbr_path_eval_normal_grad_host")
    return d_n


# ---- the denoiser ("Denoiser") ----------------------------------------------------------------------------------
def denoise_params(levels: Optional[int] = None, sigma_n: Optional[float] = None, sigma_x: Optional[float] = None,
                   sigma_a: Optional[float] = None, sigma_c: Optional[float] = None) -> PathDenoise:
    """The filter's parameters (None: DENOISE_DEFAULTS), checked as the library checks them; ValueError when bad."""
    given = {"levels": levels, "sigma_n": sigma_n, "sigma_x": sigma_x, "sigma_a": sigma_a, "sigma_c": sigma_c}
    v = {k: DENOISE_DEFAULTS[k] if x is None else x for k, x in given.items()}
    if int(v["levels"]) != v["levels"] or not 1 <= int(v["levels"]) <= 8:
        raise ValueError(f"levels must be an integer in 1..8, got {v['levels']}")
    for k in ("sigma_n", "sigma_x", "sigma_a", "sigma_c"):
        if not (float(v[k]) > 0 and np.isfinite(float(v[k]))):
            raise ValueError(f"{k} must be positive and finite, got {v[k]}")
    return PathDenoise(int(v["levels"]), float(v["sigma_n"]), float(v["sigma_x"]), float(v["sigma_a"]), float(v["sigma_c"]))


def _host_image(x, shape, what: str) -> np.ndarray:
    """A fresh (so aligned) contiguous float32 copy of `x`, which must have `shape`."""
    a = np.asarray(x)
    if tuple(a.shape) != tuple(shape):
        raise ValueError(f"{what} must be {list(shape)}, got {list(a.shape)}")
    return np.array(a, dtype=np.float32, order="C", copy=True)


def _geom_shape(geom, what: str = "geom") -> tuple:
    shp = tuple(geom.shape)
    if len(shp) != 3 or shp[2] != 8 or shp[0] < 1 or shp[1] < 1:
        raise ValueError(f"{what} must be [H,W,8], got {list(shp)}")
    return shp[0], shp[1]


def features_host(bvh: Dict[str, object], H: int, W: int, fov_x_deg: float = 35.0, objects: Optional[Sequence[PathObject]] = None,
                  obj_nrm: Optional[np.ndarray] = None, n_scene_tri: int = 0, normal: Optional[np.ndarray] = None) -> np.ndarray:
    """`PathTracer.features` on the CPU with the routine the kernel runs -> geom [H,W,8].  `bvh`: what `build_bvh` returned;
    `objects`, `obj_nrm`, `n_scene_tri`: `merge_objects`' table, its corner normals and the depth mesh's triangle count; `normal`
    [H,W,3]: the shading-normal map."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"H and W must be positive, got {H} x {W}")
    table, _ = _table_ptrs(_uncolored(objects))
    cn = None if obj_nrm is None else np.array(obj_nrm, dtype=np.float32, order="C", copy=True)
    nm = None if normal is None else _host_image(normal, (H, W, 3), "normal")
    geom = np.empty((H, W, 8), np.float32)
    check(symbol("matpbr_path_features_host")(_ptr(bvh["nodes"]), _ptr(bvh["tris"]), H, W, float(fov_x_deg), table, len(objects) if objects else 0,
                                              _ptr(cn) if cn is not None else None, int(n_scene_tri), _ptr(nm) if nm is not None else None,
                                              _ptr(geom)), "matpbr_path_features_host")
    return geom


def feature_colors_host(bvh: Dict[str, object], H: int, W: int, fov_x_deg: float = 35.0, objects: Optional[Sequence[PathObject]] = None,
                        obj_col: Optional[np.ndarray] = None, n_scene_tri: int = 0) -> np.ndarray:
    """`PathTracer.feature_colors` on the CPU with the routine the kernel runs -> [H,W,3]: the interpolated colour where the camera
    ray through the pixel centre first hits a vertex-coloured object, (1, 1, 1) elsewhere.  `objects`, `obj_col`, `n_scene_tri`:
    `merge_objects`' table, its corner colours and the depth mesh's triangle count."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"H and W must be positive, got {H} x {W}")
    table, _ = _table_ptrs(objects)
    cc = None if obj_col is None else np.array(obj_col, dtype=np.float32, order="C", copy=True)
    out = np.empty((H, W, 3), np.float32)
    check(symbol("matpbr_path_feature_colors_host")(_ptr(bvh["nodes"]), _ptr(bvh["tris"]), H, W, float(fov_x_deg), table,
                                                    len(objects) if objects else 0, int(n_scene_tri), _ptr(cc) if cc is not None else None,
                                                    _ptr(out)), "matpbr_path_feature_colors_host")
    return out


def feature_tints_host(bvh: Dict[str, object], H: int, W: int, fov_x_deg: float = 35.0, objects: Optional[Sequence[PathObject]] = None,
                       obj_col: Optional[np.ndarray] = None, textures=None, n_scene_tri: int = 0) -> np.ndarray:
    """`PathTracer.feature_tints` on the CPU with the routine the kernel runs -> [H,W,3]: the interpolated colour times the base-colour
    fetch where the camera ray through the pixel centre first hits a coloured or textured object, (1, 1, 1) elsewhere.  `objects`,
    `obj_col`, `textures`, `n_scene_tri`: `merge_objects`' table, its corner colours, its (obj_uv, records, texels) and the depth
    mesh's triangle count."""
    H, W = int(H), int(W)
    if H < 1 or W < 1:
        raise ValueError(f"H and W must be positive, got {H} x {W}")
    table, _ = _table_ptrs(objects)
    cc = None if obj_col is None else np.array(obj_col, dtype=np.float32, order="C", copy=True)
    uv = rec = tx = None
    n_texels = 0
    if textures is not None:
        uv = np.array(textures[0], dtype=np.float32, order="C", copy=True)
        tx_arr = _aligned_texels(textures[2])
        rec, tx, n_texels = _tex_ptrs(objects, textures[1], tx_arr)
    out = np.empty((H, W, 3), np.float32)
    check(symbol("matpbr_path_feature_tints_host")(_ptr(bvh["nodes"]), _ptr(bvh["tris"]), H, W, float(fov_x_deg), table,
                                                   len(objects) if objects else 0, int(n_scene_tri), _ptr(cc) if cc is not None else None,
                                                   _ptr(uv) if uv is not None else None, rec, tx, n_texels, _ptr(out)),
          "matpbr_path_feature_tints_host")
    return out


def denoise_prepare_host(A: np.ndarray, B: np.ndarray, geom: np.ndarray) -> np.ndarray:
    """The filter's first step on the CPU with the routine the kernel runs: A, B [H,W,3], geom [H,W,8] -> cv0 [H,W,4] = ((A + B) / 2,
    the prefiltered variance of the mean's luminance)."""
    H, W = _geom_shape(np.asarray(geom))
    a, b, g = _host_image(A, (H, W, 3), "A"), _host_image(B, (H, W, 3), "B"), _host_image(geom, (H, W, 8), "geom")
    cv = np.empty((H, W, 4), np.float32)
    check(symbol("matpbr_path_denoise_prepare_host")(_ptr(a), _ptr(b), _ptr(g), H, W, _ptr(cv)), "matpbr_path_denoise_prepare_host")
    return cv


def denoise_level_host(cv: np.ndarray, geom: np.ndarray, alb: np.ndarray, level: int, **params) -> np.ndarray:
    """One a-trous level (stride 2^level) on the CPU with the routine the kernel runs: cv [H,W,4], geom [H,W,8], alb [H,W,3] ->
    cv [H,W,4].  `params`: levels, sigma_n, sigma_x, sigma_a, sigma_c (`denoise_params`)."""
    prm = denoise_params(**params)
    H, W = _geom_shape(np.asarray(geom))
    if not 0 <= int(level) <= 7:
        raise ValueError(f"level must lie in 0..7, got {level}")
    c, g, al = _host_image(cv, (H, W, 4), "cv"), _host_image(geom, (H, W, 8), "geom"), _host_image(alb, (H, W, 3), "alb")
    out = np.empty((H, W, 4), np.float32)
    check(symbol("matpbr_path_denoise_level_host")(_ptr(c), _ptr(g), _ptr(al), H, W, ctypes.cast(ctypes.byref(prm), _P), int(level), _ptr(out)),
          "matpbr_path_denoise_level_host")
    return out


def _device_image(x, shape, what: str, device=None) -> torch.Tensor:
    t = torch.as_tensor(x)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what} must be {list(shape)}, got {list(t.shape)}")
    return t.to(device if device is not None else t.device, torch.float32).contiguous()


def _device_of(*xs):
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    return torch.device("cuda")


@torch.no_grad()
def denoise_prepare(A, B, geom) -> torch.Tensor:
    """`denoise_prepare_host` on the device (the current torch stream) -> cv0 [H,W,4]."""
    H, W = _geom_shape(torch.as_tensor(geom))
    dev = _device_of(geom, A, B)
    a, b, g = _device_image(A, (H, W, 3), "A", dev), _device_image(B, (H, W, 3), "B", dev), _device_image(geom, (H, W, 8), "geom", dev)
    cv = torch.empty(H, W, 4, device=dev, dtype=torch.float32)
    check(symbol("matpbr_path_denoise_prepare")(a.data_ptr(), b.data_ptr(), g.data_ptr(), H, W, cv.data_ptr(),
                                                torch.cuda.current_stream(dev).cuda_stream), "matpbr_path_denoise_prepare")
    return cv


@torch.no_grad()
def denoise_level(cv, geom, alb, level: int, **params) -> torch.Tensor:
    """`denoise_level_host` on the device (the current torch stream) -> cv [H,W,4]."""
    prm = denoise_params(**params)
    H, W = _geom_shape(torch.as_tensor(geom))
    if not 0 <= int(level) <= 7:
        raise ValueError(f"level must lie in 0..7, got {level}")
    dev = _device_of(geom, cv, alb)
    c, g, al = _device_image(cv, (H, W, 4), "cv", dev), _device_image(geom, (H, W, 8), "geom", dev), _device_image(alb, (H, W, 3), "alb", dev)
    out = torch.empty(H, W, 4, device=dev, dtype=torch.float32)
    check(symbol("matpbr_path_denoise_level")(c.data_ptr(), g.data_ptr(), al.data_ptr(), H, W, ctypes.cast(ctypes.byref(prm), _P), int(level),
                                              out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "matpbr_path_denoise_level")
    return out


@torch.no_grad()
def denoise(A, B, alb, geom, workspace: Optional[torch.Tensor] = None, **params) -> torch.Tensor:
    """The whole filter on the device (the current torch stream): two half renders A, B [H,W,3], the albedo guide alb [H,W,3] and the
    features geom [H,W,8] -> the denoised mean [H,W,3].  Equal to `denoise_prepare` and `levels` calls of `denoise_level`, bit for
    bit.  `workspace`: a uint8 device tensor of at least matpbr_path_denoise_workspace_bytes (default: allocated here)."""
    prm = denoise_params(**params)
    H, W = _geom_shape(torch.as_tensor(geom))
    dev = _device_of(geom, A, B, alb)
    a, b = _device_image(A, (H, W, 3), "A", dev), _device_image(B, (H, W, 3), "B", dev)
    al, g = _device_image(alb, (H, W, 3), "alb", dev), _device_image(geom, (H, W, 8), "geom", dev)
    nbytes = int(symbol("matpbr_path_denoise_workspace_bytes")(H, W))
    if workspace is None or workspace.numel() * workspace.element_size() < nbytes:
        workspace = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    out = torch.empty(H, W, 3, device=dev, dtype=torch.float32)
    check(symbol("matpbr_path_denoise")(a.data_ptr(), b.data_ptr(), g.data_ptr(), al.data_ptr(), H, W, ctypes.cast(ctypes.byref(prm), _P),
                                        out.data_ptr(), workspace.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream),
          "matpbr_path_denoise")
    return out


# ---- the differential render's composite ("Differential render") -------------------------------------------------
def _composite_scale(scale: float) -> float:
    sc = float(scale)
    if not (np.isfinite(np.float32(sc)) and np.float32(sc) > 0):
        raise ValueError(f"scale must be finite and positive (1 / the number of frames summed), got {scale}")
    return sc


def composite_host(fg, delta, alpha, photo, scale: float = 1.0) -> np.ndarray:
    """`composite` on the CPU with the routine the kernel runs: fg, delta, photo [H,W,3], alpha [H,W] -> [H,W,3], the same bits."""
    ph = np.asarray(photo)
    if ph.ndim != 3 or ph.shape[2] != 3 or ph.shape[0] < 1 or ph.shape[1] < 1:
        raise ValueError(f"photo must be [H,W,3], got {list(ph.shape)}")
    H, W = ph.shape[:2]
    sc = _composite_scale(scale)
    f, d, al, p = _host_image(fg, (H, W, 3), "fg"), _host_image(delta, (H, W, 3), "delta"), _host_image(alpha, (H, W), "alpha"), _host_image(ph, (H, W, 3), "photo")
    out = np.empty((H, W, 3), np.float32)
    check(symbol("matpbr_path_composite_host")(_ptr(f), _ptr(d), _ptr(al), _ptr(p), H, W, sc, _ptr(out)), "matpbr_path_composite_host")
    return out


@torch.no_grad()
def composite(fg, delta, alpha, photo, scale: float = 1.0) -> torch.Tensor:
    """The differential render composited into the photograph, on the device (the current torch stream): max(0, (fg + delta) scale +
    (1 - alpha scale) photo) per channel, every operation rounded on its own.  fg, delta, alpha: `PathTracer.render_diff`'s outputs,
    or their sums over some frames with `scale` = 1 / (the number of frames); photo [H,W,3], linear.  Where fg, delta and alpha are 0
    the photograph (>= 0) comes through bit for bit."""
    shp = tuple(torch.as_tensor(photo).shape)
    if len(shp) != 3 or shp[2] != 3 or shp[0] < 1 or shp[1] < 1:
        raise ValueError(f"photo must be [H,W,3], got {list(shp)}")
    H, W = shp[:2]
    sc = _composite_scale(scale)
    dev = _device_of(fg, delta, alpha, photo)
    f, d, al, p = (_device_image(fg, (H, W, 3), "fg", dev), _device_image(delta, (H, W, 3), "delta", dev), _device_image(alpha, (H, W), "alpha", dev),
                   _device_image(photo, (H, W, 3), "photo", dev))
    out = torch.empty(H, W, 3, device=dev, dtype=torch.float32)
    check(symbol("matpbr_path_composite")(f.data_ptr(), d.data_ptr(), al.data_ptr(), p.data_ptr(), H, W, sc, out.data_ptr(),
                                          torch.cuda.current_stream(dev).cuda_stream), "matpbr_path_composite")
    return out


# ---- the differential render's denoiser ("Denoiser for the differential render") ----------------------------------
# A, B: the (fg [H,W,3], delta [H,W,3], alpha [H,W]) triples of two sums of `PathTracer.render_diff`'s outputs over the same number of
# frames, with independent seeds and equal spp; scale = 1 / (frames summed per half).
def _halves(A, B, H: int, W: int, image) -> list:
    """The six images of two triples, in the library's order, each checked and converted by `image(x, shape, what)`."""
    if len(A) != 3 or len(B) != 3:
        raise ValueError("A and B must be (fg, delta, alpha) triples")
    return [image(x, (H, W, 3) if k < 2 else (H, W), f"{name}[{k}] ({('fg', 'delta', 'alpha')[k]})") for name, t in (("A", A), ("B", B))
            for k, x in enumerate(t)]


def _prm_ptr(prm: PathDenoise):
    return ctypes.cast(ctypes.byref(prm), _P)


def denoise_diff_prepare_host(A, B, geom, scale: float = 1.0) -> tuple:
    """The filter's first step on the CPU with the routine the kernel runs -> (cv0 [H,W,4], cov [H,W]): the own layer's unpremultiplied
    mean with the prefiltered variance of its luminance, and the own layer's coverage."""
    H, W = _geom_shape(np.asarray(geom))
    sc = _composite_scale(scale)
    hs, g = _halves(A, B, H, W, _host_image), _host_image(geom, (H, W, 8), "geom")
    cv, cov = np.empty((H, W, 4), np.float32), np.empty((H, W), np.float32)
    check(symbol("matpbr_path_denoise_diff_prepare_host")(*map(_ptr, hs), _ptr(g), H, W, sc, _ptr(cv), _ptr(cov)), "matpbr_path_denoise_diff_prepare_host")
    return cv, cov


def denoise_diff_level_host(cv, cov, geom, alb, level: int, **params) -> np.ndarray:
    """One a-trous level of the differential render's filter on the CPU with the routine the kernel runs -> cv [H,W,4]."""
    prm = denoise_params(**params)
    H, W = _geom_shape(np.asarray(geom))
    if not 0 <= int(level) <= 7:
        raise ValueError(f"level must lie in 0..7, got {level}")
    c, k, g, al = (_host_image(cv, (H, W, 4), "cv"), _host_image(cov, (H, W), "cov"), _host_image(geom, (H, W, 8), "geom"),
                   _host_image(alb, (H, W, 3), "alb"))
    out = np.empty((H, W, 4), np.float32)
    check(symbol("matpbr_path_denoise_diff_level_host")(_ptr(c), _ptr(k), _ptr(g), _ptr(al), H, W, _prm_ptr(prm), int(level), _ptr(out)),
          "matpbr_path_denoise_diff_level_host")
    return out


def denoise_diff_finish_host(cv, cov, A, B, geom, scale: float = 1.0) -> tuple:
    """The filter's last step on the CPU with the routine the kernel runs -> (fg', delta', alpha'): the own layer's filtered colour times
    its coverage, the other layer's mean and the mean alpha as they are."""
    H, W = _geom_shape(np.asarray(geom))
    sc = _composite_scale(scale)
    c, k, g = _host_image(cv, (H, W, 4), "cv"), _host_image(cov, (H, W), "cov"), _host_image(geom, (H, W, 8), "geom")
    hs = _halves(A, B, H, W, _host_image)
    fg, delta, alpha = np.empty((H, W, 3), np.float32), np.empty((H, W, 3), np.float32), np.empty((H, W), np.float32)
    check(symbol("matpbr_path_denoise_diff_finish_host")(_ptr(c), _ptr(k), *map(_ptr, hs), _ptr(g), H, W, sc, _ptr(fg), _ptr(delta), _ptr(alpha)),
          "matpbr_path_denoise_diff_finish_host")
    return fg, delta, alpha


def denoise_diff_host(A, B, alb, geom, scale: float = 1.0, **params) -> tuple:
    """`denoise_diff` on the CPU with the routines the kernels run -> (fg', delta', alpha').  Equal to its separate steps bit for bit."""
    prm = denoise_params(**params)
    H, W = _geom_shape(np.asarray(geom))
    sc = _composite_scale(scale)
    hs, g, al = _halves(A, B, H, W, _host_image), _host_image(geom, (H, W, 8), "geom"), _host_image(alb, (H, W, 3), "alb")
    nbytes = int(symbol("matpbr_path_denoise_diff_workspace_bytes")(H, W))
    ws = np.empty(nbytes // 4, np.float32)
    fg, delta, alpha = np.empty((H, W, 3), np.float32), np.empty((H, W, 3), np.float32), np.empty((H, W), np.float32)
    check(symbol("matpbr_path_denoise_diff_host")(*map(_ptr, hs), _ptr(g), _ptr(al), H, W, sc, _prm_ptr(prm), _ptr(fg), _ptr(delta), _ptr(alpha),
                                                  _ptr(ws), nbytes), "matpbr_path_denoise_diff_host")
    return fg, delta, alpha


@torch.no_grad()
def denoise_diff_prepare(A, B, geom, scale: float = 1.0) -> tuple:
    """`denoise_diff_prepare_host` on the device (the current torch stream) -> (cv0 [H,W,4], cov [H,W])."""
    H, W = _geom_shape(torch.as_tensor(geom))
    sc = _composite_scale(scale)
    dev = _device_of(geom, *A, *B)
    hs = _halves(A, B, H, W, lambda x, shape, what: _device_image(x, shape, what, dev))
    g = _device_image(geom, (H, W, 8), "geom", dev)
    cv, cov = torch.empty(H, W, 4, device=dev, dtype=torch.float32), torch.empty(H, W, device=dev, dtype=torch.float32)
    check(symbol("matpbr_path_denoise_diff_prepare")(*(h.data_ptr() for h in hs), g.data_ptr(), H, W, sc, cv.data_ptr(), cov.data_ptr(),
                                                     torch.cuda.current_stream(dev).cuda_stream), "matpbr_path_denoise_diff_prepare")
    return cv, cov


@torch.no_grad()
def denoise_diff_level(cv, cov, geom, alb, level: int, **params) -> torch.Tensor:
    """`denoise_diff_level_host` on the device (the current torch stream) -> cv [H,W,4]."""
    prm = denoise_params(**params)
    H, W = _geom_shape(torch.as_tensor(geom))
    if not 0 <= int(level) <= 7:
        raise ValueError(f"level must lie in 0..7, got {level}")
    dev = _device_of(geom, cv, cov, alb)
    c, k = _device_image(cv, (H, W, 4), "cv", dev), _device_image(cov, (H, W), "cov", dev)
    g, al = _device_image(geom, (H, W, 8), "geom", dev), _device_image(alb, (H, W, 3), "alb", dev)
    out = torch.empty(H, W, 4, device=dev, dtype=torch.float32)
    check(symbol("matpbr_path_denoise_diff_level")(c.data_ptr(), k.data_ptr(), g.data_ptr(), al.data_ptr(), H, W, _prm_ptr(prm), int(level),
                                                   out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "matpbr_path_denoise_diff_level")
    return out


@torch.no_grad()
def denoise_diff_finish(cv, cov, A, B, geom, scale: float = 1.0) -> tuple:
    """`denoise_diff_finish_host` on the device (the current torch stream) -> (fg', delta', alpha')."""
    H, W = _geom_shape(torch.as_tensor(geom))
    sc = _composite_scale(scale)
    dev = _device_of(geom, cv, cov, *A, *B)
    c, k, g = _device_image(cv, (H, W, 4), "cv", dev), _device_image(cov, (H, W), "cov", dev), _device_image(geom, (H, W, 8), "geom", dev)
    hs = _halves(A, B, H, W, lambda x, shape, what: _device_image(x, shape, what, dev))
    fg, delta = torch.empty(H, W, 3, device=dev, dtype=torch.float32), torch.empty(H, W, 3, device=dev, dtype=torch.float32)
    alpha = torch.empty(H, W, device=dev, dtype=torch.float32)
    check(symbol("matpbr_path_denoise_diff_finish")(c.data_ptr(), k.data_ptr(), *(h.data_ptr() for h in hs), g.data_ptr(), H, W, sc, fg.data_ptr(),
                                                    delta.data_ptr(), alpha.data_ptr(), torch.cuda.current_stream(dev).cuda_stream),
          "matpbr_path_denoise_diff_finish")
    return fg, delta, alpha


@torch.no_grad()
def denoise_diff(A, B, alb, geom, scale: float = 1.0, workspace: Optional[torch.Tensor] = None, **params) -> tuple:
    """The differential render's filter on the device (the current torch stream): the triples A and B, the albedo guide alb [H,W,3] and
    the features geom [H,W,8] -> (fg', delta', alpha'), which `composite(fg', delta', alpha', photo, 1.0)` puts into the photograph.
    Equal to `denoise_diff_prepare`, `levels` calls of `denoise_diff_level` and `denoise_diff_finish`, bit for bit.  `workspace`: a uint8
    device tensor of at least matpbr_path_denoise_diff_workspace_bytes (default: allocated here)."""
    prm = denoise_params(**params)
    H, W = _geom_shape(torch.as_tensor(geom))
    sc = _composite_scale(scale)
    dev = _device_of(geom, alb, *A, *B)
    hs = _halves(A, B, H, W, lambda x, shape, what: _device_image(x, shape, what, dev))
    al, g = _device_image(alb, (H, W, 3), "alb", dev), _device_image(geom, (H, W, 8), "geom", dev)
    nbytes = int(symbol("matpbr_path_denoise_diff_workspace_bytes")(H, W))
    if workspace is None or workspace.numel() * workspace.element_size() < nbytes:
        workspace = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    fg, delta = torch.empty(H, W, 3, device=dev, dtype=torch.float32), torch.empty(H, W, 3, device=dev, dtype=torch.float32)
    alpha = torch.empty(H, W, device=dev, dtype=torch.float32)
    check(symbol("matpbr_path_denoise_diff")(*(h.data_ptr() for h in hs), g.data_ptr(), al.data_ptr(), H, W, sc, _prm_ptr(prm), fg.data_ptr(),
                                             delta.data_ptr(), alpha.data_ptr(), workspace.data_ptr(), nbytes,
                                             torch.cuda.current_stream(dev).cuda_stream), "matpbr_path_denoise_diff")
    return fg, delta, alpha


class PathTracer:
    """One mesh in the renderer's frame (camera at the origin looking down -z, `fov_x_deg` horizontal field of view, H x W pixels).
    The BVH is built once on the host and kept on the device; `render` takes the maps and the envmap of each frame.
    `objects`: meshes inserted into the scene ("Inserted objects"), in the same frame, outward winding, a list
    of {"vertices" [Nv,3], "triangles" [Nt,3], "bsdf": {"type": "dielectric", "int_ior": 1.49, "ext_ior": 1.000277} or
    {"type": "diffuse", "reflectance": (r, g, b)} or {"type": "pbr", "albedo": (r, g, b), "roughness": r, "metallic": m} (the depth
    mesh's own BSDF on constants; DESIGN.md section 1.4, "PBR inserted objects")} and optionally "normals" [Nv,3] (per vertex,
    outward): with them the object shades smooth, with the normals interpolated at each hit; without them flat.  An object with
    {"type": "area", "radiance": (r, g, b)} is an area light ("Emissive inserted objects"): it emits its
    radiance from its outward faces, reflects nothing, takes no "normals", and is sampled as an emitter beside the envmap at every
    vertex (`stats["n_lights"]` counts them; an envmap of zero luminance leaves the lights as the only emitters).  An object with
    {"type": "roughdielectric", "int_ior": 1.49, "ext_ior": 1.000277, "alpha": 0.1} is rough (frosted) glass (DESIGN.md section 1.4,
    "Rough dielectric objects"; `stats["n_rough_objects"]` counts them): it shades from both sides, takes "normals", and, unlike
    clear glass, takes an emitter sample at every vertex.  A diffuse or pbr object may carry "colors" [Nv,3] (per vertex, linear RGB in
    [0, 1]; DESIGN.md section 1.4, "Vertex-coloured inserted objects"; `stats["n_colored_objects"]` counts them): its reflectance or
    albedo is multiplied by the colour interpolated at each hit.  A diffuse or pbr object may carry "uv" [Nv,2] with "texture" [h,w,3]
    (base colour, linear, in [0, 1], row 0 the top row) and, a pbr one, "orm_texture" [h,w,3] ("Textured inserted
    objects"; `stats["n_textured_objects"]` counts them): the reflectance or the albedo is multiplied by the base colour, the roughness
    and the metallic by the orm image's g and b, each read with bilinear filtering and repeat wrapping at the coordinate interpolated
    at the hit.  A tracer with objects renders forward only."""

    def __init__(self, vertices: np.ndarray, triangles: np.ndarray, H: int, W: int, fov_x_deg: float = 35.0, device="cuda",
                 objects: Optional[Sequence[dict]] = None):
        self.H, self.W, self.fov = int(H), int(W), float(fov_x_deg)
        self.device = torch.device(device)
        n_scene = int(np.asarray(triangles).reshape(-1, 3).shape[0])
        self.objects = None
        self.obj_nrm: Optional[torch.Tensor] = None   # corner normals of the inserted triangles, when some object is smooth
        self.n_scene_tris = n_scene
        self.pbr = None                               # the PathObjectPbr records, when some object is of kind BSDF_PBR
        self.lights = None                            # (PathLights, tris, cdf on the device), when some object is of kind BSDF_AREA
        self.rough = False                            # some object is of kind BSDF_ROUGH_DIELECTRIC: `render` takes the rough entry point
        self.obj_col: Optional[torch.Tensor] = None   # corner colours of the inserted triangles, when some object is coloured
        self.textures = None                          # (obj_uv, PathObjectTex records, texels on the device), when some object is textured
        n_smooth = n_pbr = n_lights = n_rough = n_colored = n_textured = 0
        if objects:
            vertices, triangles, table, corner, records, lt, tint, tex = merge_objects(vertices, triangles, objects, normals=True, pbr=True,
                                                                                       lights=True, colors=True, textures=True)
            self.objects = (PathObject * len(table))(*table)
            n_smooth = sum(1 for t in table if t.kind & OBJECT_SMOOTH)
            n_pbr = sum(1 for t in table if t.kind & ~OBJECT_FLAGS == BSDF_PBR)
            n_rough = sum(1 for t in table if t.kind & ~OBJECT_SMOOTH == BSDF_ROUGH_DIELECTRIC)
            n_colored = sum(1 for t in table if t.kind & OBJECT_COLORED)
            n_textured = sum(1 for t in table if t.kind & OBJECT_TEXTURED)
            for have, level in ((lt is not None, "lights"), (n_rough, "rough"), (n_pbr, "pbr"), (corner is not None, "normals"),
                                (tint is not None, "colors"), (tex is not None, "textures")):
                if have:                              # a library built before the feature: PathError now, not at the first render
                    symbol("matpbr_path_render_objects_" + level)
            if tint is not None:
                symbol("matpbr_path_feature_colors")
                self.obj_col = torch.from_numpy(tint).to(self.device)
            if tex is not None:
                symbol("matpbr_path_feature_tints")
                self.textures = (torch.from_numpy(tex[0]).to(self.device), (PathObjectTex * len(tex[1]))(*tex[1]),
                                 torch.from_numpy(tex[2]).to(self.device))
            if lt is not None:
                n_lights = int(lt["header"].n_lights)
                self.lights = (lt["header"], torch.from_numpy(lt["tris"]).to(self.device), torch.from_numpy(lt["cdf"]).to(self.device))
            self.rough = n_rough > 0
            if n_pbr or lt is not None or n_rough or n_colored or n_textured:   # the entry points from the lights' on take the records beside the table as well
                self.pbr = (PathObjectPbr * len(records))(*records)
            if corner is not None:
                self.obj_nrm = torch.from_numpy(corner).to(self.device)
            bvh = build_bvh(vertices, triangles, n_scene)
        else:
            bvh = build_bvh(vertices, triangles)
        self.stats = {k: bvh[k] for k in ("n_nodes", "depth", "n_leaves", "build_s")}
        self.stats["n_tris"] = int(np.asarray(triangles).reshape(-1, 3).shape[0])
        self.stats["n_objects"] = len(self.objects) if self.objects is not None else 0
        self.stats["n_object_tris"] = self.stats["n_tris"] - n_scene
        self.stats["n_smooth_objects"] = n_smooth
        self.stats["n_pbr_objects"] = n_pbr
        self.stats["n_lights"] = n_lights
        self.stats["n_rough_objects"] = n_rough
        self.stats["n_colored_objects"] = n_colored
        self.stats["n_textured_objects"] = n_textured
        self.stats["bytes"] = int(bvh["nodes"].nbytes + bvh["tris"].nbytes)
        self.nodes = torch.from_numpy(bvh["nodes"]).to(self.device)
        self.tris = torch.from_numpy(bvh["tris"]).to(self.device)
        self._ws: Optional[torch.Tensor] = None      # render_bwd's workspace, kept between calls
        self._dn_ws: Optional[torch.Tensor] = None   # denoise's

    def _tables(self, env: torch.Tensor):
        tab = env_tables(env.cpu().numpy())          # host, fp64 -> fp32: microseconds for the 16 x 32 maps of the pipeline
        return (env.contiguous(), *(torch.from_numpy(np.ascontiguousarray(tab[k])).to(self.device) for k in ("row_cdf", "col_cdf", "pdf")))

    def tables(self, envmap) -> tuple:
        """(env, row_cdf, col_cdf, pdf) on the device for `render` / `render_bwd`'s `tables=`: hold them fixed across calls."""
        env = torch.as_tensor(envmap).to(self.device, torch.float32)
        if env.dim() != 3 or env.shape[2] != 3:
            raise ValueError(f"envmap must be [He,We,3], got {tuple(env.shape)}")
        return self._tables(env)

    def _inputs(self, albedo, roughness, metallic, envmap, tables):
        H, W, dev = self.H, self.W, self.device
        f = lambda x, c: torch.as_tensor(x).to(dev, torch.float32).reshape(H, W, c).contiguous()
        a, r, m = f(albedo, 3), f(roughness, 1), f(metallic, 1)
        if tables is None:
            env, row, col, pdf = self.tables(envmap)
        else:
            _, row, col, pdf = tables
            env = torch.as_tensor(envmap).to(dev, torch.float32).contiguous()
            if tuple(env.shape) != tuple(pdf.shape) + (3,):
                raise ValueError(f"envmap {tuple(env.shape)} does not match its tables {tuple(pdf.shape)}")
        return a, r, m, env, row, col, pdf

    def _frame(self, a, r, m, env, row, col, pdf, spp, max_depth, seed, spp_per_launch) -> tuple:
        """The 18 common arguments of a render or a backward pass (SIGNATURES' _FRAME) over what `_inputs` returned."""
        return (self.nodes.data_ptr(), self.tris.data_ptr(), a.data_ptr(), r.data_ptr(), m.data_ptr(), self.H, self.W, self.fov,
                env.data_ptr(), row.data_ptr(), col.data_ptr(), pdf.data_ptr(), int(env.shape[0]), int(env.shape[1]),
                int(spp), int(max_depth), int(seed) & 0xFFFFFFFF, int(spp_per_launch))

    def _normal(self, normal, what: str) -> torch.Tensor:
        """The shading-normal map [H,W,3] on the device, used as given; `what` names the caller in the refusals."""
        if self.objects is not None:
            raise ValueError(f"{what} knows no shading normals on a tracer with inserted objects: build the PathTracer without `objects`")
        nrm = torch.as_tensor(normal)
        if tuple(nrm.shape) != (self.H, self.W, 3):
            raise ValueError(f"normal must be [{self.H},{self.W},3], got {tuple(nrm.shape)}")
        return nrm.to(self.device, torch.float32).contiguous()

    def object_args(self) -> tuple:
        """(table, n_objects, obj_nrm, n_scene_tri, records, lights header, light_tris, light_cdf, obj_col, obj_uv, texture records, texels,
        n_texels): the object arguments of a forward entry point after `stream`, as the C ABI takes them, None where the tracer has
        none.  An entry takes the first OBJECT_ENTRIES[its name] of them.  The last four are there on a tracer with a textured object
        only, the one whose `render` takes the entry that reads them: a tracer without one returns the nine values it always has."""
        ptr = lambda t: t.data_ptr() if t is not None else None
        table, records = _table_ptrs(self.objects, self.pbr)
        head, ltris, lcdf = self.lights if self.lights is not None else (None, None, None)
        return (table, len(self.objects) if self.objects is not None else 0, ptr(self.obj_nrm), self.n_scene_tris, records,
                ctypes.cast(ctypes.byref(head), _P) if head is not None else None, ptr(ltris), ptr(lcdf), ptr(self.obj_col),
                *(self._texture_args() if self.textures is not None else ()))

    def _texture_args(self) -> tuple:
        """(obj_uv, texture records, texels, n_texels) as the C ABI takes them; (None, None, None, 0) without a textured object."""
        if self.textures is None:
            return None, None, None, 0
        uv, rec, texels = self.textures
        return (uv.data_ptr(), *_tex_ptrs(self.objects, rec, texels))

    @torch.no_grad()
    def render(self, albedo: torch.Tensor, roughness: torch.Tensor, metallic: torch.Tensor, envmap, spp: int = 64, max_depth: int = 4,
               seed: int = 0, spp_per_launch: int = 8, out: Optional[torch.Tensor] = None, rays: Optional[torch.Tensor] = None,
               tables: Optional[tuple] = None, normal=None) -> torch.Tensor:
        """-> linear radiance [H,W,3] on the current torch stream.  albedo [H,W,3], roughness / metallic [H,W] or [H,W,1], envmap
        [He,We,3] (tensor or array, the `sh.py` equirectangular convention).  Every split into launches of `spp_per_launch` samples gives
        the same bits.  `rays` (optional int32 [H,W] on the device): the rays each pixel traced are added to it.  `tables`: what
        `tables(envmap)` returned (default: built from `envmap` now).  `normal` [H,W,3] (unit length, used as given): the shading-normal
        map ("Shading normals"); None shades with the face normals.  A tracer with objects refuses it."""
        H, W, dev = self.H, self.W, self.device
        nrm = self._normal(normal, "render") if normal is not None else None
        inputs = self._inputs(albedo, roughness, metallic, envmap, tables)
        if out is None:
            out = torch.empty(H, W, 3, device=dev, dtype=torch.float32)
        lib = load()
        args = (*self._frame(*inputs, spp, max_depth, seed, spp_per_launch), out.data_ptr(), rays.data_ptr() if rays is not None else None,
                torch.cuda.current_stream(dev).cuda_stream)
        if nrm is not None:
            entry, own = "matpbr_path_render_normals", (nrm.data_ptr(),)
        elif self.objects is None:
            entry, own = "matpbr_path_render", ()
        else:
            entry = "matpbr_path_render_objects" + ("_textures" if self.textures is not None else "_colors" if self.obj_col is not None else "_rough" if self.rough else "_lights" if self.lights is not None else
                                                    "_pbr" if self.pbr is not None else "_normals" if self.obj_nrm is not None else "")
            own = self.object_args()[:OBJECT_ENTRIES[entry]]
        check(symbol(entry, lib)(*args, *own), entry)
        return out

    @torch.no_grad()
    def render_diff(self, albedo: torch.Tensor, roughness: torch.Tensor, metallic: torch.Tensor, envmap, spp: int = 64, max_depth: int = 4,
                    seed: int = 0, spp_per_launch: int = 8, tables: Optional[tuple] = None, rays: Optional[torch.Tensor] = None) -> tuple:
        """The differential render ("Differential render") with `render`'s arguments and random numbers ->
        (fg [H,W,3], delta [H,W,3], alpha [H,W], rewalked [H,W] int32) on the device, the first three means over `spp`.  fg: the radiance
        of the samples whose camera ray lands on an inserted object; alpha: their share; delta: what the objects add to and take from
        the other samples, the sample's radiance minus the same sample's walked again without the objects, over the samples whose first
        walk met an object (`rewalked` counts them; every sample that misses the objects, where the table holds a light).  Where
        rewalked is 0, delta is exactly 0.  `composite` puts them into a photograph.  Every split into launches gives the same bits.  A
        tracer without objects raises ValueError."""
        if self.objects is None:
            raise ValueError("render_diff renders what inserted objects change: build the PathTracer with `objects`")
        fn = symbol("matpbr_path_render_objects_diff")
        H, W, dev = self.H, self.W, self.device
        inputs = self._inputs(albedo, roughness, metallic, envmap, tables)
        fg, delta = torch.empty(H, W, 3, device=dev, dtype=torch.float32), torch.empty(H, W, 3, device=dev, dtype=torch.float32)
        alpha, rewalked = torch.empty(H, W, device=dev, dtype=torch.float32), torch.zeros(H, W, device=dev, dtype=torch.int32)
        check(fn(*self._frame(*inputs, spp, max_depth, seed, spp_per_launch), rays.data_ptr() if rays is not None else None,
                 torch.cuda.current_stream(dev).cuda_stream, *self.object_args()[:9], *self._texture_args(), fg.data_ptr(), delta.data_ptr(),
                 alpha.data_ptr(), rewalked.data_ptr()), "matpbr_path_render_objects_diff")
        return fg, delta, alpha, rewalked

    @torch.no_grad()
    def render_diff_through(self, albedo: torch.Tensor, roughness: torch.Tensor, metallic: torch.Tensor, envmap, photo, spp: int = 64,
                            max_depth: int = 4, seed: int = 0, spp_per_launch: int = 8, tables: Optional[tuple] = None,
                            rays: Optional[torch.Tensor] = None) -> tuple:
        """`render_diff` with the photograph seen through inserted glass ("Seen through glass") ->
        (fg [H,W,3], delta [H,W,3], alpha [H,W], through [H,W,3], rewalked [H,W] int32).  `photo` [H,W,3]: the photograph, linear, finite
        and >= 0.  A sample whose camera ray lands on an object and leaves it through clear glass alone (smooth or flat dielectric
        vertices) onto the depth mesh's front adds throughput x photo at the landing point's texel to `through`; its fg is then what
        the objects change in the landing point's light (the sample minus its tail walked again without the objects, where that walk
        met one; nothing where it met none), and may be negative.  Rough glass, chains that end on another object, on a light, on the
        envmap or inside the glass at max_depth keep `render_diff`'s rule.  delta and alpha are `render_diff`'s bits; `rewalked`
        counts both kinds of second walk.  The picture is `composite(fg + through, delta, alpha, photo)`.  Every split into launches
        gives the same bits.  A tracer without objects, or a photograph of another shape, raises ValueError."""
        if self.objects is None:
            raise ValueError("render_diff_through renders what inserted objects change: build the PathTracer with `objects`")
        ph = torch.as_tensor(photo)
        if tuple(ph.shape) != (self.H, self.W, 3):
            raise ValueError(f"photo must be [{self.H},{self.W},3], got {tuple(ph.shape)}")
        fn = symbol("matpbr_path_render_objects_through")
        H, W, dev = self.H, self.W, self.device
        ph = ph.to(dev, torch.float32).contiguous()
        inputs = self._inputs(albedo, roughness, metallic, envmap, tables)
        fg, delta = torch.empty(H, W, 3, device=dev, dtype=torch.float32), torch.empty(H, W, 3, device=dev, dtype=torch.float32)
        alpha, rewalked = torch.empty(H, W, device=dev, dtype=torch.float32), torch.zeros(H, W, device=dev, dtype=torch.int32)
        through = torch.empty(H, W, 3, device=dev, dtype=torch.float32)
        check(fn(*self._frame(*inputs, spp, max_depth, seed, spp_per_launch), rays.data_ptr() if rays is not None else None,
                 torch.cuda.current_stream(dev).cuda_stream, *self.object_args()[:9], *self._texture_args(), fg.data_ptr(), delta.data_ptr(),
                 alpha.data_ptr(), rewalked.data_ptr(), ph.data_ptr(), through.data_ptr()), "matpbr_path_render_objects_through")
        return fg, delta, alpha, through, rewalked

    @torch.no_grad()
    def features(self, normal=None) -> torch.Tensor:
        """geom [H,W,8] on the device: per pixel (p, rho) and (n, id) of the camera ray through the pixel centre, the denoiser's guides
        ("Denoiser").  n is the normal `render` shades that camera vertex with: `normal` [H,W,3] is the
        shading-normal map of `render` (a tracer with objects refuses it); id -1 = no hit, 0 = the depth mesh, 1 + k = object k."""
        nrm = self._normal(normal, "features") if normal is not None else None
        geom = torch.empty(self.H, self.W, 8, device=self.device, dtype=torch.float32)
        check(symbol("matpbr_path_features")(self.nodes.data_ptr(), self.tris.data_ptr(), self.H, self.W, self.fov, _table_ptrs(_uncolored(self.objects))[0],
                                             len(self.objects) if self.objects is not None else 0,
                                             self.obj_nrm.data_ptr() if self.obj_nrm is not None else None, self.n_scene_tris,
                                             nrm.data_ptr() if nrm is not None else None, geom.data_ptr(),
                                             torch.cuda.current_stream(self.device).cuda_stream), "matpbr_path_features")
        return geom

    @torch.no_grad()
    def feature_colors(self) -> torch.Tensor:
        """[H,W,3] on the device: the interpolated colour where the camera ray through the pixel centre (`features`' ray) first hits a
        vertex-coloured object, (1, 1, 1) elsewhere: what `relight.albedo_guide` multiplies a coloured object's constant by."""
        out = torch.empty(self.H, self.W, 3, device=self.device, dtype=torch.float32)
        check(symbol("matpbr_path_feature_colors")(self.nodes.data_ptr(), self.tris.data_ptr(), self.H, self.W, self.fov,
                                                   _table_ptrs(_uncolored(self.objects, OBJECT_TEXTURED))[0],
                                                   len(self.objects) if self.objects is not None else 0, self.n_scene_tris,
                                                   self.obj_col.data_ptr() if self.obj_col is not None else None, out.data_ptr(),
                                                   torch.cuda.current_stream(self.device).cuda_stream), "matpbr_path_feature_colors")
        return out

    @torch.no_grad()
    def feature_tints(self) -> torch.Tensor:
        """[H,W,3] on the device: the interpolated colour times the base-colour fetch where the camera ray through the pixel centre
        (`features`' ray) first hits a coloured or textured object, (1, 1, 1) elsewhere: `feature_colors` with the textures, what
        `relight.albedo_guide` multiplies a textured object's constant by."""
        out = torch.empty(self.H, self.W, 3, device=self.device, dtype=torch.float32)
        check(symbol("matpbr_path_feature_tints")(self.nodes.data_ptr(), self.tris.data_ptr(), self.H, self.W, self.fov, _table_ptrs(self.objects)[0],
                                                  len(self.objects) if self.objects is not None else 0, self.n_scene_tris,
                                                  self.obj_col.data_ptr() if self.obj_col is not None else None, *self._texture_args(),
                                                  out.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream), "matpbr_path_feature_tints")
        return out

    @torch.no_grad()
    def denoise(self, A, B, alb, geom, **params) -> torch.Tensor:
        """The a-trous filter over two half renders A, B [H,W,3] of this tracer (independent seeds, the same sample count), guided by
        the albedo alb [H,W,3] and `features()` -> the denoised mean [H,W,3].  `params`: levels, sigma_n, sigma_x, sigma_a, sigma_c
        (default DENOISE_DEFAULTS).  Forward only."""
        if tuple(torch.as_tensor(geom).shape) != (self.H, self.W, 8):
            raise ValueError(f"geom must be [{self.H},{self.W},8], got {list(torch.as_tensor(geom).shape)}")
        nbytes = int(symbol("matpbr_path_denoise_workspace_bytes")(self.H, self.W))
        if self._dn_ws is None or self._dn_ws.numel() < nbytes:
            self._dn_ws = torch.empty(nbytes, device=self.device, dtype=torch.uint8)
        to = lambda x: x.to(self.device) if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x)).to(self.device)
        return denoise(to(A), to(B), to(alb), to(geom), workspace=self._dn_ws, **params)

    @torch.no_grad()
    def denoise_diff(self, A, B, alb, geom, scale: float = 1.0, **params) -> tuple:
        """The a-trous filter over two halves of `render_diff` ("Denoiser for the differential render"): A and B
        are (fg, delta, alpha) triples, each a sum over the same number of frames with independent seeds and equal spp, `scale` 1 / (the
        frames summed per half) -> (fg', delta', alpha'), which `composite(fg', delta', alpha', photo, 1.0)` puts into the photograph.
        Each pixel's own layer is filtered (fg where the camera ray through its centre lands on an object, delta elsewhere); the other
        layer and alpha pass through as their means.  `params`: `denoise`'s.  Forward only."""
        if tuple(torch.as_tensor(geom).shape) != (self.H, self.W, 8):
            raise ValueError(f"geom must be [{self.H},{self.W},8], got {list(torch.as_tensor(geom).shape)}")
        nbytes = int(symbol("matpbr_path_denoise_diff_workspace_bytes")(self.H, self.W))
        if self._dn_ws is None or self._dn_ws.numel() < nbytes:
            self._dn_ws = torch.empty(nbytes, device=self.device, dtype=torch.uint8)
        to = lambda x: x.to(self.device) if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x)).to(self.device)
        return denoise_diff(tuple(map(to, A)), tuple(map(to, B)), to(alb), to(geom), scale, workspace=self._dn_ws, **params)

    @torch.no_grad()
    def render_trans(self, albedo: torch.Tensor, roughness: torch.Tensor, metallic: torch.Tensor, envmap, mask, bg, ior: float = 1.2,
                     spec_trans: float = 0.4, refract_distance: float = 100.0, spp: int = 64, max_depth: int = 4, seed: int = 0,
                     spp_per_launch: int = 8, tables: Optional[tuple] = None, rays: Optional[torch.Tensor] = None, normal=None) -> torch.Tensor:
        """`render` with the depth mesh shading as the reference's TransBSDF ("Transparency editing"): where
        `mask` [H,W] (bool) is set the surface is glass of index `ior` and transmission `spec_trans` over the picture `bg` [H,W,3].
        The maps are used as given (`relight.render_trans` edits them inside the mask first).  Forward only: there is no backward
        pass through it, a tracer with inserted objects refuses it, and it refuses a shading-normal map (`normal`)."""
        if normal is not None:
            raise ValueError("render_trans knows no shading normals: the transparency edit shades with the face normals")
        if self.objects is not None:
            raise ValueError("render_trans knows no inserted objects: build the PathTracer without `objects`")
        H, W, dev = self.H, self.W, self.device
        mk, bgt = torch.as_tensor(mask), torch.as_tensor(bg)
        if tuple(mk.shape) != (H, W):
            raise ValueError(f"mask must be [{H},{W}], got {tuple(mk.shape)}")
        if tuple(bgt.shape) != (H, W, 3):
            raise ValueError(f"bg must be [{H},{W},3], got {tuple(bgt.shape)}")
        ed = trans_edit(ior, spec_trans, refract_distance)
        mk = (mk != 0).to(dev, torch.uint8).contiguous()
        bgt = bgt.to(dev, torch.float32).contiguous()
        inputs = self._inputs(albedo, roughness, metallic, envmap, tables)
        out = torch.empty(H, W, 3, device=dev, dtype=torch.float32)
        check(load().matpbr_path_render_trans(*self._frame(*inputs, spp, max_depth, seed, spp_per_launch), out.data_ptr(),
                                              rays.data_ptr() if rays is not None else None, torch.cuda.current_stream(dev).cuda_stream,
                                              mk.data_ptr(), bgt.data_ptr(), ctypes.cast(ctypes.byref(ed), _P)), "matpbr_path_render_trans")
        return out

    @torch.no_grad()
    def render_bwd(self, albedo: torch.Tensor, roughness: torch.Tensor, metallic: torch.Tensor, envmap, d_out: torch.Tensor, spp: int = 64,
                   max_depth: int = 4, seed: int = 0, spp_per_launch: int = 8, want=("a", "r", "m", "env"), grads: Optional[dict] = None,
                   tables: Optional[tuple] = None, rays: Optional[torch.Tensor] = None, normal=None) -> Dict[str, torch.Tensor]:
        """The backward pass of `render` with the same arguments: d loss / d {"a" [H,W,3], "r" [H,W,1], "m" [H,W,1], "env" [He,We,3]}
        for d_out = d loss / d render [H,W,3], for the keys in `want`.  The derivative of the fixed-seed estimator with the sampling
        detached; bit-identical for every `spp_per_launch`.  `grads`: device buffers to ADD to (by key; the
        missing ones start from zero).  `rays` (optional int32 [H,W]): the rays both replays traced are added to it.  `normal`: the
        shading-normal map of `render`; with it `want` may hold "n", d loss / d normal [H,W,3] with respect to the map's components as
        free variables (normalising is the caller's)."""
        if self.objects is not None:
            raise ValueError("render_bwd knows no inserted objects: build the PathTracer without `objects` for gradients")
        if "n" in want and normal is None:
            raise ValueError("want 'n' needs the shading-normal map it is the gradient of: pass `normal`")
        nrm = self._normal(normal, "render_bwd") if normal is not None else None
        H, W, dev = self.H, self.W, self.device
        inputs = self._inputs(albedo, roughness, metallic, envmap, tables)
        He, We = int(inputs[3].shape[0]), int(inputs[3].shape[1])
        d_out = torch.as_tensor(d_out).to(dev, torch.float32).reshape(H, W, 3).contiguous()
        shapes = {"a": (H, W, 3), "r": (H, W, 1), "m": (H, W, 1), "env": (He, We, 3), "n": (H, W, 3)}
        grads = dict(grads or {})
        for k in want:
            if k not in shapes:
                raise ValueError(f"want: keys of {tuple(shapes)}, got {k!r}")
            if k not in grads:
                grads[k] = torch.zeros(shapes[k], device=dev, dtype=torch.float32)
            g = grads[k]
            if tuple(g.shape) != shapes[k] or g.dtype != torch.float32 or not g.is_contiguous() or g.device.type != dev.type:
                raise ValueError(f"grads[{k!r}] must be contiguous float32 {shapes[k]} on {dev}")
        if "env" in want and He * We > MAX_BWD_ENV_TEXELS:
            raise ValueError(f"the envmap gradient needs He * We <= {MAX_BWD_ENV_TEXELS}, got {He} x {We}")
        lib = load()
        size = lib.matpbr_path_render_bwd_workspace_bytes if nrm is None else lib.matpbr_path_render_bwd_normals_workspace_bytes
        nbytes = int(size(H, W, He, We))
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        ptr = lambda k: grads[k].data_ptr() if k in want else None
        args = (*self._frame(*inputs, spp, max_depth, seed, spp_per_launch), d_out.data_ptr(), ptr("a"), ptr("r"), ptr("m"), ptr("env"),
                self._ws.data_ptr(), nbytes, rays.data_ptr() if rays is not None else None, torch.cuda.current_stream(dev).cuda_stream)
        if nrm is None:
            check(lib.matpbr_path_render_bwd(*args), "matpbr_path_render_bwd")
        else:
            check(lib.matpbr_path_render_bwd_normals(*args, nrm.data_ptr(), ptr("n")), "matpbr_path_render_bwd_normals")
        return {k: grads[k] for k in want}


class PathRenderFn(torch.autograd.Function):
    """out = PathTracer.render(a, r, m, env[, normal=nrm]) (bit for bit), differentiable in a [H,W,3], r [H,W,1], m [H,W,1], env
    [He,We,3] and the shading-normal map nrm [H,W,3] (None: face normals) by `render_bwd` with the forward's seed.  `ctx_in`:
    {"tracer", "spp", "max_depth", "seed", "spp_per_launch"} and the envmap-table cache `PathTables`."""

    @staticmethod
    def forward(ctx, a, r, m, env, ctx_in, nrm=None):
        tracer = ctx_in["tracer"]
        tabs = ctx_in["tables"].get(tracer, env)
        kw = {k: ctx_in[k] for k in ("spp", "max_depth", "seed", "spp_per_launch")}
        out = tracer.render(a.detach(), r.detach(), m.detach(), env.detach(), tables=tabs, normal=None if nrm is None else nrm.detach(), **kw)
        ctx.save_for_backward(a, r, m, env, *(() if nrm is None else (nrm,)))
        ctx.tracer, ctx.tabs, ctx.kw = tracer, tabs, kw
        return out

    @staticmethod
    def backward(ctx, d_out):
        a, r, m, env, *rest = ctx.saved_tensors
        nrm = rest[0] if rest else None
        need = ctx.needs_input_grad
        need = need[:4] + (bool(nrm is not None and need[5]),)
        want = [k for k, n in zip(("a", "r", "m", "env", "n"), need) if n]
        g = ctx.tracer.render_bwd(a.detach(), r.detach(), m.detach(), env.detach(), d_out, want=want, tables=ctx.tabs,
                                  normal=None if nrm is None else nrm.detach(), **ctx.kw) if want else {}
        return (g["a"].reshape(a.shape) if need[0] else None, g["r"].reshape(r.shape) if need[1] else None,
                g["m"].reshape(m.shape) if need[2] else None, g["env"].reshape(env.shape) if need[3] else None, None,
                g["n"].reshape(nrm.shape) if need[4] else None)


class PathTables:
    """The envmap's sampling tables, rebuilt only when the envmap tensor is another object or its version counter moved (an in-place
    optimiser step)."""

    def __init__(self):
        self._key, self._tabs = None, None

    def get(self, tracer: PathTracer, env: torch.Tensor) -> tuple:
        key = (env, env._version, tuple(env.shape))
        if self._key is None or self._key[0] is not env or self._key[1:] != key[1:]:
            self._tabs = tracer.tables(env.detach())
            self._key = key
        return self._tabs
