"""The ctypes ABI of libmatpbr_path.so (include/matpbr_path.h): its constants, structures and signatures, the symbols grouped by the
feature they came with, `load` / `symbol` / `check`, and the helpers that turn arrays and tables into the pointers the C ABI takes.
The path render's other modules (path_scene, path_host, path_filters, pathtrace) sit on this one.  There is no fallback: a missing
or failing library raises."""
import ctypes
import threading
from typing import Optional

import numpy as np

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
OBJECT_MEDIUM = 0x800          # MATPBR_PATH_OBJECT_MEDIUM, OR-ed into the kind of a dielectric or roughdielectric object ("Media inside glass")
OBJECT_PHOTO = 0x1000          # MATPBR_PATH_OBJECT_PHOTO, OR-ed into the kind of a diffuse, pbr or roughdielectric object ("Reflected in inserted objects")
MEDIUM_MAX_G = 0.99            # |g| of the Henyey-Greenstein phase function at most this
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


class PathObjectMedium(ctypes.Structure):
    """MatpbrPathObjectMedium (include/matpbr_path.h): absorption per channel, grey scattering (both per scene unit) and the
    Henyey-Greenstein asymmetry of the medium inside one glass object."""
    _fields_ = [("sigma_a", ctypes.c_float * 3), ("sigma_s", ctypes.c_float), ("g", ctypes.c_float), ("reserved", ctypes.c_float * 3)]


class PathLights(ctypes.Structure):
    """MatpbrPathLights (include/matpbr_path.h): the per-light header of a table with objects of kind BSDF_AREA."""
    _fields_ = [("n_lights", ctypes.c_int32), ("object", ctypes.c_int32 * MAX_OBJECTS), ("first", ctypes.c_int32 * MAX_OBJECTS),
                ("n_tri", ctypes.c_int32 * MAX_OBJECTS), ("area", ctypes.c_float * MAX_OBJECTS)]


class PathXform(ctypes.Structure):
    """MatpbrPathXform (include/matpbr_path.h): one object's pose, p' = R (s (p - c)) + c + t."""
    _fields_ = [("R", ctypes.c_float * 9), ("s", ctypes.c_float), ("t", ctypes.c_float * 3), ("c", ctypes.c_float * 3)]


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
# the thirteen object arguments (`PathTracer.object_args()`): objects, n_objects, obj_nrm, n_scene_tri, pbr, lights, light_tris, light_cdf,
# obj_col, obj_uv, tex, texels, n_texels
_OBJECTS = [_P, ctypes.c_int, _P, ctypes.c_long] + [_P] * 8 + [ctypes.c_long]
# the object entry points, one per level of DESIGN.md section 1.4, "The object entries" -> how many of `PathTracer.object_args()` each takes
OBJECT_ENTRIES = {"matpbr_path_render_objects": 2, "matpbr_path_render_objects_normals": 4, "matpbr_path_render_objects_pbr": 5,
                  "matpbr_path_render_objects_lights": 8, "matpbr_path_render_objects_rough": 8, "matpbr_path_render_objects_colors": 9,
                  "matpbr_path_render_objects_textures": 13, "matpbr_path_render_objects_through": 13}
# level 8 takes the thirteen of level 7 and then the medium records (`PathTracer.media_arg`), which `object_args()` does not hold
MEDIA_ENTRY = "matpbr_path_render_objects_media"
# the differential family -> how many of (photo, through, base, media) each takes after rays, stream, the thirteen object arguments and
# fg, delta, alpha, rewalked
DIFF_ENTRIES = {"matpbr_path_render_objects_diff": 0, "matpbr_path_render_objects_through": 2, "matpbr_path_render_objects_ratio": 3,
                "matpbr_path_render_objects_diff_media": 4, "matpbr_path_render_objects_reflect": 4}
SIGNATURES = {
    **{name: (ctypes.c_int, _RENDER + _OBJECTS[:n]) for name, n in OBJECT_ENTRIES.items() if name not in DIFF_ENTRIES},
    MEDIA_ENTRY: (ctypes.c_int, _RENDER + _OBJECTS + [_P]),
    **{name: (ctypes.c_int, _FRAME + [_P, _P] + _OBJECTS + [_P] * (4 + n)) for name, n in DIFF_ENTRIES.items()},
    "matpbr_path_version": (ctypes.c_int, []),
    "matpbr_path_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "matpbr_path_bvh_size": (ctypes.c_int, [ctypes.c_long, _P]),
    "matpbr_path_bvh_build": (ctypes.c_int, [_P, ctypes.c_long, _P, ctypes.c_long, _P, ctypes.c_long, _P, _P, _P, _P]),
    "matpbr_path_bvh_build_objects": (ctypes.c_int, [_P, ctypes.c_long, _P, ctypes.c_long, ctypes.c_long, _P, ctypes.c_long, _P, _P, _P, _P]),
    "matpbr_path_trace_host": (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_long, ctypes.c_float, ctypes.c_float, _P, _P]),
    "matpbr_path_env_tables": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, _P, _P, _P, _P]),
    "matpbr_path_env_sample_host": (ctypes.c_int, [_P, _P, _P, ctypes.c_int, ctypes.c_int, _P, ctypes.c_long, _P, _P, _P]),
    "matpbr_path_render": (ctypes.c_int, _RENDER),
    "matpbr_path_object_sample_host": (ctypes.c_int, [_P] * 4 + [ctypes.c_long] + [_P] * 4),
    "matpbr_path_object_normal_host": (ctypes.c_int, [_P] * 4 + [ctypes.c_long] + [_P] * 3),
    "matpbr_path_object_lookup_host": (ctypes.c_int, [_P, ctypes.c_int, _P, _P, ctypes.c_long, _P, _P, _P, _P]),
    "matpbr_path_light_tables": (ctypes.c_int, [_P, ctypes.c_long, _P, ctypes.c_long, _P, ctypes.c_int, _P, _P, _P, _P, ctypes.c_long, _P]),
    "matpbr_path_light_sample_host": (ctypes.c_int, [_P, _P, _P, ctypes.c_long, ctypes.c_int, _P, _P, ctypes.c_long] + [_P] * 7),
    "matpbr_path_light_pdf_host": (ctypes.c_int, [_P, _P, ctypes.c_long, ctypes.c_int, _P, _P, _P, _P, ctypes.c_long, _P, _P]),
    "matpbr_path_rough_sample_host": (ctypes.c_int, [_P] * 5 + [ctypes.c_long] + [_P] * 4),
    "matpbr_path_rough_eval_host": (ctypes.c_int, [_P] * 5 + [ctypes.c_long] + [_P] * 2),
    "matpbr_path_object_sample_shading_host": (ctypes.c_int, [_P] * 5 + [ctypes.c_long] + [_P] * 4),
    "matpbr_path_object_color_host": (ctypes.c_int, [_P] * 4 + [ctypes.c_long] + [_P] * 3),
    "matpbr_path_feature_colors": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_float, _P, ctypes.c_int, ctypes.c_long, _P, _P, _P]),
    "matpbr_path_feature_colors_host": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_float, _P, ctypes.c_int, ctypes.c_long, _P, _P]),
    "matpbr_path_object_texture_host": (ctypes.c_int, [_P] * 4 + [ctypes.c_long, _P, _P, ctypes.c_long] + [_P] * 5),
    "matpbr_path_feature_tints": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_float, _P, ctypes.c_int, ctypes.c_long, _P, _P, _P, _P,
                                                 ctypes.c_long, _P, _P]),
    "matpbr_path_feature_tints_host": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_float, _P, ctypes.c_int, ctypes.c_long, _P, _P, _P, _P,
                                                      ctypes.c_long, _P]),
    "matpbr_path_reflect_chain_host": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_long, _P, _P, _P, _P,
                                                      ctypes.c_long] + [_P] * 5),
    "matpbr_path_render_edit_diff": (ctypes.c_int, _FRAME + [_P, _P] + [_P] * 8),
    "matpbr_path_render_relight": (ctypes.c_int, _FRAME + [_P, _P] + [_P] * 4 + [ctypes.c_int, ctypes.c_int] + [_P] * 3),
    "matpbr_path_composite_relight": (ctypes.c_int, [_P] * 3 + [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, _P, _P]),
    "matpbr_path_composite_relight_host": (ctypes.c_int, [_P] * 3 + [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, _P]),
    "matpbr_path_medium_segment_host": (ctypes.c_int, [_P, _P, _P, ctypes.c_long, _P, _P, _P]),
    "matpbr_path_phase_sample_host": (ctypes.c_int, [ctypes.c_float, _P, _P, ctypes.c_long, _P]),
    "matpbr_path_composite_ratio": (ctypes.c_int, [_P] * 5 + [ctypes.c_int, ctypes.c_int, ctypes.c_float, _P, _P]),
    "matpbr_path_composite_ratio_host": (ctypes.c_int, [_P] * 5 + [ctypes.c_int, ctypes.c_int, ctypes.c_float, _P]),
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
    "matpbr_path_bvh_build_grafted": (ctypes.c_int, [_P, ctypes.c_long, ctypes.c_long, _P, ctypes.c_long, ctypes.c_long, ctypes.c_double, _P, ctypes.c_long] + [_P] * 9),
    "matpbr_path_xform_check_host": (ctypes.c_int, [_P, ctypes.c_int]),
    "matpbr_path_objects_move": (ctypes.c_int, [_P] * 3 + [ctypes.c_long] * 4 + [_P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_float] + [_P] * 4 +
                                 [ctypes.c_long, _P, _P]),
    "matpbr_path_objects_move_host": (ctypes.c_int, [_P] * 3 + [ctypes.c_long] * 4 + [_P, ctypes.c_int, _P, ctypes.c_int, _P, ctypes.c_float] + [_P] * 4 +
                                      [ctypes.c_long, _P]),
}
VERSION = 3
MAX_BWD_ENV_TEXELS = 1024
# the symbols added at version 3, by the feature each group came with, as `symbol` names it, in the order the features were merged: a
# version-3 library built before one of them loads, and `symbol` names what it lacks.  The first ten groups are the partition of
# LATE_SYMBOLS; the six after them ("Ratio shadow transfer", "Moving inserted objects", "Media inside glass",
# "Reflected in inserted objects", "Material edits in the photograph", "Relighting in the photograph") stand beside it
FEATURE_SYMBOLS = {
    "smooth inserted objects": ("matpbr_path_render_objects_normals", "matpbr_path_object_normal_host", "matpbr_path_object_sample_shading_host"),
    "the denoiser": ("matpbr_path_features", "matpbr_path_features_host", "matpbr_path_denoise_prepare", "matpbr_path_denoise_prepare_host",
                     "matpbr_path_denoise_level", "matpbr_path_denoise_level_host", "matpbr_path_denoise_workspace_bytes", "matpbr_path_denoise"),
    "PBR inserted objects": ("matpbr_path_render_objects_pbr", "matpbr_path_object_lookup_host"),
    "emissive inserted objects": ("matpbr_path_light_tables", "matpbr_path_render_objects_lights", "matpbr_path_light_sample_host",
                                  "matpbr_path_light_pdf_host"),
    "rough dielectric inserted objects": ("matpbr_path_render_objects_rough", "matpbr_path_rough_sample_host", "matpbr_path_rough_eval_host"),
    "vertex-coloured inserted objects": ("matpbr_path_render_objects_colors", "matpbr_path_object_color_host", "matpbr_path_feature_colors",
                                         "matpbr_path_feature_colors_host"),
    "textured inserted objects": ("matpbr_path_render_objects_textures", "matpbr_path_object_texture_host", "matpbr_path_feature_tints",
                                  "matpbr_path_feature_tints_host"),
    "the differential render": ("matpbr_path_render_objects_diff", "matpbr_path_composite", "matpbr_path_composite_host", "matpbr_path_trace_scene_host"),
    "the differential render's denoiser": ("matpbr_path_denoise_diff_prepare", "matpbr_path_denoise_diff_prepare_host", "matpbr_path_denoise_diff_level",
                                           "matpbr_path_denoise_diff_level_host", "matpbr_path_denoise_diff_finish",
                                           "matpbr_path_denoise_diff_finish_host", "matpbr_path_denoise_diff_workspace_bytes", "matpbr_path_denoise_diff",
                                           "matpbr_path_denoise_diff_host"),
    "the photograph seen through inserted glass": ("matpbr_path_render_objects_through", "matpbr_path_through_chain_host"),
    "ratio shadow transfer": ("matpbr_path_render_objects_ratio", "matpbr_path_composite_ratio", "matpbr_path_composite_ratio_host"),
    "moving inserted objects": ("matpbr_path_bvh_build_grafted", "matpbr_path_xform_check_host", "matpbr_path_objects_move",
                                "matpbr_path_objects_move_host"),
    "media inside glass objects": ("matpbr_path_render_objects_media", "matpbr_path_render_objects_diff_media", "matpbr_path_medium_segment_host",
                                   "matpbr_path_phase_sample_host"),
    "the photograph reflected in inserted objects": ("matpbr_path_render_objects_reflect", "matpbr_path_reflect_chain_host"),
    "material edits in the photograph": ("matpbr_path_render_edit_diff",),
    "relighting in the photograph": ("matpbr_path_render_relight", "matpbr_path_composite_relight", "matpbr_path_composite_relight_host"),
}
(SMOOTH_SYMBOLS, DENOISE_SYMBOLS, PBR_SYMBOLS, LIGHT_SYMBOLS, ROUGH_SYMBOLS, COLOR_SYMBOLS, TEXTURE_SYMBOLS, DIFF_SYMBOLS, DIFF_DENOISE_SYMBOLS,
 THROUGH_SYMBOLS, RATIO_SYMBOLS, MOVE_SYMBOLS, MEDIUM_SYMBOLS, REFLECT_SYMBOLS, MAPEDIT_SYMBOLS, RELIGHT_SYMBOLS) = FEATURE_SYMBOLS.values()
_FEATURE_OF = {name: what for what, names in FEATURE_SYMBOLS.items() for name in names}   # every late symbol -> its feature
_FEATURE = {name: what for name, what in _FEATURE_OF.items() if what in list(FEATURE_SYMBOLS)[:10]}
LATE_SYMBOLS = tuple(_FEATURE)
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
            if name in _FEATURE_OF and not hasattr(lib, name):
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
        what = _FEATURE_OF.get(name, "smooth inserted objects")
        raise PathError(f"libmatpbr_path.so has no {name}: it was built before {what}; rebuild it (build.build_path_library)")
    return getattr(lib, name)


def check(code: int, what: str) -> None:
    if code != 0:
        msg = load().matpbr_path_strerror(code)
        raise PathError(f"{what} failed: {msg.decode() if msg else code} ({code})")


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


def _ref(struct):
    """A ctypes structure or scalar, by reference, as the void pointer the C ABI takes."""
    return ctypes.cast(ctypes.byref(struct), _P)


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
    flags to hide (the colour guide takes the colour flag and not the texture flag).  OBJECT_MEDIUM is always hidden: a medium changes
    no geometry and no first-hit guide, and only the two entries that render it take its flag.  So is OBJECT_PHOTO, which only
    matpbr_path_render_objects_reflect takes."""
    flags |= OBJECT_MEDIUM | OBJECT_PHOTO
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


def _aligned_texels(texels) -> np.ndarray:
    """`texels` as float32 [n,4] in memory whose address is a multiple of 16, as the library's float4 loads need it."""
    a = np.asarray(texels, dtype=np.float32).reshape(-1, 4)
    buf = np.empty(a.size + 4, np.float32)
    off = (-buf.ctypes.data % 16) // 4
    out = buf[off:off + a.size].reshape(-1, 4)
    out[...] = a
    return out


def _unflagged(table):
    """`table` as every entry but matpbr_path_render_objects_reflect takes it: the same table where no object carries OBJECT_PHOTO, else
    a copy without it (every other flag stays)."""
    if table is None or not any(t.kind & OBJECT_PHOTO for t in table):
        return table
    return [PathObject(t.kind & ~OBJECT_PHOTO, t.first_tri, t.n_tri, t.p) for t in table]
