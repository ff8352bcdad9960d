"""The refusals of libmatpbr_path.so's entry points that take the common arguments of a frame (include/matpbr_path.h): the eleven forward
renders, the five differential renders of inserted objects, `matpbr_path_render_edit_diff`, the two backward passes and
`matpbr_path_features`, each with every term of the validity condition broken in turn, and the thirteen object entries (forward levels
1 to 8 and the differential family at levels 7, 8 and 9) with every rule of their level ("The object
entries").  Every case is invalid in exactly one respect and returns MATPBR_PATH_ERR_INVALID_ARG; every other pointer is a non-null
dummy, which a refusing call never reads.  Validation precedes every launch, so no GPU is needed."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import path_testlib as tl  # noqa: E402

INVALID_ARG = -1   # MATPBR_PATH_ERR_INVALID_ARG
COMMON = ("nodes", "tris", "a", "r", "m", "H", "W", "fov", "env", "row_cdf", "col_cdf", "env_pdf", "He", "We", "spp", "max_depth", "seed",
          "spp_per_launch")
OBJECTS = ("objects", "n_objects", "obj_nrm", "n_scene_tri")
LIGHTS = ("pbr", "lights", "light_tris", "light_cdf")
TAIL = OBJECTS + LIGHTS + ("obj_col", "obj_uv", "tex", "texels", "n_texels")   # the thirteen object arguments of level 7
FORWARD = {"matpbr_path_render": (), "matpbr_path_render_objects": OBJECTS[:2], "matpbr_path_render_objects_normals": OBJECTS,
           "matpbr_path_render_objects_pbr": OBJECTS + ("pbr",), "matpbr_path_render_objects_lights": OBJECTS + LIGHTS,
           "matpbr_path_render_objects_rough": OBJECTS + LIGHTS, "matpbr_path_render_trans": ("mask", "bg", "edit"),
           "matpbr_path_render_normals": ("nrm",), "matpbr_path_render_objects_colors": TAIL[:9],
           "matpbr_path_render_objects_textures": TAIL, "matpbr_path_render_objects_media": TAIL + ("media",)}
# the differential family: what each entry takes after fg, delta, alpha, rewalked
DIFF = {"matpbr_path_render_objects_diff": (), "matpbr_path_render_objects_through": ("photo", "through"),
        "matpbr_path_render_objects_ratio": ("photo", "through", "base"),
        "matpbr_path_render_objects_diff_media": ("photo", "through", "base", "media"),
        "matpbr_path_render_objects_reflect": ("photo", "through", "base", "media")}
EDIT_DIFF = "matpbr_path_render_edit_diff"
# the object entries: their level; up to level 5 it is also the highest kind they admit (levels 1 and 2: kind 2)
LEVEL = {"matpbr_path_render_objects": 1, "matpbr_path_render_objects_normals": 2, "matpbr_path_render_objects_pbr": 3,
         "matpbr_path_render_objects_lights": 4, "matpbr_path_render_objects_rough": 5, "matpbr_path_render_objects_colors": 6,
         "matpbr_path_render_objects_textures": 7, "matpbr_path_render_objects_media": 8, "matpbr_path_render_objects_diff": 7,
         "matpbr_path_render_objects_through": 7, "matpbr_path_render_objects_ratio": 7, "matpbr_path_render_objects_diff_media": 8,
         "matpbr_path_render_objects_reflect": 9}
# the pointers an entry requires besides the frame's (every other pointer after the frame is nullable or consulted only where the table needs it)
REQUIRED = {"matpbr_path_render_objects_diff": ("fg", "delta", "alpha"),
            "matpbr_path_render_objects_through": ("fg", "delta", "alpha", "photo", "through"),
            "matpbr_path_render_objects_ratio": ("fg", "delta", "alpha", "base"), "matpbr_path_render_objects_diff_media": ("fg", "delta", "alpha"),
            "matpbr_path_render_objects_reflect": ("fg", "delta", "alpha", "photo", "through"),
            EDIT_DIFF: ("a_e", "r_e", "m_e", "mask", "delta", "base")}
BOTH_OR_NEITHER = ("matpbr_path_render_objects_ratio", "matpbr_path_render_objects_diff_media")   # photo and through
COLORED, TEXTURED, MEDIUM, PHOTO = 0x200, 0x400, 0x800, 0x1000   # MATPBR_PATH_OBJECT_*
DIFFUSE_KIND = 2                                                 # MATPBR_PATH_BSDF_DIFFUSE: it may carry every flag but the medium's
BACKWARD = {"matpbr_path_render_bwd": (), "matpbr_path_render_bwd_normals": ("nrm", "d_n")}
FEATURES = "matpbr_path_features"
ORDER = {name: COMMON + ("out", "rays", "stream") + tail for name, tail in FORWARD.items()}
ORDER.update({name: COMMON + ("d_out", "d_a", "d_r", "d_m", "d_env", "workspace", "workspace_bytes", "rays", "stream") + tail
              for name, tail in BACKWARD.items()})
ORDER.update({name: COMMON + ("rays", "stream") + TAIL + ("fg", "delta", "alpha", "rewalked") + tail for name, tail in DIFF.items()})
ORDER[EDIT_DIFF] = COMMON + ("rays", "stream", "a_e", "r_e", "m_e", "mask", "nrm", "delta", "base", "rewalked")
ORDER[FEATURES] = ("nodes", "tris", "H", "W", "fov") + OBJECTS + ("nrm_map", "geom", "stream")
WITH_TABLE = tuple(name for name, names in ORDER.items() if "n_scene_tri" in names)   # the entries that know n_scene_tri
_RAW = np.zeros(18, np.float64)
DUMMY = _RAW[(-_RAW.ctypes.data % 16) // 8:][:16]   # what every pointer of a call points at: 16-byte aligned, as light_tris must be
N_TRI = 20                                          # the triangles of every object of a table


@pytest.fixture(scope="module")
def path_lib():
    return tl.load()


def _workspace_bytes(path_lib, entry, c):
    size = path_lib.load().matpbr_path_render_bwd_workspace_bytes if entry == "matpbr_path_render_bwd" else \
        path_lib.load().matpbr_path_render_bwd_normals_workspace_bytes
    return int(size(c["H"], c["W"], c["He"], c["We"]))


def _scene(path_lib, kinds):
    """A valid table of N_TRI-triangle objects of `kinds`, one after the other from triangle 1, its records, its light header (the
    kind-4 objects in order, records contiguous from 0, area 1), its texture records (one 2 x 2 base-colour image at texel 0) and its
    medium records -> [table, records, header, tex, media]."""
    p = {path_lib.BSDF_DIELECTRIC: (1.5, 1.0, 0.0), path_lib.BSDF_DIFFUSE: (0.5, 0.5, 0.5), path_lib.BSDF_PBR: (0.0, 0.0, 0.0),
         path_lib.BSDF_AREA: (0.5, 0.5, 0.5), path_lib.BSDF_ROUGH_DIELECTRIC: (1.5, 1.0, 0.1)}
    table = (path_lib.PathObject * len(kinds))(*(path_lib.PathObject(kind, 1 + N_TRI * k, N_TRI,
                                                                     (ctypes.c_float * 3)(*p[kind & 0xFF]))
                                                 for k, kind in enumerate(kinds)))
    records = (path_lib.PathObjectPbr * len(kinds))(*(path_lib.PathObjectPbr((ctypes.c_float * 3)(0.5, 0.5, 0.5), 0.5, 0.0) for _ in kinds))
    header = path_lib.PathLights()
    for k, kind in enumerate(kinds):
        if kind & ~path_lib.OBJECT_SMOOTH == path_lib.BSDF_AREA:
            l = header.n_lights
            header.object[l], header.first[l], header.n_tri[l], header.area[l] = k, N_TRI * l, N_TRI, 1.0
            header.n_lights += 1
    tex = (path_lib.PathObjectTex * len(kinds))(*(path_lib.PathObjectTex(0, 2, 2, 0, 0, 0) for _ in kinds))
    media = (path_lib.PathObjectMedium * len(kinds))(*(path_lib.PathObjectMedium((ctypes.c_float * 3)(0.1, 0.2, 0.3), 0.5, 0.0) for _ in kinds))
    return [table, records, header, tex, media]


def _scene_args(c, scene):
    """The arguments of `scene` among those the entry of `c` takes."""
    table, records, header, tex, media = scene
    c["keep"].append(scene)
    args = {"objects": ctypes.cast(table, ctypes.c_void_p), "n_objects": len(table), "pbr": ctypes.cast(records, ctypes.c_void_p),
            "lights": ctypes.cast(ctypes.byref(header), ctypes.c_void_p), "tex": ctypes.cast(tex, ctypes.c_void_p),
            "media": ctypes.cast(media, ctypes.c_void_p)}
    return {k: v for k, v in args.items() if k in c}


def _own_kind(path_lib, entry):
    """The kind of the one object of the entry's valid call: the highest it admits."""
    return max(min(LEVEL.get(entry, 2), path_lib.BSDF_ROUGH_DIELECTRIC), path_lib.BSDF_DIFFUSE)


def _valid(path_lib, entry):
    """The arguments of a call of `entry` that the library accepts, by name; the objects they point at under "keep"."""
    ptr = DUMMY.ctypes.data
    assert ptr % 16 == 0
    c = {k: ptr for k in ORDER[entry]}
    c.update(H=4, W=6, fov=35.0, stream=None)
    if entry != FEATURES:
        c.update(He=2, We=4, spp=3, max_depth=4, seed=0, spp_per_launch=2, rays=None)
    c["keep"] = [path_lib.trans_edit()]
    if "objects" in c:
        c.update(_scene_args(c, _scene(path_lib, [_own_kind(path_lib, entry)])))
    if "n_scene_tri" in c:
        c.update(n_scene_tri=1)
    if "n_texels" in c:
        c.update(n_texels=4)   # the 2 x 2 image of `_scene`'s texture records
    if "edit" in c:
        c.update(edit=ctypes.cast(ctypes.byref(c["keep"][0]), ctypes.c_void_p))
    if entry == FEATURES:
        c.update(nrm_map=None)
    if entry in BACKWARD:   # no gradient asked for: a valid call returns before it launches anything
        c.update(d_a=None, d_r=None, d_m=None, d_env=None, workspace_bytes=_workspace_bytes(path_lib, entry, c))
        if "d_n" in c:
            c.update(d_n=None)
    return c


# ---- the cases: name -> the arguments it replaces (a callable takes the binding, the entry point and the valid arguments; a case that
# is itself a callable returns those arguments) ----------------------------------------------------------------------------------------
def _table_case(kinds=(), spoil=None, needs=None, **args):
    """The entry's valid object, then one of kind `needs` unless the valid object is of that kind, then objects of `kinds`; the table,
    its records and its header spoiled by `spoil(table, records, header)`; `args` replace further arguments."""
    def patch(path_lib, entry, c):
        own = _own_kind(path_lib, entry)
        scene = _scene(path_lib, [own] + [k for k in (needs,) if k not in (None, own)] + list(kinds))
        if spoil:
            spoil(*scene)
        return {**_scene_args(c, scene), **{k: v(path_lib, entry, c) if callable(v) else v for k, v in args.items()}}

    return patch


def _smooth(path_lib, entry, c):
    """The table of the valid call with the smooth flag on an object that may carry it."""
    own = _own_kind(path_lib, entry)
    kinds = [own, path_lib.BSDF_DIFFUSE | path_lib.OBJECT_SMOOTH] if own == path_lib.BSDF_AREA else [own | path_lib.OBJECT_SMOOTH]
    return _scene_args(c, _scene(path_lib, kinds))


def _set(what, index, field, value):
    """spoil: table / records / tex / media / header [index] . field = value (a header's field is an array over the lights; index None:
    a scalar)."""
    def spoil(table, records, header, tex, media):
        target = {"table": table, "records": records, "tex": tex, "media": media}.get(what)
        if target is not None:
            if isinstance(field, tuple):
                getattr(target[index], field[0])[field[1]] = value
            else:
                setattr(target[index], field, value)
        elif index is None:
            setattr(header, field, value)
        else:
            getattr(header, field)[index] = value

    return spoil


SIZES = {f"{k} = {v}": {k: v} for k in ("H", "W", "He", "We", "spp", "spp_per_launch") for v in (0, -1)}
DEPTHS = {f"max_depth = {v}": {"max_depth": v} for v in (0, 17)}
FOVS = {f"fov_x_deg = {v}": {"fov": v} for v in (0.0, 180.0, float("nan"))}
BACKWARD_CASES = {
    "a workspace one byte short": {"workspace_bytes": lambda p, e, c: c["workspace_bytes"] - 1},
    "a workspace address that is not a multiple of 8": {"workspace": lambda p, e, c: c["workspace"] + 4},
    "d_env with 1025 texels": {"He": 25, "We": 41, "d_env": DUMMY.ctypes.data,
                               "workspace_bytes": lambda p, e, c: _workspace_bytes(p, e, dict(c, He=25, We=41))},
}
TABLE_CASES = {
    "n_scene_tri = -1": {"n_scene_tri": -1},
    "a range starting below n_scene_tri": {"n_scene_tri": 2},
    "a smooth flag without obj_nrm": lambda p, e, c: {**_smooth(p, e, c), "obj_nrm": None},
}
# every object entry
OBJECT_CASES = {
    "overlapping ranges": _table_case([2], _set("table", 1, "first_tri", N_TRI)),
    "n_objects = 9": _table_case([2] * 8),
    "n_objects = 1 with objects = NULL": {"objects": None},
    "n_objects = -1": {"n_objects": -1},
}
# the entries that know records: the last object of the table is of kind 3
PBR_CASES = {
    "kind 3 without records": _table_case(needs=3, pbr=None),
    "kind 3 with a roughness below 0.07": _table_case(needs=3, spoil=_set("records", -1, "r", 0.05)),
}
# the entries that know lights: the last object of the table is the header's only light
_LIGHT = -1
LIGHT_CASES = {
    "kind 4 with the smooth flag": _table_case(needs=4 | 0x100),
    "kind 4 with lights = NULL": _table_case(needs=4, lights=None),
    "kind 4 with light_tris = NULL": _table_case(needs=4, light_tris=None),
    "kind 4 with light_cdf = NULL": _table_case(needs=4, light_cdf=None),
    "kind 4 with light_tris 4 bytes off its alignment": _table_case(needs=4, light_tris=lambda p, e, c: c["light_tris"] + 4),
    "a header with n_lights = 2": _table_case(needs=4, spoil=_set("header", None, "n_lights", 2)),
    "a header with another object[0]": _table_case(needs=4, spoil=_set("header", 0, "object", 7)),
    "a header with first[0] = 1": _table_case(needs=4, spoil=_set("header", 0, "first", 1)),
    "a header with n_tri[0] one short": _table_case(needs=4, spoil=_set("header", 0, "n_tri", N_TRI - 1)),
    "a light of area 0": _table_case(needs=4, spoil=_set("header", 0, "area", 0.0)),
    "a light of area NaN": _table_case(needs=4, spoil=_set("header", 0, "area", float("nan"))),
    "a negative radiance": _table_case(needs=4, spoil=_set("table", _LIGHT, ("p", 1), -0.5)),
    "an infinite radiance": _table_case(needs=4, spoil=_set("table", _LIGHT, ("p", 2), float("inf"))),
}
ROUGH_CASES = {
    "kind 5 with alpha 0.01": _table_case(spoil=_set("table", 0, ("p", 2), 0.01)),
    "kind 5 with alpha 1.5": _table_case(spoil=_set("table", 0, ("p", 2), 1.5)),
    "kind 5 with equal indices": _table_case(spoil=_set("table", 0, ("p", 1), 1.5)),
    "kind 5 with a zero index": _table_case(spoil=_set("table", 0, ("p", 0), 0.0)),
}
# a flag above an entry's level: the flag, on a kind that may carry it -> the first level that admits it
FLAG_CASES = {"the colour flag": (DIFFUSE_KIND | COLORED, 6), "the texture flag": (DIFFUSE_KIND | TEXTURED, 7), "the medium flag": (1 | MEDIUM, 8),
              "the photo flag": (DIFFUSE_KIND | PHOTO, 9)}
# each flag's own rules at the entries that admit it: the last object of the table carries the flag, beside valid arguments for it
COLOR_CASES = {"a coloured object without obj_col": _table_case([DIFFUSE_KIND | COLORED], obj_col=None)}
TEXTURE_CASES = {
    "a textured object without obj_uv": _table_case([DIFFUSE_KIND | TEXTURED], obj_uv=None),
    "a textured object without tex": _table_case([DIFFUSE_KIND | TEXTURED], tex=None),
    "a textured object without texels": _table_case([DIFFUSE_KIND | TEXTURED], texels=None),
    "a textured object with texels 4 bytes off their alignment": _table_case([DIFFUSE_KIND | TEXTURED], texels=lambda p, e, c: c["texels"] + 4),
}
MEDIUM_CASES = {
    "a medium flag with media = NULL": _table_case([1 | MEDIUM], media=None),
    "a medium with a negative sigma_s": _table_case([1 | MEDIUM], spoil=_set("media", -1, "sigma_s", -1.0)),
    "a medium with g = 1": _table_case([1 | MEDIUM], spoil=_set("media", -1, "g", 1.0)),
}


def _cases():
    out = []
    for entry, names in ORDER.items():
        cases = {f"{k} = NULL": {k: None} for k in names
                 if k in ("nodes", "tris", "a", "r", "m", "env", "row_cdf", "col_cdf", "env_pdf", "out", "d_out", "workspace", "geom") +
                 REQUIRED.get(entry, ())}
        cases.update({k: v for k, v in {**SIZES, **DEPTHS}.items() if next(iter(v)) in names})
        cases.update(FOVS)
        if entry in BACKWARD:
            cases.update(BACKWARD_CASES)
        if entry == "matpbr_path_render_bwd_normals":
            cases["d_n without nrm"] = {"nrm": None, "d_n": DUMMY.ctypes.data}
        if entry in BOTH_OR_NEITHER:
            cases.update({"photo without through": {"through": None}, "through without photo": {"photo": None}})
        if entry in DIFF:
            cases["n_objects = 0"] = {"n_objects": 0}
        if entry in WITH_TABLE:
            cases.update(TABLE_CASES)
        if entry in LEVEL:
            level = LEVEL[entry]
            cases.update(OBJECT_CASES)
            # a kind above the entry's level, beside valid records and light arguments
            cases.update({f"kind {k}": _table_case([k]) for k in (3, 4, 5) if k > level})
            if level == 1:
                cases["the smooth flag"] = _smooth
            if level >= 3:
                cases.update(PBR_CASES)
            if level >= 4:
                cases.update(LIGHT_CASES)
            if level >= 5:
                cases.update(ROUGH_CASES)
            cases.update({what: _table_case([kind]) for what, (kind, first) in FLAG_CASES.items() if level < first})
            if level >= 6:
                cases.update(COLOR_CASES)
            if level >= 7:
                cases.update(TEXTURE_CASES)
            if level >= 8:
                cases.update(MEDIUM_CASES)
        out += [pytest.param(entry, patch, id=f"{entry[len('matpbr_path_'):]}: {what}") for what, patch in cases.items()]
    return out


@pytest.mark.parametrize("entry, patch", _cases())
def test_an_argument_invalid_in_one_respect_is_refused(path_lib, entry, patch):
    c = _valid(path_lib, entry)
    args = dict(c)
    for k, v in (patch(path_lib, entry, c) if callable(patch) else patch).items():
        assert k in args, k
        args[k] = v(path_lib, entry, c) if callable(v) else v
    assert path_lib.symbol(entry)(*(args[k] for k in ORDER[entry])) == INVALID_ARG


@pytest.mark.parametrize("entry", sorted(BACKWARD))
def test_the_valid_backward_call_the_cases_start_from_is_accepted(path_lib, entry):
    """With no gradient asked for, a backward call whose arguments pass returns OK before it touches the device: the one entry point
    where the valid call that every case spoils can itself run without a GPU."""
    c = _valid(path_lib, entry)
    assert path_lib.symbol(entry)(*(c[k] for k in ORDER[entry])) == 0


def test_the_argument_orders_are_the_bindings(path_lib):
    for entry, names in ORDER.items():
        assert len(names) == len(path_lib.SIGNATURES[entry][1]), entry
    assert len(ORDER) == 20


# the argument lists of the thirteen object entries as path_abi.SIGNATURES spelled them one by one before it derived them from one object
# tail: P void pointer, i int, l long, f float, u uint32
_FRAME_TYPES = "PPPPPiifPPPPiiiiui"
_TAIL_TYPES = "PiPlPPPPPPPPl"
SPELLED = {"matpbr_path_render_objects": _FRAME_TYPES + "PPP" + "Pi", "matpbr_path_render_objects_normals": _FRAME_TYPES + "PPP" + "PiPl",
           "matpbr_path_render_objects_pbr": _FRAME_TYPES + "PPP" + "PiPlP", "matpbr_path_render_objects_lights": _FRAME_TYPES + "PPP" + "PiPlPPPP",
           "matpbr_path_render_objects_rough": _FRAME_TYPES + "PPP" + "PiPlPPPP", "matpbr_path_render_objects_colors": _FRAME_TYPES + "PPP" + "PiPlPPPPP",
           "matpbr_path_render_objects_textures": _FRAME_TYPES + "PPP" + _TAIL_TYPES, "matpbr_path_render_objects_media": _FRAME_TYPES + "PPP" + _TAIL_TYPES + "P",
           "matpbr_path_render_objects_diff": _FRAME_TYPES + "PP" + _TAIL_TYPES + "PPPP",
           "matpbr_path_render_objects_through": _FRAME_TYPES + "PP" + _TAIL_TYPES + "PPPPPP",
           "matpbr_path_render_objects_ratio": _FRAME_TYPES + "PP" + _TAIL_TYPES + "PPPPPPP",
           "matpbr_path_render_objects_diff_media": _FRAME_TYPES + "PP" + _TAIL_TYPES + "PPPPPPPP",
           "matpbr_path_render_objects_reflect": _FRAME_TYPES + "PP" + _TAIL_TYPES + "PPPPPPPP"}


def test_the_derived_signatures_are_the_lists_they_replace(path_lib):
    types = {"P": ctypes.c_void_p, "i": ctypes.c_int, "l": ctypes.c_long, "f": ctypes.c_float, "u": ctypes.c_uint32}
    assert set(SPELLED) == set(LEVEL) == set(path_lib.OBJECT_ENTRIES) | set(path_lib.DIFF_ENTRIES) | {path_lib.MEDIA_ENTRY}
    for entry, spelled in SPELLED.items():
        assert path_lib.SIGNATURES[entry] == (ctypes.c_int, [types[t] for t in spelled]), entry
    assert path_lib.DIFF_ENTRIES == {name: len(tail) for name, tail in DIFF.items()}
