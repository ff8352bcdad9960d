"""The refusals of libmatpbr_path.so's entry points that take the common arguments of a frame (include/matpbr_path.h): the eight forward
renders, the two backward passes and `matpbr_path_features`, each with every term of the validity condition broken in turn, and the
five object entries with every rule of their level ("The object entries").  Every case is invalid in exactly
one respect and returns MATPBR_PATH_ERR_INVALID_ARG; every other pointer is a non-null dummy, which a refusing call never reads.
Validation precedes every launch, so no GPU is needed."""
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
FORWARD = {"matpbr_path_render": (), "matpbr_path_render_objects": OBJECTS[:2], "matpbr_path_render_objects_normals": OBJECTS,
           "matpbr_path_render_objects_pbr": OBJECTS + ("pbr",), "matpbr_path_render_objects_lights": OBJECTS + LIGHTS,
           "matpbr_path_render_objects_rough": OBJECTS + LIGHTS, "matpbr_path_render_trans": ("mask", "bg", "edit"),
           "matpbr_path_render_normals": ("nrm",)}
# the object entries: their level, which is also the highest kind they admit (levels 1 and 2: kind 2)
LEVEL = {"matpbr_path_render_objects": 1, "matpbr_path_render_objects_normals": 2, "matpbr_path_render_objects_pbr": 3,
         "matpbr_path_render_objects_lights": 4, "matpbr_path_render_objects_rough": 5}
BACKWARD = {"matpbr_path_render_bwd": (), "matpbr_path_render_bwd_normals": ("nrm", "d_n")}
FEATURES = "matpbr_path_features"
ORDER = {name: COMMON + ("out", "rays", "stream") + tail for name, tail in FORWARD.items()}
ORDER.update({name: COMMON + ("d_out", "d_a", "d_r", "d_m", "d_env", "workspace", "workspace_bytes", "rays", "stream") + tail
              for name, tail in BACKWARD.items()})
ORDER[FEATURES] = ("nodes", "tris", "H", "W", "fov") + OBJECTS + ("nrm_map", "geom", "stream")
WITH_TABLE = ("matpbr_path_render_objects_normals", "matpbr_path_render_objects_pbr", "matpbr_path_render_objects_lights",
              "matpbr_path_render_objects_rough", FEATURES)
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
    """A valid table of N_TRI-triangle objects of `kinds`, one after the other from triangle 1, its records and its light header (the
    kind-4 objects in order, records contiguous from 0, area 1) -> [table, records, header]."""
    p = {path_lib.BSDF_DIELECTRIC: (1.5, 1.0, 0.0), path_lib.BSDF_DIFFUSE: (0.5, 0.5, 0.5), path_lib.BSDF_PBR: (0.0, 0.0, 0.0),
         path_lib.BSDF_AREA: (0.5, 0.5, 0.5), path_lib.BSDF_ROUGH_DIELECTRIC: (1.5, 1.0, 0.1)}
    table = (path_lib.PathObject * len(kinds))(*(path_lib.PathObject(kind, 1 + N_TRI * k, N_TRI,
                                                                     (ctypes.c_float * 3)(*p[kind & ~path_lib.OBJECT_SMOOTH]))
                                                 for k, kind in enumerate(kinds)))
    records = (path_lib.PathObjectPbr * len(kinds))(*(path_lib.PathObjectPbr((ctypes.c_float * 3)(0.5, 0.5, 0.5), 0.5, 0.0) for _ in kinds))
    header = path_lib.PathLights()
    for k, kind in enumerate(kinds):
        if kind & ~path_lib.OBJECT_SMOOTH == path_lib.BSDF_AREA:
            l = header.n_lights
            header.object[l], header.first[l], header.n_tri[l], header.area[l] = k, N_TRI * l, N_TRI, 1.0
            header.n_lights += 1
    return [table, records, header]


def _scene_args(c, scene):
    """The arguments of `scene` among those the entry of `c` takes."""
    table, records, header = scene
    c["keep"].append(scene)
    args = {"objects": ctypes.cast(table, ctypes.c_void_p), "n_objects": len(table), "pbr": ctypes.cast(records, ctypes.c_void_p),
            "lights": ctypes.cast(ctypes.byref(header), ctypes.c_void_p)}
    return {k: v for k, v in args.items() if k in c}


def _own_kind(path_lib, entry):
    """The kind of the one object of the entry's valid call: the highest it admits."""
    return max(LEVEL.get(entry, 2), path_lib.BSDF_DIFFUSE)


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
    """spoil: table / records / header [index] . field = value (a header's field is an array over the lights; index None: a scalar)."""
    def spoil(table, records, header):
        target = {"table": table, "records": records}.get(what)
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


def _cases():
    out = []
    for entry, names in ORDER.items():
        cases = {f"{k} = NULL": {k: None} for k in names
                 if k in ("nodes", "tris", "a", "r", "m", "env", "row_cdf", "col_cdf", "env_pdf", "out", "d_out", "workspace", "geom")}
        cases.update({k: v for k, v in {**SIZES, **DEPTHS}.items() if next(iter(v)) in names})
        cases.update(FOVS)
        if entry in BACKWARD:
            cases.update(BACKWARD_CASES)
        if entry == "matpbr_path_render_bwd_normals":
            cases["d_n without nrm"] = {"nrm": None, "d_n": DUMMY.ctypes.data}
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
            if level == 5:
                cases.update(ROUGH_CASES)
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
    assert len(ORDER) == 11
