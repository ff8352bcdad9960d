"""The refusals of libmatpbr_path.so's entry points that take the common arguments of a frame (include/matpbr_path.h): the six forward
renders, the two backward passes and `matpbr_path_features`, each with every term of the validity condition broken in turn.  Every
case is invalid in exactly one respect and returns MATPBR_PATH_ERR_INVALID_ARG; every other pointer is a non-null dummy, which a
refusing call never reads.  Validation precedes every launch, so no GPU is needed."""
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
FORWARD = {"matpbr_path_render": (), "matpbr_path_render_objects": OBJECTS[:2], "matpbr_path_render_objects_normals": OBJECTS,
           "matpbr_path_render_objects_pbr": OBJECTS + ("pbr",), "matpbr_path_render_trans": ("mask", "bg", "edit"),
           "matpbr_path_render_normals": ("nrm",)}
BACKWARD = {"matpbr_path_render_bwd": (), "matpbr_path_render_bwd_normals": ("nrm", "d_n")}
FEATURES = "matpbr_path_features"
ORDER = {name: COMMON + ("out", "rays", "stream") + tail for name, tail in FORWARD.items()}
ORDER.update({name: COMMON + ("d_out", "d_a", "d_r", "d_m", "d_env", "workspace", "workspace_bytes", "rays", "stream") + tail
              for name, tail in BACKWARD.items()})
ORDER[FEATURES] = ("nodes", "tris", "H", "W", "fov") + OBJECTS + ("nrm_map", "geom", "stream")
WITH_TABLE = ("matpbr_path_render_objects_normals", "matpbr_path_render_objects_pbr", FEATURES)
DUMMY = np.zeros(16, np.float64)   # what every pointer of a call points at


@pytest.fixture(scope="module")
def path_lib():
    return tl.load()


def _workspace_bytes(path_lib, entry, c):
    size = path_lib.load().matpbr_path_render_bwd_workspace_bytes if entry == "matpbr_path_render_bwd" else \
        path_lib.load().matpbr_path_render_bwd_normals_workspace_bytes
    return int(size(c["H"], c["W"], c["He"], c["We"]))


def _table(path_lib, kind):
    return (path_lib.PathObject * 1)(path_lib.PathObject(kind, 1, 20, (ctypes.c_float * 3)(0.5, 0.5, 0.5)))


def _valid(path_lib, entry):
    """The arguments of a call of `entry` that the library accepts, by name; the objects they point at under "keep"."""
    ptr = DUMMY.ctypes.data
    assert ptr % 8 == 0
    c = {k: ptr for k in ORDER[entry]}
    c.update(H=4, W=6, fov=35.0, stream=None)
    if entry != FEATURES:
        c.update(He=2, We=4, spp=3, max_depth=4, seed=0, spp_per_launch=2, rays=None)
    kind = path_lib.BSDF_PBR if entry == "matpbr_path_render_objects_pbr" else path_lib.BSDF_DIFFUSE
    keep = [_table(path_lib, kind), (path_lib.PathObjectPbr * 1)(path_lib.PathObjectPbr((ctypes.c_float * 3)(0.5, 0.5, 0.5), 0.5, 0.0)),
            path_lib.trans_edit()]
    if "objects" in c:
        c.update(objects=ctypes.cast(keep[0], ctypes.c_void_p), n_objects=1)
    if "n_scene_tri" in c:
        c.update(n_scene_tri=1)
    if "pbr" in c:
        c.update(pbr=ctypes.cast(keep[1], ctypes.c_void_p))
    if "edit" in c:
        c.update(edit=ctypes.cast(ctypes.byref(keep[2]), ctypes.c_void_p))
    if entry == FEATURES:
        c.update(nrm_map=None)
    if entry in BACKWARD:   # no gradient asked for: a valid call returns before it launches anything
        c.update(d_a=None, d_r=None, d_m=None, d_env=None, workspace_bytes=_workspace_bytes(path_lib, entry, c))
        if "d_n" in c:
            c.update(d_n=None)
    c["keep"] = keep
    return c


# ---- the cases: name -> the arguments it replaces (a callable takes the binding, the entry point and the valid arguments) -------------
def _smooth_table(path_lib, entry, c):
    c["keep"].append(_table(path_lib, c["keep"][0][0].kind | path_lib.OBJECT_SMOOTH))
    return ctypes.cast(c["keep"][-1], ctypes.c_void_p)


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
    "a smooth flag without obj_nrm": {"objects": _smooth_table, "obj_nrm": None},
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
        if entry == "matpbr_path_render_objects_pbr":
            cases["kind 3 without records"] = {"pbr": None}
        out += [pytest.param(entry, patch, id=f"{entry[len('matpbr_path_'):]}: {what}") for what, patch in cases.items()]
    return out


@pytest.mark.parametrize("entry, patch", _cases())
def test_an_argument_invalid_in_one_respect_is_refused(path_lib, entry, patch):
    c = _valid(path_lib, entry)
    args = dict(c)
    for k, v in patch.items():
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
    assert len(ORDER) == 9
