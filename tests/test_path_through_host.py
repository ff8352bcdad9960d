"""The photograph seen through inserted glass on the CPU ("Seen through glass"; no GPU): the camera chain of
`matpbr_path_through_chain_host`, built from the routines the kernel runs, against the fp64 chain of `path_through_fp64`; the header
against the binding; the refusals of `render_oi(see_through=True)` and of the command line before any GPU work."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import path_diff_fp64 as pd  # noqa: E402
import path_fp64 as pf  # noqa: E402
import path_objects_fp64 as pob  # noqa: E402
import path_testlib as tl  # noqa: E402
import path_through_fp64 as tf  # noqa: E402

FOV = pf.FOV
_report = tl.reporter("path through host", "test_path_through_host")


@pytest.fixture(scope="module")
def path_lib():
    return tl.load()


def _host_scene(path_lib, objects):
    """The groove at 24 x 20 with `objects`: the fp64 side (V, T, table) and the library's (host BVH, table, corner normals)."""
    from materialist_amd import mesh

    H, W = 20, 24
    rm = mesh.reference_mesh(pf.groove_scene(H, W), FOV)
    V, T, table = pob.merged(rm["vertices"], rm["triangles"], objects)
    Vm, Tm, lib_table, corner = path_lib.merge_objects(rm["vertices"], rm["triangles"], objects, normals=True)
    n_scene = rm["triangles"].shape[0]
    return {"H": H, "W": W, "V": V, "T": T, "table": table, "n_scene": n_scene, "bvh": path_lib.build_bvh(Vm, Tm, n_scene),
            "lib_table": lib_table, "corner": corner}


@pytest.fixture(scope="module")
def scene(path_lib):
    return _host_scene(path_lib, tf.scene_objects())


def _chain_host(path_lib, s, max_depth, seed, sample=0):
    n = s["H"] * s["W"]
    return path_lib.through_chain_host(s["bvh"], s["lib_table"], s["n_scene"], s["H"], s["W"], np.arange(n), seed, sample, max_depth,
                                       obj_nrm=s["corner"], fov_x_deg=FOV)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_depth", [3, 6, 16])
def test_the_chain_matches_fp64(path_lib, scene, oracle64, max_depth):
    """Every pixel of S, sample 0, seeds 0-2: landing depth and texel equal on at least 0.99 of the lanes (the rest are edge ties under
    the tree: `test_path_diff_host.py` grants 0.999 to one trace, and a chain is up to a few traces); on the agreeing see-through lanes
    thr_k within 1e-6 relative and the landing ray within 1e-5."""
    s = scene
    tf.preconditions(s, oracle64)
    for seed in (0, 1, 2):
        ref = tf.chains(oracle64, s, max_depth, seed)
        got = _chain_host(path_lib, s, max_depth, seed)
        agree = (got["depth"] == ref["k"]) & ((ref["k"] < 0) | (got["texel"] == ref["q"]))
        see = agree & (ref["k"] >= 0)
        thr_err = np.abs(got["thr"][see] / ref["thr"][see, None] - 1.0).max()
        ray_err = max(np.abs(got["o"][see] - ref["o"][see]).max(), np.abs(got["d"][see] - ref["d"][see]).max())
        _report(f"max_depth {max_depth} seed {seed}: see-through lanes in fp64; lanes whose depth and texel agree (bound 0.99); worst thr_k error "
                f"(bound 1e-6); worst landing-ray error (bound 1e-5)",
                f"{int((ref['k'] >= 0).sum())}; {agree.mean():.4f}; {thr_err:.3e}; {ray_err:.3e}")
        assert agree.mean() >= 0.99, (max_depth, seed, np.nonzero(~agree)[0][:10])
        assert see.sum() >= 90 and thr_err <= 1e-6 and ray_err <= 1e-5
        assert (got["thr"][see] == got["thr"][see, :1]).all()                       # a dielectric's weight has no colour
        off = got["depth"] < 0
        assert (got["texel"][off] == -1).all() and not got["thr"][off].any() and not got["o"][off].any() and not got["d"][off].any()
        assert ((got["depth"] >= 1) | off).all() and (got["depth"] < max_depth).all()


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_uncovered_lanes_and_a_table_without_glass_return_minus_one(path_lib, scene, oracle64):
    s = scene
    for seed in (0, 1, 2):
        got = _chain_host(path_lib, s, 16, seed)
        ref = tf.chains(oracle64, s, 16, seed)
        # c_s of the library's own camera trace: exact; of the fp64 camera ray: up to silhouette ties
        o, d = pd.camera_rays(s["H"], s["W"], seed)
        own = path_lib.trace_host(s["bvh"], o.astype(np.float32), d.astype(np.float32))[1] >= s["n_scene"]
        assert 0.4 < ref["covered"].mean() < 0.5
        assert (got["depth"][~ref["covered"] & ~own] == -1).all() and (~ref["covered"] & ~own).mean() > 0.5
    plain = _host_scene(path_lib, [pd.cube_object(pd.VISIBLE_CUBE)])
    o, d = pd.camera_rays(plain["H"], plain["W"], 0)
    assert (pf.brute(plain["V"][plain["T"]], o, d)[1] >= plain["n_scene"]).mean() > 0.02   # the cube is seen
    for max_depth in (2, 16):
        got = _chain_host(path_lib, plain, max_depth, 0)
        assert (got["depth"] == -1).all() and (got["texel"] == -1).all()
    # max_depth 1 traces the camera ray alone: no landing
    assert (_chain_host(path_lib, s, 1, 0)["depth"] == -1).all()


def test_refusals(path_lib, scene):
    s = scene
    fn = path_lib.symbol("matpbr_path_through_chain_host")
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    N = 4
    pix, sd, smp = np.arange(N, dtype=np.int32), np.zeros(N, np.uint32), np.zeros(N, np.int32)
    depth, texel = np.empty(N, np.int32), np.empty(N, np.int32)
    thr, o, d = (np.empty((N, 3), np.float32) for _ in range(3))
    tab = ctypes.cast((path_lib.PathObject * len(s["lib_table"]))(*s["lib_table"]), ctypes.c_void_p)
    args = [p(s["bvh"]["nodes"]), p(s["bvh"]["tris"]), s["H"], s["W"], FOV, 6, tab, len(s["lib_table"]), p(s["corner"]), s["n_scene"], p(pix), p(sd),
            p(smp), N, p(depth), p(texel), p(thr), p(o), p(d)]
    assert fn(*args) == 0
    for j, bad in ((0, None), (1, None), (2, 0), (3, 0), (4, 0.0), (4, 180.0), (5, 0), (5, 17), (6, None), (7, 0), (8, None), (9, -1), (10, None), (11, None),
                   (12, None), (13, -1), (14, None), (15, None), (16, None), (17, None), (18, None)):
        assert fn(*(bad if i == j else x for i, x in enumerate(args))) == -1, j
    outside = np.array([0, 1, 2, s["H"] * s["W"]], np.int32)
    assert fn(*(p(outside) if i == 10 else x for i, x in enumerate(args))) == -1
    with pytest.raises(path_lib.PathError):
        path_lib.through_chain_host(s["bvh"], s["lib_table"], s["n_scene"], s["H"], s["W"], [0], 0, -1, 6, obj_nrm=s["corner"])


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_command_line_and_render_oi_refuse_before_any_gpu_work(monkeypatch):
    sys.path.insert(0, ROOT)
    import render_final
    from materialist_amd import pathtrace, relight

    base = ["--save_name", "case", "--mode", "oi"]
    a = render_final.parse_args(base + ["--oi_composite", "--oi_see_through"])
    assert a.oi_see_through and a.oi_composite
    assert not render_final.parse_args(base + ["--oi_composite"]).oi_see_through
    with pytest.raises(SystemExit) as e:
        render_final.parse_args(base + ["--oi_see_through"])
    assert e.value.code == 2

    def no_library(*_a, **_k):
        raise AssertionError("the refusal comes before any library call")

    monkeypatch.setattr(pathtrace, "load", no_library)
    monkeypatch.setattr(pathtrace, "symbol", no_library)
    with pytest.raises(ValueError, match="see_through needs composite"):
        relight.render_oi("no_such_scene", see_through=True)
    with pytest.raises(ValueError, match="see_through needs composite"):
        relight.render_oi("no_such_scene", see_through=True, composite_denoise=True)


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_what_the_binding_binds(path_lib):
    with open(os.path.join(ROOT, "include", "matpbr_path.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(matpbr_path_\w+)\s*\(", text))
    names = ("matpbr_path_render_objects_through", "matpbr_path_through_chain_host")
    assert tuple(path_lib.THROUGH_SYMBOLS) == names and set(names) <= declared and set(names) <= set(path_lib.LATE_SYMBOLS)
    lib = path_lib.load()
    for name in names:
        assert hasattr(lib, name), name
        fn = path_lib.symbol(name, lib)
        assert fn.argtypes == path_lib.SIGNATURES[name][1] and fn.restype == path_lib.SIGNATURES[name][0], name
    P = ctypes.c_void_p
    assert path_lib.SIGNATURES[names[0]][1] == path_lib.SIGNATURES["matpbr_path_render_objects_diff"][1] + [P, P]
    assert path_lib.OBJECT_ENTRIES[names[0]] == path_lib.OBJECT_ENTRIES["matpbr_path_render_objects_textures"] == 13
    assert lib.matpbr_path_version() == path_lib.VERSION == 3

    class Old:
        pass

    with pytest.raises(path_lib.PathError, match="matpbr_path_render_objects_through.*seen through inserted glass"):
        path_lib.symbol(names[0], Old())
