"""The photograph reflected in inserted objects on the CPU ("Reflected in inserted objects"; no GPU): the camera
chain of `matpbr_path_reflect_chain_host`, built from the routines the kernel runs, against the fp64 chain of `path_reflect_fp64`; the
twin against `matpbr_path_through_chain_host` on a table without the flag; the refusals of the library, of an object list, of
`render_oi(reflect_photo=True)` and of the command line before any GPU work; the header against the binding."""
import ctypes
import json
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
import path_oi_fp64 as po  # noqa: E402
import path_reflect_fp64 as rf  # noqa: E402
import path_testlib as tl  # noqa: E402
import path_through_fp64 as tf  # noqa: E402

FOV = pf.FOV
THR_BOUND = 1.7e-4   # 4 x 4.14e-5, the worst thr_k error of the host twin against fp64 on scene R (the docstring of test 1)
_report = tl.reporter("path reflect host", "test_path_reflect_host")


@pytest.fixture(scope="module")
def path_lib():
    return tl.load()


def _host_scene(path_lib, objects):
    """The groove at 24 x 20 with `objects`: the fp64 side (V, T, table, maps) and the library's (host BVH, table, corner normals, records)."""
    from materialist_amd import mesh

    H, W = 20, 24
    rm = mesh.reference_mesh(pf.groove_scene(H, W), FOV)
    V, T, table = rf.merged(rm["vertices"], rm["triangles"], objects)
    Vm, Tm, lib_table, corner, records = path_lib.merge_objects(rm["vertices"], rm["triangles"], objects, normals=True, pbr=True)
    n_scene = rm["triangles"].shape[0]
    rng = np.random.default_rng(11)
    a, r, m = pf.groove_maps(H, W, rng)
    env = pf.groove_env(rng)
    return {"H": H, "W": W, "V": V, "T": T, "table": table, "n_scene": n_scene, "rm": rm, "a": a, "r": r, "m": m, "env": env,
            "tab": path_lib.env_tables(env), "photo": rf.photograph(H, W), "bvh": path_lib.build_bvh(Vm, Tm, n_scene), "lib_table": lib_table,
            "corner": corner, "records": records}


@pytest.fixture(scope="module")
def scene(path_lib):
    return _host_scene(path_lib, rf.scene_objects())


def _chain_host(path_lib, s, max_depth, seed, sample=0, which="reflect"):
    n = s["H"] * s["W"]
    own = {"records": s["records"]} if which == "reflect" else {}
    return getattr(path_lib, which + "_chain_host")(s["bvh"], s["lib_table"], s["n_scene"], s["H"], s["W"], np.arange(n), seed, sample, max_depth,
                                                    obj_nrm=s["corner"], fov_x_deg=FOV, **own)


# ---- 1, 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_depth", [3, 6, 16])
def test_the_chain_matches_fp64(path_lib, scene, oracle64, max_depth):
    """Every pixel of R, sample 0, seeds 0-2: landing depth and texel equal on at least 0.99 of the lanes, `test_path_through_host.py`'s
    bound (measured: every lane); on the agreeing see-through lanes the landing ray within 1e-5, that file's tolerance (measured worst
    3.5e-6), and thr_k within 1.7e-4 relative to the channel.  That file's 1e-6 holds along dielectric chains; a chain through the chrome
    sphere (GGX of roughness 0.1: the weight is f / pdf about a peak of width 1e-4) measured a worst error of the host twin against fp64
    of 4.14e-5 over these nine cases (1.1e-5, 1.0e-5 and 4.1e-5 by seed), and the bound is 4 x that, the project's max(4 e, floor) rule."""
    s = scene
    rf.preconditions(s, oracle64, s["tab"])
    assert [t.kind & path_lib.OBJECT_PHOTO != 0 for t in s["lib_table"]] == [True, True, True, False, False, False]
    for seed in (0, 1, 2):
        ref = rf.chains(oracle64, s, max_depth, seed)
        got = _chain_host(path_lib, s, max_depth, seed)
        agree = (got["depth"] == ref["k"]) & ((ref["k"] < 0) | (got["texel"] == ref["q"]))
        see = agree & (ref["k"] >= 0)
        thr_err = (np.abs(got["thr"][see] - ref["thr"][see]) / np.abs(ref["thr"][see])).max()
        ray_err = max(np.abs(got["o"][see] - ref["o"][see]).max(), np.abs(got["d"][see] - ref["d"][see]).max())
        _report(f"max_depth {max_depth} seed {seed}: see-through lanes in fp64; of them through a flagged vertex; lanes whose depth and texel agree "
                f"(bound 0.99); worst thr_k error (bound {THR_BOUND:g}); worst landing-ray error (bound 1e-5)",
                f"{int((ref['k'] >= 0).sum())}; {int((ref['flagged'] & (ref['k'] >= 0)).sum())}; {agree.mean():.4f}; {thr_err:.3e}; {ray_err:.3e}")
        assert agree.mean() >= 0.99, (max_depth, seed, np.nonzero(~agree)[0][:10])
        assert see.sum() >= 60 and thr_err <= THR_BOUND and ray_err <= 1e-5
        plain = see & ~ref["flagged"]                                               # chains of glass alone keep that file's bound
        assert plain.sum() >= 5 and np.abs(got["thr"][plain] / ref["thr"][plain] - 1.0).max() <= 1e-6
        assert (got["thr"][see & ref["flagged"]] != got["thr"][see & ref["flagged"], :1]).any()   # chrome has a colour
        off = got["depth"] < 0
        assert (got["texel"][off] == -1).all() and not got["thr"][off].any() and not got["o"][off].any() and not got["d"][off].any()
        assert ((got["depth"] >= 1) | off).all() and (got["depth"] < max_depth).all()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_table_without_the_flag_gives_the_through_chain_bit_for_bit(path_lib, oracle64):
    """`path_through_fp64`'s scene S and scene R without its flags: every output of the new twin has `through_chain_host`'s bits; on R the
    flags do change the chain."""
    for objects in (tf.scene_objects(), rf.scene_objects(photo=False)):
        s = _host_scene(path_lib, objects)
        assert not any(t.kind & path_lib.OBJECT_PHOTO for t in s["lib_table"])
        for max_depth, seed in ((3, 0), (16, 1)):
            new, old = _chain_host(path_lib, s, max_depth, seed), _chain_host(path_lib, s, max_depth, seed, which="through")
            assert (old["depth"] >= 0).sum() >= 10                                  # R without flags: the far glass cube alone
            for key in ("depth", "texel", "thr", "o", "d"):
                assert np.array_equal(new[key].view(np.uint32), old[key].view(np.uint32)), (key, max_depth, seed)
    flagged = _host_scene(path_lib, rf.scene_objects())
    assert (_chain_host(path_lib, flagged, 16, 1)["depth"] >= 0).sum() > (old["depth"] >= 0).sum() + 20


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
def _chain_args(path_lib, s, table, N=4):
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    pix, sd, smp = np.arange(N, dtype=np.int32), np.zeros(N, np.uint32), np.zeros(N, np.int32)
    depth, texel = np.empty(N, np.int32), np.empty(N, np.int32)
    thr, o, d = (np.empty((N, 3), np.float32) for _ in range(3))
    keep = (pix, sd, smp, depth, texel, thr, o, d, (path_lib.PathObject * len(table))(*table), (path_lib.PathObjectPbr * len(table))(*s["records"]))
    args = [p(s["bvh"]["nodes"]), p(s["bvh"]["tris"]), s["H"], s["W"], FOV, 6, ctypes.cast(keep[8], ctypes.c_void_p), len(table), p(s["corner"]),
            s["n_scene"], ctypes.cast(keep[9], ctypes.c_void_p), p(pix), p(sd), p(smp), N, p(depth), p(texel), p(thr), p(o), p(d)]
    return keep, args


def _with_kind(path_lib, table, k, kind):
    return [path_lib.PathObject(kind if j == k else t.kind, t.first_tri, t.n_tri, t.p) for j, t in enumerate(table)]


def test_the_library_refuses_the_flag_where_it_does_not_belong(path_lib):
    """R_light's table through `matpbr_path_reflect_chain_host` and, with NULL buffers after a valid table, through
    `matpbr_path_render_objects_reflect` (the table is checked on the host before any launch): the flag on kind 1 or 4 is refused, and
    so is a flagged coloured object and a flagged kind 3 without its record in the twin; the entries from before the flag keep
    refusing it; the render refuses NULL `photo` / `through`."""
    s = _host_scene(path_lib, rf.scene_objects(light=True))
    table = s["lib_table"]
    kinds = [t.kind & 0xff for t in table]
    assert kinds == [path_lib.BSDF_PBR, path_lib.BSDF_ROUGH_DIELECTRIC, path_lib.BSDF_DIFFUSE, path_lib.BSDF_DIELECTRIC, path_lib.BSDF_DIELECTRIC,
                     path_lib.BSDF_PBR, path_lib.BSDF_AREA]
    fn = path_lib.symbol("matpbr_path_reflect_chain_host")
    keep, args = _chain_args(path_lib, s, table)
    assert fn(*args) == 0
    for k in (3, 6):                                                             # kind 1, kind 4
        bad = _with_kind(path_lib, table, k, table[k].kind | path_lib.OBJECT_PHOTO)
        keep_b, args_b = _chain_args(path_lib, s, bad)
        assert fn(*args_b) == -1, k
    keep_c, args_c = _chain_args(path_lib, s, _with_kind(path_lib, table, 2, table[2].kind | path_lib.OBJECT_COLORED))
    assert fn(*args_c) == -1
    assert fn(*(None if i == 10 else x for i, x in enumerate(args))) == -1       # the chrome sphere's record
    for j, bad in ((0, None), (1, None), (2, 0), (5, 17), (6, None), (7, 0), (9, -1), (11, None), (14, -1), (15, None), (19, None)):
        assert fn(*(bad if i == j else x for i, x in enumerate(args))) == -1, j
    old = path_lib.symbol("matpbr_path_through_chain_host")
    assert old(*args[:10], *args[11:]) == -1                                     # an unknown kind to the entry from before the flag
    keep_u, args_u = _chain_args(path_lib, s, path_lib._unflagged(table))
    assert old(*args_u[:10], *args_u[11:]) == 0
    with pytest.raises(path_lib.PathError):
        path_lib.through_chain_host(s["bvh"], table, s["n_scene"], s["H"], s["W"], [0], 0, 0, 6, obj_nrm=s["corner"])

    # the render entry: every check runs on the host before a launch, so a refusal needs no device
    render = path_lib.symbol("matpbr_path_render_objects_reflect")
    lights = path_lib.light_tables(s["V"], s["T"], table, s["records"])
    buf = np.zeros(16, np.float32)
    q = buf.ctypes.data_as(ctypes.c_void_p)                                      # stands for a buffer no refused call reads
    head = ctypes.cast(ctypes.byref(lights["header"]), ctypes.c_void_p)

    def call(tab, photo=q, through=q, fg=q):
        arr = (path_lib.PathObject * len(tab))(*tab)
        return render(q, q, q, q, q, s["H"], s["W"], FOV, q, q, q, q, 8, 16, 1, 4, 0, 1, None, None, ctypes.cast(arr, ctypes.c_void_p), len(tab),
                      s["corner"].ctypes.data_as(ctypes.c_void_p), s["n_scene"], ctypes.cast(keep[9], ctypes.c_void_p), head, q, q, None, None, None,
                      None, 0, fg, q, q, None, photo, through, None, None)

    for k in (3, 6):
        assert call(_with_kind(path_lib, table, k, table[k].kind | path_lib.OBJECT_PHOTO)) == -1, k
    assert call(table, photo=None) == -1 and call(table, through=None) == -1 and call(table, fg=None) == -1
    assert call(_with_kind(path_lib, table, 2, table[2].kind | 0x2000)) == -1    # a bit nobody knows
    for name in ("matpbr_path_render_objects_diff_media", "matpbr_path_render_objects_through", "matpbr_path_render_objects_ratio"):
        assert name in path_lib.SIGNATURES                                       # they take the table without the flag alone: `_unflagged`
    assert all(not (t.kind & path_lib.OBJECT_PHOTO) for t in path_lib._unflagged(table))
    assert all(not (t.kind & path_lib.OBJECT_PHOTO) for t in path_lib._uncolored(table, 0))
    assert [t.kind for t in path_lib._unflagged(table)] == [t.kind & ~path_lib.OBJECT_PHOTO for t in table]


def test_the_object_list_validates_photo(path_lib, tmp_path):
    """`load_oi_scene`: "photo" true on a dielectric or an area entry, a value that is no bool and another spelling each get a message
    that names the key; true and false on an eligible entry come back; `merge_objects` sets the flag and refuses the same."""
    from materialist_amd import mesh, relight

    ob = pd.cube_object(pd.VISIBLE_CUBE)
    mesh.write_ply(str(tmp_path / "cube.ply"), ob["vertices"].astype(np.float32), ob["triangles"])

    def load(entry):
        path = str(tmp_path / "list.json")
        with open(path, "w") as f:
            json.dump({"objects": [dict({"ply": "cube.ply"}, **entry)]}, f)
        return relight.load_oi_scene(path)

    for bsdf in (rf.CHROME, rf.FROSTED, po.DIFFUSE_08):
        assert load({"bsdf": bsdf, "photo": True})[0]["photo"] is True and load({"bsdf": bsdf, "photo": False})[0]["photo"] is False
        assert load({"bsdf": bsdf})[0]["photo"] is None
    assert load({"bsdf": po.GLASS, "photo": False})[0]["photo"] is False
    with pytest.raises(ValueError, match=r"objects\[0\]: bad photo: photo: .*'dielectric' object is see-through already"):
        load({"bsdf": po.GLASS, "photo": True})
    with pytest.raises(ValueError, match=r"objects\[0\]: bad photo: photo: .*'area' object has no BSDF"):
        load({"bsdf": {"type": "area", "radiance": 2.0}, "photo": True})
    for bad in (1, "yes", None, [True]):
        with pytest.raises(ValueError, match=r"objects\[0\]: bad photo: photo must be true or false"):
            load({"bsdf": rf.CHROME, "photo": bad})
    with pytest.raises(ValueError, match=r"unknown key 'Photo' \(known: .*'photo'\)"):
        load({"bsdf": rf.CHROME, "Photo": True})
    rm_v, rm_t = np.array([[-1, -1, -3], [1, -1, -3], [0, 1, -3]], np.float64), np.array([[0, 1, 2]], np.int32)
    table = path_lib.merge_objects(rm_v, rm_t, [dict(ob, bsdf=rf.CHROME, photo=True), dict(ob, photo=False), ob])[2]
    assert [t.kind for t in table] == [path_lib.BSDF_PBR | path_lib.OBJECT_PHOTO, path_lib.BSDF_DIFFUSE, path_lib.BSDF_DIFFUSE]
    with pytest.raises(ValueError, match="object 0: photo: .*'dielectric'"):
        path_lib.merge_objects(rm_v, rm_t, [dict(ob, bsdf=po.GLASS, photo=True)])
    with pytest.raises(ValueError, match="object 0: photo must be true or false"):
        path_lib.merge_objects(rm_v, rm_t, [dict(ob, photo=1)])


def test_the_command_line_and_render_oi_refuse_before_any_gpu_work(monkeypatch):
    sys.path.insert(0, ROOT)
    import render_final
    from materialist_amd import pathtrace, relight

    base = ["--save_name", "case", "--mode", "oi"]
    a = render_final.parse_args(base + ["--oi_composite", "--oi_reflect_photo"])
    assert a.oi_reflect_photo and a.oi_composite
    assert not render_final.parse_args(base + ["--oi_composite"]).oi_reflect_photo
    with pytest.raises(SystemExit) as e:
        render_final.parse_args(base + ["--oi_reflect_photo"])
    assert e.value.code == 2

    def no_library(*_a, **_k):
        raise AssertionError("the refusal comes before any library call")

    monkeypatch.setattr(pathtrace, "load", no_library)
    monkeypatch.setattr(pathtrace, "symbol", no_library)
    with pytest.raises(ValueError, match="reflect_photo needs composite"):
        relight.render_oi("no_such_scene", reflect_photo=True)
    with pytest.raises(ValueError, match="reflect_photo needs composite"):
        relight.render_oi("no_such_scene", reflect_photo=True, see_through=True, composite_denoise=True)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_what_the_binding_binds(path_lib):
    with open(os.path.join(ROOT, "include", "matpbr_path.h")) as f:
        raw = f.read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(matpbr_path_\w+)\s*\(", text))
    names = ("matpbr_path_render_objects_reflect", "matpbr_path_reflect_chain_host")
    assert tuple(path_lib.REFLECT_SYMBOLS) == names and set(names) <= declared and not set(names) & set(path_lib.LATE_SYMBOLS)
    assert re.search(r"#define MATPBR_PATH_OBJECT_PHOTO 0x1000\b", raw) and path_lib.OBJECT_PHOTO == 0x1000
    assert re.search(r"#define MATPBR_PATH_VERSION 3\b", raw)
    lib = path_lib.load()
    for name in names:
        assert hasattr(lib, name), name
        fn = path_lib.symbol(name, lib)
        assert fn.argtypes == path_lib.SIGNATURES[name][1] and fn.restype == path_lib.SIGNATURES[name][0], name
    P = ctypes.c_void_p
    assert path_lib.SIGNATURES[names[0]][1] == path_lib.SIGNATURES["matpbr_path_render_objects_diff_media"][1]
    old = path_lib.SIGNATURES["matpbr_path_through_chain_host"][1]
    assert path_lib.SIGNATURES[names[1]][1] == old[:10] + [P] + old[10:]
    assert lib.matpbr_path_version() == path_lib.VERSION == 3

    class Old:
        pass

    for name in names:
        with pytest.raises(path_lib.PathError, match=name + ".*reflected in inserted objects"):
            path_lib.symbol(name, Old())
