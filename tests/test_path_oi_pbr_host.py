"""Host side of PBR inserted objects ("PBR inserted objects"): the exported symbols, `object_bsdf` /
`merge_objects`, the table lookup the kernel runs (on the CPU), the argument checks of the C ABI, the fp64 restatement against the
depth mesh's own and over the library's fp32 traversal, the features and the albedo guide of a PBR object, and the object list file
of `render_final.py --mode oi --oi_scene`.  No GPU needed."""
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

import path_fp64 as pf  # noqa: E402
import path_objects_fp64 as pob  # noqa: E402
import path_oi_fp64 as po  # noqa: E402
import path_oi_pbr_fp64 as pp  # noqa: E402
import path_oi_smooth_fp64 as ps  # noqa: E402
import path_testlib as tl  # noqa: E402

FOV = pf.FOV


@pytest.fixture(scope="module")
def path_lib():
    return tl.load()


_report = tl.reporter("path oi pbr", "test_path_oi_pbr_host")


# ---- 1: the symbols ----------------------------------------------------------------------------------------------------------------------
def test_every_declared_symbol_is_exported_and_bound(path_lib):
    with open(os.path.join(ROOT, "include", "matpbr_path.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(matpbr_path_\w+)\s*\(", text))
    assert {"matpbr_path_render_objects_pbr", "matpbr_path_object_lookup_host", "matpbr_path_render_objects_normals"} <= declared
    lib = path_lib.load()
    for name in sorted(declared):
        assert name in path_lib.SIGNATURES, name
        fn = path_lib.symbol(name, lib)
        assert fn.argtypes == path_lib.SIGNATURES[name][1] and fn.restype == path_lib.SIGNATURES[name][0], name
    assert set(path_lib.SIGNATURES) == declared
    assert set(path_lib.PBR_SYMBOLS) == {"matpbr_path_render_objects_pbr", "matpbr_path_object_lookup_host"}
    assert set(path_lib.PBR_SYMBOLS) <= set(path_lib.LATE_SYMBOLS)
    assert lib.matpbr_path_version() == 3 == path_lib.VERSION
    assert "MATPBR_PATH_BSDF_PBR = 3" in text and path_lib.BSDF_PBR == 3
    # the record mirrors the header's struct: a[3], r, m, reserved[3]
    assert ctypes.sizeof(path_lib.PathObjectPbr) == 32 and path_lib.PathObjectPbr.r.offset == 12 and path_lib.PathObjectPbr.m.offset == 16
    assert ctypes.sizeof(path_lib.PathObject) == 24                     # frozen

    class Old:                                                          # a version-3 library built before the feature
        pass

    for name in path_lib.PBR_SYMBOLS:
        with pytest.raises(path_lib.PathError, match=name):
            path_lib.symbol(name, Old())


# ---- 2: object_bsdf and merge_objects ---------------------------------------------------------------------------------------------------
def test_object_bsdf_and_merge_objects(path_lib):
    assert path_lib.object_bsdf({"type": "pbr"}) == (3, (0.8, 0.8, 0.8, 0.5, 0.0))
    assert path_lib.object_bsdf({"type": "pbr", "albedo": 0.25, "roughness": 1.0, "metallic": 1}) == (3, (0.25, 0.25, 0.25, 1.0, 1.0))
    assert path_lib.object_bsdf({"type": "pbr", "albedo": [0.95, 0.64, 0.54], "roughness": 0.07, "metallic": 0.5}) == (3, (0.95, 0.64, 0.54, 0.07, 0.5))
    assert path_lib.object_bsdf({"type": "pbr", "albedo": (0.0, 1.0, 0.5)})[1][:3] == (0.0, 1.0, 0.5)
    nan, inf = float("nan"), float("inf")
    for field, values in (("albedo", (-0.01, 1.5, nan, inf, [0.5, 0.5, 1.01], [0.5, nan, 0.5], [0.1, 0.2], [[0.1, 0.2, 0.3]])),
                          ("roughness", (0.05, 0.0, 0.0699, 1.01, -1.0, nan, inf)), ("metallic", (-0.01, 1.01, nan, inf))):
        for v in values:
            with pytest.raises(ValueError, match=field):
                path_lib.object_bsdf({"type": "pbr", field: v})
    for bad in ({"type": "plastic"}, {"type": "glass"}, {"type": "PBR"}, {}, None, "pbr"):
        with pytest.raises(ValueError, match="type"):
            path_lib.object_bsdf(bad)
    # the two other types are what they were
    assert path_lib.object_bsdf(po.GLASS) == (1, (1.49, 1.000277, 0.0)) and path_lib.object_bsdf(po.DIFFUSE_08) == (2, (0.8, 0.8, 0.8))
    # the CPU twins of the object samplers know no PBR object: its sampler is the depth mesh's device code
    with pytest.raises(ValueError, match="pbr"):
        path_lib.object_sample_host(pp.PLASTIC, np.float32([0, 0, 1]), np.float32([[0, 0, 1]]), np.float32([[0.5, 0.5, 0.5]]))

    Vs = np.array([[0.0, 0.0, -2.0], [1.0, 0.0, -2.0], [0.0, 1.0, -2.0]])
    Ts = np.array([[0, 1, 2]], np.int32)
    V, T, U = ps.icosphere((0.0, 0.0, -1.0), 0.2, 0)
    Vc, Tc = po.cube((0.3, 0.0, -1.0), 0.1, (0.1, 0.2, 0.3))
    objects = [{"vertices": Vc, "triangles": Tc, "bsdf": po.DIFFUSE_08}, {"vertices": V, "triangles": T, "bsdf": pp.METAL, "normals": U},
               {"vertices": Vc + 0.5, "triangles": Tc, "bsdf": pp.PLASTIC}, {"vertices": V + 0.5, "triangles": T, "bsdf": po.GLASS}]
    assert len(path_lib.merge_objects(Vs, Ts, objects)) == 3 and len(path_lib.merge_objects(Vs, Ts, objects, normals=True)) == 4
    out = path_lib.merge_objects(Vs, Ts, objects, pbr=True)
    assert len(out) == 4 and len(path_lib.merge_objects(Vs, Ts, objects, normals=True, pbr=True)) == 5
    table, records = out[2], out[3]
    assert [t.kind for t in table] == [2, 3 | path_lib.OBJECT_SMOOTH, 3, 1]
    assert [(t.first_tri, t.n_tri) for t in table] == [(1, 12), (13, 20), (33, 12), (45, 20)]
    assert all(tuple(table[k].p) == (0.0, 0.0, 0.0) for k in (1, 2))    # a PBR entry's p[] carries nothing
    assert len(records) == 4 and all(isinstance(x, path_lib.PathObjectPbr) for x in records)
    f32 = lambda *x: tuple(float(np.float32(v)) for v in x)
    assert (tuple(records[1].a), records[1].r, records[1].m) == (f32(0.95, 0.64, 0.54), *f32(0.07, 1.0))
    assert (tuple(records[2].a), records[2].r, records[2].m) == (f32(0.5, 0.5, 0.5), *f32(0.6, 0.0))
    for k in (0, 3):                                                    # zero where the object is of another kind
        assert (tuple(records[k].a), records[k].r, records[k].m) == ((0.0, 0.0, 0.0), 0.0, 0.0)
    with pytest.raises(ValueError, match="roughness"):
        path_lib.merge_objects(Vs, Ts, [dict(objects[2], bsdf={"type": "pbr", "roughness": 0.01})], pbr=True)


# ---- 3: the table lookup and the C ABI's checks ------------------------------------------------------------------------------------------
def _table8(path_lib):
    """Eight objects with mixed kinds and smooth flags, ranges in no particular order with gaps between some; the smallest range
    starts at 100."""
    S = path_lib.OBJECT_SMOOTH
    spec = [(3, 140, 7, None), (1 | S, 100, 20, (1.49, 1.0, 0.0)), (3 | S, 400, 1, None), (2, 147, 13, (0.8, 0.5, 0.3)),
            (3, 160, 40, None), (2 | S, 300, 100, (0.1, 0.2, 0.3)), (1, 120, 20, (1.33, 1.0, 0.0)), (3 | S, 1000, 50000, None)]
    rng = np.random.default_rng(31)
    table, records = [], []
    for kind, first, n, p in spec:
        table.append(path_lib.PathObject(kind, first, n, (ctypes.c_float * 3)(*(p or (0.0, 0.0, 0.0)))))
        is_pbr = kind & ~S == 3
        a = rng.uniform(0, 1, 3) if is_pbr else np.zeros(3)
        records.append(path_lib.PathObjectPbr((ctypes.c_float * 3)(*a), rng.uniform(0.07, 1) if is_pbr else 0.0, rng.uniform(0, 1) if is_pbr else 0.0))
    return spec, table, records


def test_table_lookup_runs_the_kernels_routine(path_lib):
    spec, table, records = _table8(path_lib)
    ids = [99, -5, 0]                                                   # one below the smallest range, and further below
    for _, first, n, _ in spec:
        ids += [first, first + n - 1]                                   # the first and the last triangle of each range
    ids += [200, 299, 401, 999, 51000, 2 ** 31 - 1]                     # in the gaps and past the end
    ids = np.array(ids, np.int32)
    kind, a, r, m = path_lib.object_lookup_host(table, records, ids)
    for q, i in enumerate(ids.tolist()):
        owner = [k for k, (_, first, n, _) in enumerate(spec) if first <= i < first + n]
        assert len(owner) <= 1
        if not owner:
            assert kind[q] == 0 and not a[q].any() and r[q] == 0 and m[q] == 0, i
            continue
        k = owner[0]
        assert kind[q] == spec[k][0], (i, k)                            # the smooth flag is kept
        if spec[k][0] & ~path_lib.OBJECT_SMOOTH == 3:
            assert tuple(a[q]) == tuple(records[k].a) and r[q] == records[k].r and m[q] == records[k].m, (i, k)
        else:
            assert not a[q].any() and r[q] == 0 and m[q] == 0, (i, k)
    assert (kind == 0).sum() == 9 and (kind != 0).sum() == 16
    # without a PBR object the records may be missing
    plain = [t for t, s in zip(table, spec) if s[0] & ~path_lib.OBJECT_SMOOTH != 3]
    k2 = path_lib.object_lookup_host(plain, None, ids)[0]
    assert np.array_equal(k2 != 0, np.isin(kind & ~path_lib.OBJECT_SMOOTH, (1, 2)))


def test_c_abi_rejects_bad_records_before_any_gpu_work(path_lib):
    lib = path_lib.load()
    P = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    tab = lambda t: ctypes.cast(t, ctypes.c_void_p)
    ids = np.array([1, 5], np.int32)
    kind, a, r, m = np.zeros(2, np.int32), np.zeros((2, 3), np.float32), np.zeros(2, np.float32), np.zeros(2, np.float32)
    lookup = lambda t, n, rec: lib.matpbr_path_object_lookup_host(tab(t), n, tab(rec) if rec is not None else None, P(ids), 2, P(kind), P(a), P(r), P(m))
    obj = lambda k: (path_lib.PathObject * 1)(path_lib.PathObject(k, 1, 20, (ctypes.c_float * 3)(9.0, -9.0, float("nan"))))   # p[] is ignored
    rec = lambda a0, r0, m0: (path_lib.PathObjectPbr * 1)(path_lib.PathObjectPbr((ctypes.c_float * 3)(*a0), r0, m0))
    good = rec((0.0, 1.0, 0.5), 0.07, 1.0)
    assert lookup(obj(3), 1, good) == 0 and kind.tolist() == [3, 3]
    assert lookup(obj(0x103), 1, good) == 0 and kind.tolist() == [0x103, 0x103]
    nan, inf = float("nan"), float("inf")
    bad = [rec((0.5, 0.5, 0.5), 0.05, 0.0), rec((1.5, 0.5, 0.5), 0.5, 0.0), rec((0.5, 0.5, nan), 0.5, 0.0), rec((0.5, 0.5, 0.5), nan, 0.0),
           rec((0.5, 0.5, 0.5), 0.5, nan), rec((0.5, -0.1, 0.5), 0.5, 0.0), rec((0.5, 0.5, 0.5), 1.5, 0.0), rec((0.5, 0.5, 0.5), 0.5, 1.5),
           rec((0.5, 0.5, 0.5), 0.5, -0.5), rec((0.5, inf, 0.5), 0.5, 0.5), rec((0.5, 0.5, 0.5), inf, 0.5)]
    for b in bad:
        assert lookup(obj(3), 1, b) == -1
    assert lookup(obj(3), 1, None) == -1                                # a PBR object needs its record
    assert lookup(obj(4), 1, good) == -1 and lookup(obj(0x203), 1, good) == -1   # still unknown kinds
    # the renders: validation precedes the launch, so no GPU is needed
    one = np.zeros(1, np.float32)
    head = [P(one)] * 5 + [4, 4, 35.0] + [P(one)] * 4 + [2, 4, 1, 4, 0, 1, P(one), None, None]
    for k in (3, 0x103):
        assert lib.matpbr_path_render_objects(*head, tab(obj(k)), 1) == -1                       # an unknown kind there
        assert lib.matpbr_path_render_objects_normals(*head, tab(obj(k)), 1, P(one), 1) == -1    # and there
    render = lib.matpbr_path_render_objects_pbr
    for b in bad:
        assert render(*head, tab(obj(3)), 1, None, 1, tab(b)) == -1
    assert render(*head, tab(obj(3)), 1, None, 1, None) == -1           # no records
    assert render(*head, tab(obj(0x103)), 1, None, 1, tab(good)) == -1  # a smooth object needs its normals
    assert render(*head, tab(obj(3)), 1, None, 2, tab(good)) == -1      # a range that starts below n_scene_tri
    assert render(*head, tab(obj(3)), 9, None, 1, tab(good)) == -1      # more than MATPBR_PATH_MAX_OBJECTS
    assert render(*head, tab(obj(4)), 1, None, 1, tab(good)) == -1
    bad_depth = list(head)
    bad_depth[15] = 17                                                  # max_depth beyond MATPBR_PATH_MAX_MAX_DEPTH, a valid table
    assert render(*bad_depth, tab(obj(3)), 1, None, 1, tab(good)) == -1
    # the features take the kind without a record (host entry point: no device)
    Vs, Ts = pp.FAR_TRIANGLE
    Vq, Tq = pp.quad()
    V, T, table, _, _ = path_lib.merge_objects(Vs, Ts, [{"vertices": Vq, "triangles": Tq, "bsdf": pp.PLASTIC}], normals=True, pbr=True)
    geom = path_lib.features_host(path_lib.build_bvh(V, T, 1), 5, 6, FOV, table, None, 1)
    assert np.all(geom[..., 7] == 1.0) and np.abs(geom[..., 4:7] - [0.0, 0.0, 1.0]).max() <= 1e-6


# ---- 4: the restatement against itself ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_depth", [2, 4])
def test_a_flat_pbr_quad_is_the_depth_mesh_with_constant_maps(oracle64, path_lib, max_depth):
    """"The depth mesh's branch on constants": a camera-facing quad with constant maps as the depth mesh (`path_fp64.replay`), and the
    same quad as a flat PBR object over a depth mesh that is one far-off triangle out of view, give the same fp64 numbers in every
    pixel (no tolerance: the statements and their order are the same)."""
    H, W = 10, 12
    Vq, Tq = pp.quad()
    Vq = Vq.astype(np.float32).astype(np.float64)
    const = {"albedo": (0.8, 0.45, 0.3), "roughness": 0.35, "metallic": 0.6}
    ca, cr, cm = pp.pbr_constants(const)
    a = np.broadcast_to(ca.astype(np.float32), (H, W, 3)).copy()
    r, m = np.full((H, W, 1), cr, np.float32), np.full((H, W, 1), cm, np.float32)
    env = pf.groove_env(np.random.default_rng(5))
    tab = path_lib.env_tables(env)
    Vs, Ts = pp.FAR_TRIANGLE
    V, T, table = pob.merged(Vs, Ts, [{"vertices": Vq, "triangles": Tq, "bsdf": dict(const, type="pbr")}])
    for seed in (0, 1, 2):
        ref, _ = pf.replay(oracle64, Vq, Tq, a, r, m, env, tab, H, W, max_depth, seed)
        got, rec = pob.replay_objects(oracle64, V, T, np.zeros_like(a), np.ones_like(r), np.ones_like(m), env, tab, H, W, max_depth, seed, table)
        assert rec["pbr_vertex"].all() and not rec["pbr_smooth_vertex"].any() and not rec["fallback"].any()
        assert ref.any() and np.array_equal(got, ref), (max_depth, seed, np.abs(got - ref).max())


def test_restatement_without_pbr_objects_is_the_smooth_restatement(oracle64, path_lib):
    """On the smooth table the walk returns the bits the smooth restatement returned before the walks were folded into one
    (`path_testlib.recorded_walk`)."""
    from materialist_amd import mesh

    H, W = 10, 12
    rm = mesh.reference_mesh(pf.groove_scene(H, W), FOV)
    rng = np.random.default_rng(11)
    a, r, m = pf.groove_maps(H, W, rng)
    env = pf.groove_env(rng)
    V, T, table = pob.merged(rm["vertices"], rm["triangles"], ps.table_scene())
    args = (oracle64, V, T, a, r, m, env, path_lib.env_tables(env), H, W, 6, 1, table)
    rec0 = tl.recorded_walk("smooth")
    ref = rec0["L"]
    got, rec1 = pob.replay_objects(*args)
    assert np.array_equal(ref, got) and not rec1["pbr_vertex"].any()
    assert all(np.array_equal(rec0[k], rec1[k]) for k in ("transmitted", "diffuse_object", "blocked_by_object", "redo", "fallback"))


# ---- 5, 6: the GPU test's scene ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table(path_lib):
    """The GPU test's scene: the groove at 24 x 20 with `path_oi_pbr_fp64.table_scene` in front of it."""
    from materialist_amd import mesh

    H, W = 20, 24
    rm = mesh.reference_mesh(pf.groove_scene(H, W), FOV)
    rng = np.random.default_rng(11)
    a, r, m = pf.groove_maps(H, W, rng)
    env = pf.groove_env(rng)
    objects = pp.table_scene()
    V, T, tab = pob.merged(rm["vertices"], rm["triangles"], objects)
    return {"rm": rm, "a": a, "r": r, "m": m, "env": env, "tab": path_lib.env_tables(env), "H": H, "W": W, "objects": objects, "V": V, "T": T,
            "table": tab}


def test_restatement_over_fp32_and_fp64_traversal(table, path_lib, oracle64):
    """The GPU criterion's cap: the restatement over the library's fp32 traversal and over the fp64 brute force may differ in at
    most 1 % of the pixels of each of the six renders (the counts are reported).  The scene does what it is for: a PBR vertex, a
    smooth PBR vertex and an emitter sample blocked by an object in every render; a BSDF sample ended below the face and a fallback
    at least once over the six."""
    g = table
    Vm, Tm, tb, corner, records = path_lib.merge_objects(g["rm"]["vertices"], g["rm"]["triangles"], g["objects"], normals=True, pbr=True)
    n_scene = g["rm"]["triangles"].shape[0]
    assert [t.kind for t in tb] == [0x103, 3, 0x101, 2] and Tm.shape[0] - n_scene == 184
    for entry, rec_ in zip(g["table"], records):                       # the constants the library holds are the restatement's
        if entry["bsdf"]["type"] == "pbr":
            ca, cr, cm = pp.pbr_constants(entry["bsdf"])
            assert tuple(rec_.a) == tuple(ca) and rec_.r == cr and rec_.m == cm
    bvh = path_lib.build_bvh(Vm, Tm, n_scene)

    def closest(o, d):
        t, k = path_lib.trace_host(bvh, o, d)
        return np.where(k < 0, np.inf, t.astype(np.float64)), k.astype(np.int64)

    occluded = lambda o, d: path_lib.trace_host(bvh, o, d)[1] >= 0
    keys = ("pbr_vertex", "pbr_smooth_vertex", "blocked_by_object", "pbr_below_ng", "pbr_below_ng_carrying", "pbr_emitter_below_ng", "fallback")
    seen = {k: 0 for k in keys}
    differ = []
    for max_depth in (6, 16):
        for seed in (0, 1, 2):
            args = (oracle64, g["V"], g["T"], g["a"], g["r"], g["m"], g["env"], g["tab"], g["H"], g["W"], max_depth, seed, g["table"])
            L64, rec = pob.replay_objects(*args)
            L32, _ = pob.replay_objects(*args, closest=closest, occluded=occluded)
            err = (np.abs(L32 - L64) / np.maximum(np.abs(L64), np.abs(L64).mean())).max(-1)
            differ.append(int((err > 1e-3).sum()))
            assert differ[-1] <= 0.01 * g["H"] * g["W"], (max_depth, seed, differ[-1])
            for k in ("pbr_vertex", "pbr_smooth_vertex", "blocked_by_object"):
                assert rec[k].any(), (k, max_depth, seed)
            for k in seen:
                seen[k] += int(rec[k].sum())
    assert seen["pbr_below_ng"] >= 1 and seen["fallback"] >= 1
    _report("restatement over fp32 vs fp64 traversal: pixels that differ in each of the six renders (cap 4 of 480)", differ)
    _report("pixels with " + " / ".join(keys) + " (6 renders)", " / ".join(str(seen[k]) for k in keys))


def test_features_and_the_albedo_guide_of_pbr_objects(table, path_lib, oracle64):
    import torch
    from denoise_fp64 import check_features
    from materialist_amd import relight
    from test_denoise_host import feature_reference

    g = table
    H, W = g["H"], g["W"]
    Vm, Tm, tb, corner, _ = path_lib.merge_objects(g["rm"]["vertices"], g["rm"]["triangles"], g["objects"], normals=True, pbr=True)
    n_scene = g["rm"]["triangles"].shape[0]
    ref, bvh = feature_reference(path_lib, oracle64, Vm, Tm, n_scene, tb, corner, H, W)
    got = path_lib.features_host(bvh, H, W, FOV, tb, corner, n_scene)
    assert set(np.unique(ref[..., 7])) >= {0.0, 1.0, 2.0, 3.0, 4.0}     # the mesh and all four objects are seen
    check_features(got, ref, f"pbr table {H}x{W}", _report)            # id exact, n to 1e-5
    bsdfs = [ob["bsdf"] for ob in g["objects"]]
    guide = relight.albedo_guide(torch.from_numpy(got), torch.from_numpy(g["a"]), bsdfs).numpy()
    ids = got[..., 7]
    assert np.all(guide[ids == 1] == np.float32(pp.METAL["albedo"])) and (ids == 1).sum() > 5
    assert np.all(guide[ids == 2] == np.float32(0.5)) and (ids == 2).sum() > 5
    assert np.all(guide[ids == 3] == 1.0) and np.all(guide[ids == 4] == np.float32(0.8))
    assert np.array_equal(guide[ids == 0], g["a"][ids == 0])
    none = relight.albedo_guide(torch.from_numpy(got), torch.from_numpy(g["a"]), [{"type": "pbr"}] + bsdfs[1:]).numpy()
    assert np.all(none[ids == 1] == np.float32(0.8))                     # object_bsdf's default albedo


# ---- 7: the object list file -------------------------------------------------------------------------------------------------------------
def test_oi_scene_file(tmp_path, capsys):
    import render_final
    from materialist_amd import mesh, relight

    a = render_final.parse_args(["--save_name", "case", "--mode", "oi", "--oi_scene", "scene.json"])
    assert a.oi_scene == "scene.json" and render_final.parse_args(["--save_name", "case", "--mode", "oi"]).oi_scene is None
    os.makedirs(tmp_path / "case" / "best_results")
    os.makedirs(tmp_path / "lists" / "meshes")
    Vc, Tc = po.cube((0.1, -0.04, -1.0), 0.14, (-0.3, 0.7, 0.2))
    mesh.write_ply(str(tmp_path / "lists" / "meshes" / "ball.ply"), Vc, Tc)
    mesh.write_ply(str(tmp_path / "lists" / "cube.ply"), Vc, Tc)
    path = str(tmp_path / "lists" / "scene.json")

    def write(doc):
        with open(path, "w") as f:
            f.write(doc if isinstance(doc, str) else json.dumps(doc))

    chrome = {"type": "pbr", "albedo": [0.95, 0.93, 0.88], "roughness": 0.1, "metallic": 1.0}
    write({"objects": [{"ply": "meshes/ball.ply", "bsdf": chrome, "normals": "vertex"}, {"ply": "cube.ply", "bsdf": po.GLASS},
                       {"ply": "cube.ply", "bsdf": {"type": "diffuse", "reflectance": 0.3}, "normals": "flat"}]})
    got = relight.load_oi_scene(path)
    assert [e["ply"] for e in got] == [str(tmp_path / "lists" / "meshes" / "ball.ply")] + [str(tmp_path / "lists" / "cube.ply")] * 2
    assert [e["normals"] for e in got] == ["vertex", "flat", "flat"] and got[0]["bsdf"] == chrome and got[1]["bsdf"] == po.GLASS
    # with the file, oi.ply and oi2.ply are not looked for: the next check is the first that fails
    with pytest.raises(ValueError, match="n_iter"):
        relight.render_oi("case", input_path=str(tmp_path), save_path=str(tmp_path), objects_file=path, n_iter=0)
    with pytest.raises(ValueError, match="No envmap found"):
        relight.render_oi("case", input_path=str(tmp_path), save_path=str(tmp_path), objects_file=path, object_normals="vertex")
    ball = {"ply": "meshes/ball.ply", "bsdf": chrome}
    errors = [({"objects": [dict(ball, colour=1)]}, r"objects\[0\].*'colour'"),
              ({"objects": [ball, {"ply": "meshes/none.ply", "bsdf": chrome}]}, r"objects\[1\].*none\.ply"),
              ({"objects": [ball, {"bsdf": chrome}]}, r"objects\[1\].*'ply'"),
              ({"objects": [ball, ball, dict(ball, bsdf={"type": "pbr", "roughness": 0.01})]}, r"objects\[2\].*roughness"),
              ({"objects": [dict(ball, bsdf={"type": "plastic"})]}, r"objects\[0\].*bsdf"),
              ({"objects": [{"ply": "meshes/ball.ply"}]}, r"objects\[0\].*bsdf"),
              ({"objects": [dict(ball, normals="smooth")]}, r"objects\[0\].*normals"),
              ({"objects": [ball] * 9}, "at most 8"),
              ({"objects": []}, "empty"), ({"objects": [ball], "camera": {}}, "'camera'"), ({"meshes": [ball]}, "objects"), ([ball], "objects"),
              ({"objects": ["meshes/ball.ply"]}, r"objects\[0\]"), ("{not json", "cannot read")]
    for doc, pattern in errors:
        write(doc)
        with pytest.raises(ValueError, match=pattern) as e:
            relight.render_oi("case", input_path=str(tmp_path), save_path=str(tmp_path), objects_file=path)
        assert "scene.json" in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="absent.json"):
        relight.render_oi("case", input_path=str(tmp_path), save_path=str(tmp_path), objects_file=str(tmp_path / "absent.json"))
    write({"objects": [ball] * 8})
    assert len(relight.load_oi_scene(path)) == 8
    # without the file: today's behaviour, today's words
    with pytest.raises(FileNotFoundError, match="oi.ply.*oi2.ply") as e:
        relight.render_oi("case", input_path=str(tmp_path), save_path=str(tmp_path))
    scene_dir = os.path.join(str(tmp_path), "case")
    assert str(e.value) == (f"object insertion needs {os.path.join(scene_dir, 'oi.ply')} (glass) or {os.path.join(scene_dir, 'oi2.ply')} (diffuse); "
                            "neither exists")
    with pytest.raises(SystemExit):
        render_final.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--oi_scene" in text and "oi.ply and <scene>/oi2.ply are not looked for and --oi_normals is ignored" in text
