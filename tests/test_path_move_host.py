"""Moving inserted objects on the CPU ("Moving inserted objects"): the grafted build against the merged build, the
edges of its layout, the identity and the absence of drift, a move against fp64, the lights, and every refusal that precedes the device:
bad poses, a pose beyond `reach`, a tracer that is not movable, `load_oi_scene`'s new keys and the static bake.  CPU only; the device
twin is held to these bytes by tests/test_gpu_path_move.py."""
import json
import os

import numpy as np
import pytest

import path_fp64 as pf
import path_light_fp64 as pl
import path_move_testlib as ml
import path_oi_fp64 as po
import path_testlib as tl

_report = tl.reporter("path move", "test_path_move_host")
N_RAYS = 4096


@pytest.fixture(scope="module")
def path_lib():
    return tl.load()


@pytest.fixture(scope="module")
def groove(path_lib):
    """The 24 x 20 groove with the two cubes: the merged mesh, its table, the merged and the grafted BVH, 4096 rays inside its box."""
    from materialist_amd import mesh

    rm = mesh.reference_mesh(pf.groove_scene(20, 24), pf.FOV)
    objects = po.two_cubes()
    V, T, table = path_lib.merge_objects(rm["vertices"], rm["triangles"], objects)
    ns = rm["triangles"].shape[0]
    rng = np.random.default_rng(5)
    o = rng.uniform(V.min(0), V.max(0), (N_RAYS, 3))
    d = rng.normal(size=(N_RAYS, 3))                    # uniform on the sphere, aimed at nothing
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return {"rm": rm, "objects": objects, "V": V, "T": T, "table": table, "ns": ns, "o": o, "d": d,
            "merged": path_lib.build_bvh(V, T, ns), "grafted": path_lib.build_bvh_grafted(V, T, ns, ml.REACH)}


def _same_hits(path_lib, a, b, o, d, ns, what):
    """Closest hits and both scene walks through BVH `a` and `b`: the same id and the same bits of t, but for rays whose two ids lie at
    bit-equal distances, a tie the traversal order decides -> the number of such rays."""
    ties = 0
    walks = [("closest", lambda bvh: path_lib.trace_host(bvh, o, d))] + \
        [(f"scene any={any_}", lambda bvh, any_=any_: path_lib.trace_scene_host(bvh, o, d, ns, any=bool(any_))) for any_ in (0, 1)]
    for name, walk in walks:
        (ta, ka), (tb, kb) = walk(a), walk(b)
        assert np.array_equal(ka >= 0, kb >= 0), (what, name)                       # hit or miss
        if name.endswith("any=1"):                                                    # the first triangle found: the order decides which
            continue
        differ = ka != kb
        assert np.array_equal(ta.view(np.uint32), tb.view(np.uint32)), (what, name, int((ta != tb).sum()))
        ties += int(differ.sum())                                                     # equal bits of t and another id: a tie
    return ties


def test_grafted_build_traces_as_the_merged_build(path_lib, groove):
    g = groove
    ties = _same_hits(path_lib, g["grafted"], g["merged"], g["o"], g["d"], g["ns"], "groove")
    t, k = path_lib.trace_host(g["grafted"], g["o"], g["d"])
    _report("grafted against merged BVH, 4096 rays x 3 walks: rays with another id at a bit-equal distance (ties)",
            f"{ties}; {int((k >= 0).sum())} rays hit, {int((k >= g['ns']).sum())} of them an object")
    assert (k >= g["ns"]).sum() > 50 and ((k >= 0) & (k < g["ns"])).sum() > 500
    assert ties <= 4


def _scene_side_is_the_scene_alone(path_lib, g, Vs, Ts):
    """The scene side's topology and boxes are `build_bvh`'s over the scene alone, every node index one higher."""
    alone = path_lib.build_bvh(Vs, Ts)
    ba, ca, na = ml.nodes_of(alone)
    bg, cg, ng = ml.nodes_of(g)
    n = alone["n_nodes"]
    assert g["first_object_node"] == 1 + n
    assert np.array_equal(na, ng[1:1 + n]) and np.array_equal(ba.view(np.uint32), bg[1:1 + n].view(np.uint32))
    assert np.array_equal(np.where(na < 0, ca + 1, ca), cg[1:1 + n])
    assert np.array_equal(alone["tris"], g["tris"][:alone["tris"].size])
    lo, hi = np.minimum(ba[0, 0, 0], ba[0, 1, 0]), np.maximum(ba[0, 0, 1], ba[0, 1, 1])
    assert np.array_equal(bg[0, 0, 0], lo) and np.array_equal(bg[0, 0, 1], hi)


@pytest.mark.parametrize("case", ["1 triangle", "4 triangles", "5 triangles", "8 objects", "scene of 2", "sliver scene", "sliver object"])
def test_edges_of_the_layout(path_lib, groove, case):
    rm = groove["rm"]
    Vs, Ts = rm["vertices"], rm["triangles"]
    Vc, Tc = po.cube((0.10, -0.04, -1.40), 0.20, (-0.3, 0.7, 0.2))
    if case in ("1 triangle", "4 triangles", "5 triangles"):          # slot 1 a leaf, a full leaf, the first inner node
        objects = [{"vertices": Vc, "triangles": Tc[:int(case[0])], "bsdf": po.DIFFUSE_08}]
    elif case == "8 objects":
        objects = [{"vertices": Vc + (0.05 * k, 0, 0), "triangles": Tc, "bsdf": po.DIFFUSE_08} for k in range(8)]
    elif case == "scene of 2":                                        # slot 0 a leaf
        Vs, Ts = np.array([[-1, -1, -2], [1, -1, -2], [1, 1, -2], [-1, 1, -2]], np.float64), np.array([[0, 1, 2], [0, 2, 3]], np.int32)
        objects = po.two_cubes()
    elif case == "sliver scene":
        Vs, Ts = ml.sliver_mesh()
        objects = [{"vertices": ml.one_triangle()[0], "triangles": ml.one_triangle()[1], "bsdf": po.DIFFUSE_08}]
    else:
        objects = [{"vertices": ml.sliver_mesh()[0], "triangles": ml.sliver_mesh()[1], "bsdf": po.DIFFUSE_08}]
    V, T, table = path_lib.merge_objects(Vs, Ts, objects)
    ns = Ts.shape[0]
    g = path_lib.build_bvh_grafted(V, T, ns)
    depth, scene_nodes, object_nodes = ml.check_layout(path_lib, g, ns, T.shape[0])
    _report(f"layout, {case}", f"{g['n_nodes']} nodes ({len(object_nodes)} of the objects), depth {depth}, object depth {g['object_depth']}")
    if case.startswith("sliver"):
        assert depth == path_lib.MAX_BVH_DEPTH                        # the cap is reached: a side is cut one level below the builder's own
        assert path_lib.build_bvh(*ml.sliver_mesh())["depth"] == path_lib.MAX_BVH_DEPTH
    elif ns > 4:
        _scene_side_is_the_scene_alone(path_lib, g, Vs, Ts)
    rng = np.random.default_rng(9)
    P = V[T]
    aim = P[rng.integers(0, T.shape[0], 512)]                        # at random points of random triangles, from random origins
    w = rng.dirichlet((1, 1, 1), 512)
    target = (aim * w[:, :, None]).sum(1)
    o = target + rng.normal(size=(512, 3)) * np.abs(target).max(-1, keepdims=True)
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ties = _same_hits(path_lib, g, path_lib.build_bvh(V, T, ns), o, d, ns, case)
    assert ties <= 8, ties
    # the identity reproduces the build, whatever the layout
    ident = ml.records(path_lib, [None] * len(objects), objects)
    mv = path_lib.objects_move_host(g, table, ns, ident)
    assert np.array_equal(mv["nodes"], g["nodes"]) and np.array_equal(mv["tris"], g["tris"])


def _smooth_scene(path_lib, groove):
    """The groove with the glass cube and a smooth icosahedron."""
    Vi, Ti, Ni = ml.icosahedron()
    objects = [po.two_cubes()[0], {"vertices": Vi, "triangles": Ti, "bsdf": po.DIFFUSE_08, "normals": Ni}]
    rm = groove["rm"]
    V, T, table, nrm = path_lib.merge_objects(rm["vertices"], rm["triangles"], objects, normals=True)
    return objects, V, T, table, nrm, path_lib.build_bvh_grafted(V, T, groove["ns"], ml.REACH)


def test_identity_and_drift(path_lib, groove):
    """Move by the identity (None, an empty placement, a pivot alone): the build's bytes.  Move by M, then by the identity: the build's
    bytes again, because a move starts from the rest pose."""
    objects, V, T, table, nrm, g = _smooth_scene(path_lib, groove)
    ns = groove["ns"]
    for ident in ([None, None], [{}, {"pivot": (1, 2, 3)}], [{"scale": 1, "translate": (0, 0, 0)}, {"rotate": np.eye(3)}]):
        mv = path_lib.objects_move_host(g, table, ns, ml.records(path_lib, ident, objects), nrm)
        assert np.array_equal(mv["nodes"], g["nodes"]) and np.array_equal(mv["tris"], g["tris"])
        assert np.array_equal(mv["obj_nrm"].view(np.uint32), nrm.view(np.uint32))
    M = ml.records(path_lib, ml.POSES["oblique"], objects)
    moved = path_lib.objects_move_host(g, table, ns, M, nrm)
    assert not np.array_equal(moved["tris"], g["tris"]) and not np.array_equal(moved["obj_nrm"], nrm)
    again = path_lib.objects_move_host(g, table, ns, M, nrm)
    assert all(np.array_equal(moved[k], again[k]) for k in ("nodes", "tris", "obj_nrm"))
    back = path_lib.objects_move_host(dict(g, nodes=moved["nodes"], tris=moved["tris"]), table, ns, ml.records(path_lib, [None, None], objects), nrm)
    assert np.array_equal(back["nodes"], g["nodes"]) and np.array_equal(back["tris"], g["tris"]) and np.array_equal(back["obj_nrm"], nrm)


def _ulp_at(x):
    """The fp32 ulp at magnitude x (> 0)."""
    return np.spacing(np.asarray(x, np.float64).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("pose", list(ml.POSES))
def test_a_move_against_fp64(path_lib, groove, pose):
    """The corners.  The library evaluates p' = R (s (p - c)) + (c + t) in three steps, each in fp64 on the fp32 inputs: the scaled
    offset q = s (p - c), the rotation R q (three products and two sums a row), the sum with c + t.  Every fp64 operation is exact to
    2^-53 of its result, and no intermediate exceeds A = |p| + |c| + |t| + s |p - c| in magnitude, so the three steps together err by
    less than 16 x 2^-53 A = 2^-49 A; the one rounding to fp32 adds half an ulp of the coordinate.  Against the same formula in numpy's
    fp64 (which errs as little), a stored coordinate therefore lies within 0.5 ulp + 2^-48 A of the reference, and A <= 4 S for the
    largest coordinate magnitude S of the pose (rest record, pivot, moved corner), so 2^-48 A <= 2^-46 S < 2^-22 ulp(S): far inside the 4
    ulp, at the pose's coordinate magnitude S, that the corners are held to, and the test also holds them to what the derivation gives:
    every stored v0' and edge component within 0.5 ulp of its own magnitude beyond the absolute 2^-46 S.  (A bound in ulp of the coordinate
    alone cannot hold: a rotation may carry a coordinate to zero, where 2^-46 S is all that is left.)  An edge is R (s e), the same without the offsets, held to 4 ulp at S as well, and so is the
    corner v0' + e' that the refit forms from them in fp32 (two half-ulps of the parts and one of the sum: 1.5 ulp)."""
    g, ns, objects, table = groove["grafted"], groove["ns"], groove["objects"], groove["table"]
    rec = ml.records(path_lib, ml.POSES[pose], objects)
    mv = path_lib.objects_move_host(g, table, ns, rec)
    rest, ids = ml.records_of(g)
    got, ids_moved = ml.records_of(mv)
    assert np.array_equal(ids, ids_moved)
    worst, tight = 0.0, 0.0
    raw_rest, raw_moved = (np.frombuffer(b["tris"].tobytes(), np.float32).reshape(-1, 3, 4)[:, :, :3].astype(np.float64) for b in (g, mv))
    for ob, sim in zip(table, ml.sims64(rec)):
        sel = (ids >= ob.first_tri) & (ids < ob.first_tri + ob.n_tri)
        sel[:ns] = False
        ref = path_lib.apply_similarity(sim, rest[sel])
        S = max(np.abs(rest[sel]).max(), np.abs(ref).max(), np.abs(sim[3]).max())
        worst = max(worst, float(np.abs(got[sel] - ref).max() / _ulp_at(S)))
        # the stored v0' and edges one by one, at each coordinate's own magnitude: half an ulp of it, plus the three steps' 2^-48 A <= 2^-46 S
        R, sc = sim[0], sim[1]
        for have, want in ((raw_moved[sel, 0], ref[:, 0]), (raw_moved[sel, 1], sc * raw_rest[sel, 1] @ R.T), (raw_moved[sel, 2], sc * raw_rest[sel, 2] @ R.T)):
            own = np.abs(have - want) - 2.0 ** -46 * S
            tight = max(tight, float((own / _ulp_at(np.maximum(np.abs(want), 1e-30))).max()))
    _report(f"pose {pose}: largest corner error against the fp64 transform of the rest record, in ulp at the pose's magnitude / at the "
            f"coordinate's own beyond 2^-46 S", f"{worst:.3f} / {tight:.3f}")
    assert worst <= 4.0                                               # the bound the feature states
    assert tight <= 0.5 + 1e-6                                        # and what the fp64 evaluation derives above: an fp32 transform (a few ulp) fails here
    # the scene's nodes and triangles are the build's bytes
    first = g["first_object_node"]
    assert np.array_equal(mv["nodes"][64:64 * first], g["nodes"][64:64 * first]) and np.array_equal(mv["nodes"][:24], g["nodes"][:24])
    assert np.array_equal(mv["nodes"][48:64], g["nodes"][48:64]) and np.array_equal(mv["tris"][:48 * ns], g["tris"][:48 * ns])
    # every leaf box holds its triangles' fp64 corners, every parent box its child's two, slot 1 of node 0 all of them
    boxes, child, count = ml.nodes_of(mv)
    moved64 = rest.copy()
    for ob, sim in zip(table, ml.sims64(rec)):
        sel = (ids >= ob.first_tri) & (ids < ob.first_tri + ob.n_tri)
        moved64[sel] = path_lib.apply_similarity(sim, rest[sel])
    slots = [(0, 1)] + [(q, s) for q in range(first, g["n_nodes"]) for s in (0, 1)]
    for q, s in slots:
        lo, hi = boxes[q, s, 0].astype(np.float64), boxes[q, s, 1].astype(np.float64)
        if count[q, s] >= 0:
            c = moved64[child[q, s]:child[q, s] + count[q, s]]
            assert np.all(c >= lo) and np.all(c <= hi), (q, s)
        else:
            kid = boxes[child[q, s]].astype(np.float64)
            assert np.all(kid[:, 0] >= lo) and np.all(kid[:, 1] <= hi), (q, s)
    assert np.all(moved64[ns:] >= boxes[0, 1, 0]) and np.all(moved64[ns:] <= boxes[0, 1, 1])
    # closest hits through the moved BVH name the triangle an fp64 brute force over the fp64-transformed mesh names
    moved = ml.moved_objects(path_lib, objects, rec)
    Vm, Tm, _ = po.merged(groove["rm"]["vertices"], groove["rm"]["triangles"], [dict(ob, vertices=ob["vertices"]) for ob in moved])
    Vm[groove["rm"]["vertices"].shape[0]:] = np.concatenate([ob["vertices"] for ob in moved])      # the moved vertices unrounded
    P = Vm[Tm]
    lo, hi = P.reshape(-1, 3).min(0), P.reshape(-1, 3).max(0)
    rng = np.random.default_rng(6)
    o = rng.uniform(lo, hi, (N_RAYS, 3))
    aim = rng.uniform(lo, hi, (N_RAYS, 3))
    aim[::2] = P[ns:].reshape(-1, 3)[rng.integers(0, 3 * (Tm.shape[0] - ns), N_RAYS // 2)] + rng.normal(size=(N_RAYS // 2, 3)) * 0.05   # half of them near the objects
    d = aim - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t, k = path_lib.trace_host(mv, o, d)
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    best = np.full(N_RAYS, np.inf)
    second = np.full(N_RAYS, np.inf)
    who = np.full(N_RAYS, -1)
    for c0 in range(0, N_RAYS, 512):
        tt = _all_hits(P, e1, e2, o[c0:c0 + 512], d[c0:c0 + 512])
        order = np.argsort(tt, axis=1)[:, :2]
        rows = np.arange(tt.shape[0])
        best[c0:c0 + 512], second[c0:c0 + 512] = tt[rows, order[:, 0]], tt[rows, order[:, 1]]
        who[c0:c0 + 512] = np.where(np.isfinite(tt[rows, order[:, 0]]), order[:, 0], -1)
    with np.errstate(invalid="ignore"):                              # inf - inf where a ray misses everything
        clear = ~(np.isfinite(second) & (second - best <= 1e-5 * best))
    left_out = 1.0 - clear.mean()
    _report(f"pose {pose}: rays left out (two nearest distances within 1e-5 relative) / rays that hit an object",
            f"{left_out:.4f} / {int((who >= ns).sum())}")
    assert left_out < 0.01
    assert (who >= ns).sum() > 100
    assert np.array_equal(k[clear], who[clear]), np.nonzero(k[clear] != who[clear])[0][:10]


def _all_hits(P, e1, e2, o, d):
    """fp64 Moller-Trumbore of every ray against every triangle -> t [N,T], inf where missed."""
    pv = np.cross(d[:, None], e2[None])
    det = (e1[None] * pv).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        tv = o[:, None] - P[None, :, 0]
        u = (tv * pv).sum(-1) / det
        qv = np.cross(tv, e1[None])
        v = (d[:, None] * qv).sum(-1) / det
        t = (e2[None] * qv).sum(-1) / det
    return np.where((det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0), t, np.inf)


def test_lights(path_lib, groove):
    """A quad light and a cube, the light scaled by 2 and turned: the header's area is (float)((double) area_rest 4) exactly, the cdf is
    not touched, the moved light records are the moved triangles of the same ids bit for bit, and the light tables rebuilt from the
    fp64-transformed mesh agree in area to 1e-5 relative: the rebuilt tables round the moved vertices to fp32 first (6e-8 relative a
    coordinate, on edges a few times shorter than the coordinates), the moved area is the rest area's rounding times 4."""
    rm, ns = groove["rm"], groove["ns"]
    quad = {"vertices": np.array([[-0.2, 0.5, -1.3], [0.2, 0.5, -1.3], [0.2, 0.5, -1.0], [-0.2, 0.5, -1.0]], np.float64),
            "triangles": np.array([[0, 1, 2], [0, 2, 3]], np.int32), "bsdf": pl.QUAD_LIGHT}
    objects = [po.two_cubes()[1], quad]
    V, T, table, lights = path_lib.merge_objects(rm["vertices"], rm["triangles"], objects, lights=True)
    g = path_lib.build_bvh_grafted(V, T, ns, ml.REACH)
    rec = ml.records(path_lib, [None, {"scale": 2.0, "rotate": {"axis": (1, 2, 3), "deg": 37}, "translate": (0.05, 0.1, 0.0)}], objects)
    cdf = lights["cdf"].copy()
    mv = path_lib.objects_move_host(g, table, ns, rec, None, lights)
    assert np.array_equal(lights["cdf"], cdf)
    rest_area = float(lights["header"].area[0])
    assert mv["area"] == [float(np.float32(rest_area * 4.0))]
    tf = np.frombuffer(mv["tris"].tobytes(), np.float32).reshape(-1, 3, 4)
    ids = tf[:, 0, 3].copy().view(np.int32)
    for r in range(2):
        k = int(np.nonzero(ids == table[1].first_tri + r)[0][0])
        assert np.array_equal(mv["light_tris"][r, :, :3].view(np.uint32), tf[k, :, :3].view(np.uint32)), r
        assert np.all(mv["light_tris"][r, :, 3] == 0)
    moved = ml.moved_objects(path_lib, objects, rec)
    V2, T2, table2, rebuilt = path_lib.merge_objects(rm["vertices"], rm["triangles"], moved, lights=True)
    rel = abs(float(rebuilt["header"].area[0]) - mv["area"][0]) / mv["area"][0]
    _report("light area after a move with s = 2 against the tables rebuilt from the fp64-transformed mesh, relative", f"{rel:.3e}")
    assert rel <= 1e-5
    assert np.allclose(rebuilt["cdf"], cdf, rtol=0, atol=1e-6)        # a similarity keeps the normalised cumulative areas


def _xform(path_lib, R=np.eye(3), s=1.0, t=(0, 0, 0), c=(0, 0, 0)):
    return path_lib.xform_records([(np.asarray(R, np.float64), s, np.asarray(t, np.float64), np.asarray(c, np.float64))])


def test_refusals_of_bad_poses(path_lib, groove):
    ok = lambda rec: path_lib.symbol("matpbr_path_xform_check_host")(path_lib._ref(rec[0]), 1)
    th = np.radians(37)
    rot = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]])
    assert ok(_xform(path_lib)) == 0 and ok(_xform(path_lib, rot, 2.5, (1, 2, 3), (4, 5, 6))) == 0
    shear = np.array([[1, 0.01, 0], [0, 1, 0], [0, 0, 1.0]])
    bad = {"a NaN": _xform(path_lib, t=(0, np.nan, 0)), "an infinite pivot": _xform(path_lib, c=(np.inf, 0, 0)), "s = 0": _xform(path_lib, s=0.0),
           "s < 0": _xform(path_lib, s=-1.0), "a sheared R": _xform(path_lib, shear), "a mirrored R": _xform(path_lib, np.diag([1.0, 1.0, -1.0])),
           "a scaled R": _xform(path_lib, 1.001 * rot)}
    for what, rec in bad.items():
        assert ok(rec) == -1, what
        with pytest.raises(ValueError, match="transform of object 0"):
            path_lib.check_xforms(rec)
    assert ok(_xform(path_lib, rot + 2e-6)) == 0                      # inside the 1e-5 the corner normals rely on
    # the host twin refuses them as the device entry does: by return code, before anything is written
    g, rec = groove["grafted"], ml.records(path_lib, [None, None], groove["objects"])
    rec[1].s = 0.0
    with pytest.raises(path_lib.PathError, match="invalid argument"):
        path_lib.objects_move_host(g, groove["table"], groove["ns"], rec)
    # the placement dicts
    for tr, words in (({"scale": 0}, "'scale' must be positive"), ({"spin": 1}, "unknown key 'spin'"), ({"rotate": {"axis": (0, 0, 0), "deg": 3}}, "axis must not be zero"),
                      ({"rotate": {"axis": (0, 1, 0)}}, "'rotate' must be"), ({"translate": (1, 2)}, "3 numbers"), ({"pivot": (0, 0, np.inf)}, "finite"),
                      ({"rotate": [[1, 0], [0, 1]]}, "3 x 3")):
        with pytest.raises(ValueError, match=words):
            path_lib.similarity(tr)


def test_tracer_refusals_precede_the_device(path_lib, groove, monkeypatch):
    """`movable=True` without objects, `move_objects` on a tracer that is not movable, a wrong count, a bad pose and a pose beyond
    `reach`: each a ValueError before the library's move or the device is reached.  The tracer here is built without a device: its
    fields are set by hand, which is all `poses` reads."""
    import torch

    rm, objects = groove["rm"], groove["objects"]
    with pytest.raises(ValueError, match="movable=True moves inserted objects"):
        path_lib.PathTracer(rm["vertices"], rm["triangles"], 20, 24, pf.FOV, device="cpu", movable=True)

    def touched(*_a, **_k):
        raise AssertionError("the refusal comes before the device and the library")

    monkeypatch.setattr(torch.cuda, "current_stream", touched)
    tracer = path_lib.PathTracer.__new__(path_lib.PathTracer)
    tracer.objects, tracer._move = [0, 0], None
    with pytest.raises(ValueError, match="needs a movable tracer"):
        tracer.move_objects([None, None])
    boxes = [(np.asarray(ob["vertices"]).min(0), np.asarray(ob["vertices"]).max(0)) for ob in objects]
    tracer._move, tracer.reach = {"boxes": boxes}, float(np.abs(groove["V"]).max())
    monkeypatch.setattr(path_lib, "symbol", lambda name, lib=None: touched() if name == "matpbr_path_objects_move" else path_lib.path_abi.symbol(name, lib))
    for transforms, words in (([None], "one entry per object"), ([None, {"scale": -2}], "'scale' must be positive"),
                              ([{"rotate": np.diag([1.0, 1.0, -1.0])}, None], "transform of object 0"),
                              ([None, {"translate": (6.0, 0, 0)}], "beyond this tracer's reach"), ([{"scale": 30.0}, None], "beyond this tracer's reach")):
        with pytest.raises(ValueError, match=words):
            tracer.move_objects(transforms)
    assert len(tracer.poses([{"translate": (0.01, 0, 0)}, None])) == 2          # and a good pose passes the checks
    tracer.reach = ml.REACH
    assert len(tracer.poses(ml.POSES["away"])) == 2


def _write_list(tmp_path, entries):
    from materialist_amd import mesh

    V, T = po.cube((0.0, 0.0, -1.3), 0.2, (0.2, 0.3, 0.1))
    mesh.write_ply(str(tmp_path / "cube.ply"), V, T)
    path = str(tmp_path / "list.json")
    with open(path, "w") as f:
        json.dump({"objects": [dict({"ply": "cube.ply", "bsdf": po.DIFFUSE_08}, **e) for e in entries]}, f)
    return path, V, T


def test_object_list_keys_rule_by_rule(path_lib, tmp_path):
    from materialist_amd import relight

    good = {"transform": {"scale": 2, "rotate": {"axis": [0, 1, 0], "deg": 30}, "translate": [0.1, 0, 0], "pivot": [0, 0, -1.3]},
            "motion": {"spin": {"axis": [0, 1, 0], "deg_per_frame": 10}, "slide": [0.01, 0, 0]}}
    path, V, T = _write_list(tmp_path, [good, {}])
    got = relight.load_oi_scene(path)
    assert got[0]["transform"] == good["transform"] and got[0]["motion"] == good["motion"] and got[1]["transform"] is None and got[1]["motion"] is None
    R, s, t, c = relight.oi_pose(good["transform"], good["motion"], 3)
    assert np.allclose(R, path_lib.rotation((0, 1, 0), 60)) and s == 2 and np.allclose(t, (0.13, 0, 0)) and np.allclose(c, (0, 0, -1.3))
    assert np.array_equal(relight.oi_pose(None, None, 5, pivot=(1, 2, 3))[3], (1, 2, 3))          # the default pivot is the caller's: the box centre
    bad = [({"transform": {"scale": 0}}, "'scale' must be positive"), ({"transform": {"scale": -1}}, "'scale' must be positive"),
           ({"transform": {"shear": 1}}, "unknown key 'shear'"), ({"transform": {"rotate": {"axis": [0, 0, 0], "deg": 1}}}, "axis must not be zero"),
           ({"transform": {"rotate": [[1, 0, 0], [0, 1, 0], [0, 0, 1]]}}, "'rotate' must be"), ({"transform": [1, 2]}, "'transform' must be an object"),
           ({"transform": {"translate": [1, 2]}}, "3 numbers"), ({"motion": {"roll": 1}}, "unknown key 'roll'"),
           ({"motion": {"spin": {"axis": [0, 0, 0], "deg_per_frame": 1}}}, "axis must not be zero"), ({"motion": {"spin": {"axis": [0, 1, 0]}}}, "'spin' must be"),
           ({"motion": {"slide": [1, 2]}}, "'slide' must be 3"), ({"motion": 3}, "'motion' must be an object"), ({"pose": {}}, "unknown key 'pose'")]
    for entry, words in bad:
        path, _, _ = _write_list(tmp_path, [{}, entry])
        with pytest.raises(ValueError, match=words) as e:
            relight.load_oi_scene(path)
        assert "list.json: objects[1]" in str(e.value), str(e.value)
    # a video of nothing that moves, and a bad frame count, before the scene is looked for (there is none)
    path, _, _ = _write_list(tmp_path, [{"transform": good["transform"]}, {"motion": {"slide": [0, 0, 0]}}])
    kw = {"input_path": str(tmp_path), "save_path": str(tmp_path)}
    with pytest.raises(ValueError, match="3 equal frames"):
        relight.render_oi("nothing", objects_file=path, frames=3, **kw)
    with pytest.raises(ValueError, match="3 equal frames"):
        relight.render_oi("nothing", frames=3, **kw)
    with pytest.raises(ValueError, match="frames must be at least 1"):
        relight.render_oi("nothing", objects_file=path, frames=0, **kw)


def test_static_bake(path_lib, tmp_path, monkeypatch, capsys):
    """`render_oi(frames=1)`: an identity transform hands the tracer the untransformed arrays' bytes, a transform the fp64 transform of
    the file's vertices and normals, and "motion" is ignored with a printed line.  The tracer is replaced by a recorder: no device."""
    from materialist_amd import mesh, relight

    scene = tl.synthetic_output(str(tmp_path), H=8, W=8)
    V, T = po.cube((0.0, 0.0, -1.3), 0.2, (0.2, 0.3, 0.1))
    Nn = mesh.angle_weighted_normals(V, T)
    tr = {"scale": 1.5, "rotate": {"axis": [1, 2, 3], "deg": 37}, "translate": [0.1, -0.05, 0.02]}
    entries = [{"normals": "vertex"}, {"normals": "vertex", "transform": {"scale": 1, "translate": [0, 0, 0], "rotate": {"axis": [0, 0, 1], "deg": 0}}},
               {"normals": "vertex", "transform": tr, "motion": {"slide": [0.1, 0, 0]}}]
    path, _, _ = _write_list(tmp_path, entries)
    seen = {}

    class Recorder(Exception):
        pass

    def tracer(scene_dir, save_name, mat, device, objects=None, **movable):
        seen["objects"], seen["movable"] = objects, movable
        raise Recorder

    monkeypatch.setattr(relight, "_path_tracer", tracer)
    monkeypatch.setattr(relight, "load_estimated_brdf", lambda *a, **k: {})
    with pytest.raises(Recorder):
        relight.render_oi("case", input_path=str(tmp_path), save_path=str(tmp_path), objects_file=path, device="cpu")
    assert os.path.isdir(scene) and seen["movable"] == {}
    plain, ident, baked = seen["objects"]
    Vf, Tf = mesh.read_ply_any(str(tmp_path / "cube.ply"))[:2]
    assert plain["vertices"].tobytes() == ident["vertices"].tobytes() == np.asarray(Vf).tobytes()
    assert np.asarray(plain["normals"]).tobytes() == np.asarray(ident["normals"]).tobytes()
    sim = path_lib.similarity(tr, pivot=0.5 * (np.asarray(Vf, np.float64).min(0) + np.asarray(Vf, np.float64).max(0)))
    assert np.array_equal(baked["vertices"], path_lib.apply_similarity(sim, Vf))
    assert np.array_equal(baked["normals"], path_lib.apply_similarity(sim, plain["normals"], vectors=True))
    assert np.allclose(np.linalg.norm(baked["vertices"][1] - baked["vertices"][0]), 1.5 * np.linalg.norm(Vf[1] - Vf[0]))
    assert '"motion" is ignored' in capsys.readouterr().out
    assert Nn.shape == plain["normals"].shape
