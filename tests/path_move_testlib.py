"""What the tests of moving inserted objects share (tests/test_path_move_host.py, tests/test_gpu_path_move.py; DESIGN.md section 1.4,
"Moving inserted objects"): the small meshes, the poses, the fp64 transform as the library's fp32 records state it, and the walk over a
grafted BVH's nodes.  A plain module beside path_testlib.py: no fixtures, nothing pytest collects."""
import numpy as np

import path_oi_fp64 as po

REACH = 8.0    # the movable tracers' `reach`: POSES["away"] carries a cube to x = 6


def icosahedron(centre=(0.02, 0.0, -1.2), radius=0.12):
    """20 triangles, outward winding, and its vertex normals (the directions from the centre) -> (V [12,3], T [20,3], N [12,3])."""
    g = (1 + 5 ** 0.5) / 2
    v = np.array([[-1, g, 0], [1, g, 0], [-1, -g, 0], [1, -g, 0], [0, -1, g], [0, 1, g], [0, -1, -g], [0, 1, -g], [g, 0, -1], [g, 0, 1], [-g, 0, -1],
                  [-g, 0, 1]], np.float64)
    T = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2],
                  [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], np.int32)
    n = v / np.linalg.norm(v, axis=1, keepdims=True)
    return n * radius + np.asarray(centre, np.float64), T, n


def one_triangle(z=-1.3):
    return np.array([[-0.1, -0.1, z], [0.15, -0.05, z], [0.0, 0.12, z + 0.05]], np.float64), np.array([[0, 1, 2]], np.int32)


def sliver_mesh(n=56, z=-1.0):
    """n triangles along x whose centroids are a factor 17 apart and equal in y and z: the builder's 16 bins can only peel the largest
    one off at every level, so its depth grows with n until the level cap makes a leaf of the rest."""
    x = 17.0 ** (np.arange(n) - n // 2)
    V = np.stack([np.stack([x, np.zeros(n), np.full(n, z)], -1), np.stack([1.5 * x, np.zeros(n), np.full(n, z)], -1),
                  np.stack([x, np.full(n, 0.25), np.full(n, z)], -1)], 1).reshape(-1, 3)
    return V, np.arange(3 * n, dtype=np.int32).reshape(-1, 3)


# the poses of the two cubes of `path_oi_fp64.two_cubes` (glass at z = -1.15, diffuse at z = -1.40; the groove lies at z <= -1.6)
POSES = {
    "quarter": [{"rotate": {"axis": (0, 1, 0), "deg": 90}}, None],                                    # 90 degrees about y: R is exact
    "oblique": [{"rotate": {"axis": (1, 2, 3), "deg": 37}}, {"rotate": {"axis": (1, 2, 3), "deg": 37}, "scale": 0.5}],
    "double": [{"scale": 2.0, "translate": (-0.1, 0.0, 0.3)}, {"scale": 0.5, "rotate": {"axis": (0, 1, 0), "deg": 90}}],
    "away": [{"translate": (6.0, 0.0, 0.0)}, {"translate": (0.0, 0.0, -0.35)}],                      # one cube out of the scene's box, one through the mesh
}


def records(pt, transforms, objects):
    """`PathTracer.poses` without a tracer: the PathXform records of `transforms` over `objects`, the default pivot the centre of each
    object's bounding box."""
    sims = []
    for tr, ob in zip(transforms, objects):
        v = np.asarray(ob["vertices"], np.float64)
        sims.append(pt.similarity(tr, pivot=0.5 * (v.min(0) + v.max(0))))
    rec = pt.xform_records(sims)
    pt.check_xforms(rec)
    return rec


def sims64(rec):
    """The records as fp64 similarities: the values the library holds, fp32, widened."""
    return [(np.array(x.R, np.float64).reshape(3, 3), float(x.s), np.array(x.t, np.float64), np.array(x.c, np.float64)) for x in rec]


def moved_objects(pt, objects, rec):
    """`objects` with their vertices (rounded to fp32 as the BVH stores them) and normals under the records' similarities, in fp64."""
    out = []
    for ob, sim in zip(objects, sims64(rec)):
        v32 = np.asarray(ob["vertices"], np.float64).astype(np.float32).astype(np.float64)
        moved = dict(ob, vertices=pt.apply_similarity(sim, v32))
        if ob.get("normals") is not None:
            moved["normals"] = pt.apply_similarity(sim, np.asarray(ob["normals"], np.float64), vectors=True)
        out.append(moved)
    return out


def nodes_of(bvh):
    """-> (boxes [n,2,2,3] = node, slot, lo / hi; child [n,2]; count [n,2]) of a BVH dict."""
    raw = np.frombuffer(bvh["nodes"].tobytes(), np.float32).reshape(-1, 16)
    ints = raw[:, 12:].copy().view(np.int32)
    return raw[:, :12].reshape(-1, 2, 2, 3).copy(), ints[:, :2], ints[:, 2:]


def records_of(bvh):
    """-> (corners [T,3,3] float64: v0, v0 + e1, v0 + e2 of every stored triangle in leaf order; ids [T])."""
    tf = np.frombuffer(bvh["tris"].tobytes(), np.float32).reshape(-1, 3, 4)
    v0, e1, e2 = (tf[:, k, :3].astype(np.float64) for k in range(3))
    return np.stack([v0, v0 + e1, v0 + e2], 1), tf[:, 0, 3].copy().view(np.int32)


def check_layout(pt, g, n_scene, n_tri):
    """The grafted layout's invariants -> (the deepest slot level, the scene's node indices, the object nodes' indices)."""
    boxes, child, count = nodes_of(g)
    n, first = g["n_nodes"], g["first_object_node"]
    assert boxes.shape[0] == n and first + g["n_object_nodes"] == n
    _, ids = records_of(g)
    assert sorted(ids[:n_scene].tolist()) == list(range(n_scene)) and sorted(ids[n_scene:].tolist()) == list(range(n_scene, n_tri))
    seen, deepest, sides = np.zeros(n_tri, int), 0, {0: [], 1: []}
    level_of = {}
    for side in (0, 1):
        lo, hi = (0, n_scene) if side == 0 else (n_scene, n_tri)
        small = hi - lo <= 4
        assert (count[0, side] >= 0) == small, "a side of 4 triangles or fewer is the slot's leaf"
        if small:
            assert (child[0, side], count[0, side]) == (lo, hi - lo)
            seen[lo:hi] += 1
            deepest = max(deepest, 1)
            continue
        assert child[0, side] == (1 if side == 0 else first)
        stack = [(int(child[0, side]), 1)]
        while stack:
            q, level = stack.pop()
            sides[side].append(q)
            level_of[q] = level
            assert (1 <= q < first) if side == 0 else (first <= q < n)
            for s in (0, 1):
                deepest = max(deepest, level + 1)
                if count[q, s] < 0:
                    assert child[q, s] > q, "a child lies behind its parent"
                    stack.append((int(child[q, s]), level + 1))
                else:
                    b, c = int(child[q, s]), int(count[q, s])
                    assert lo <= b and b + c <= hi and c >= 1
                    seen[b:b + c] += 1
    assert np.all(seen == 1), "every triangle in exactly one leaf"
    assert deepest == g["depth"] <= pt.MAX_BVH_DEPTH
    assert sorted(sides[0]) == list(range(1, first)) and sorted(sides[1]) == list(range(first, n))
    assert [level_of[q] for q in range(first, n)] == g["node_level"].tolist()
    return deepest, sides[0], sides[1]
