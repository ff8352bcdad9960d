"""Host side of the path-traced re-render (libmatpbr_path.so): the BVH builder's invariants, the closest-hit
routine the kernel runs (on the CPU) against a numpy brute-force search over every triangle, and the envmap's sampling tables.
No GPU needed."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import path_testlib as tl  # noqa: E402


@pytest.fixture(scope="module")
def path_lib():
    return tl.load()


def step_depth(H=40, W=48):
    """A tilted plane with a depth step across its middle rows and a hole: the mesher closes the gap at the step."""
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = 2.0 + 0.01 * j + 0.004 * i
    d[H // 2:, :] += 0.6
    d[3:6, 30:34] = 0.0
    return d.astype(np.float32)


@pytest.fixture(scope="module")
def mesh_and_bvh(path_lib):
    from materialist_amd import mesh

    rm = mesh.reference_mesh(step_depth())
    H, W = step_depth().shape
    assert rm["triangles"].shape[0] > 2 * (H - 2) * (W - 2), "expected gap-closing triangles at the depth step"
    return rm["vertices"], rm["triangles"], path_lib.build_bvh(rm["vertices"], rm["triangles"])


def _nodes(bvh):
    raw = bvh["nodes"].view(np.uint8)
    f = raw.view(np.float32).reshape(-1, 16)
    i = raw.view(np.int32).reshape(-1, 16)
    return f[:, :12].reshape(-1, 2, 6), i[:, 12:14], i[:, 14:16]


def _tris(bvh):
    f = bvh["tris"].view(np.float32).reshape(-1, 3, 4)
    return f, bvh["tris"].view(np.int32).reshape(-1, 12)[:, 3]


def test_bvh_covers_every_triangle_once_and_nests_its_boxes(mesh_and_bvh, path_lib):
    V, T, bvh = mesh_and_bvh
    boxes, child, count = _nodes(bvh)
    tf, ids = _tris(bvh)
    assert boxes.shape[0] == bvh["n_nodes"]
    seen = np.zeros(T.shape[0], np.int64)
    max_level = 0
    stack = [(0, 0)]
    while stack:
        node, level = stack.pop()
        max_level = max(max_level, level)
        for s in range(2):
            lo, hi = boxes[node, s, :3], boxes[node, s, 3:]
            if count[node, s] < 0:
                c = int(child[node, s])
                assert 0 < c < bvh["n_nodes"]
                # every child box of the inner node c lies inside the box its parent stores for it
                for s2 in range(2):
                    if count[c, s2] == 0:
                        continue
                    assert np.all(boxes[c, s2, :3] >= lo) and np.all(boxes[c, s2, 3:] <= hi), (node, s, c, s2)
                stack.append((c, level + 1))
            else:
                b, n = int(child[node, s]), int(count[node, s])
                max_level = max(max_level, level + 1)
                for k in range(b, b + n):
                    seen[ids[k]] += 1
                    v = np.stack([tf[k, 0, :3], tf[k, 0, :3] + tf[k, 1, :3], tf[k, 0, :3] + tf[k, 2, :3]])
                    assert np.all(v >= lo - 1e-6) and np.all(v <= hi + 1e-6), (node, s, k)
    assert np.all(seen == 1), "every triangle in exactly one leaf"
    assert max_level == bvh["depth"] <= path_lib.MAX_BVH_DEPTH, (max_level, bvh["depth"])
    # the stored triangles are the mesh's, with e1 x e2 facing the camera at the origin
    P = V[T[ids]]
    np.testing.assert_allclose(tf[:, 0, :3], P[:, 0], rtol=1e-6, atol=1e-6)
    nrm = np.cross(tf[:, 1, :3].astype(np.float64), tf[:, 2, :3].astype(np.float64))
    assert np.all((nrm * P[:, 0]).sum(-1) <= 1e-12)


def test_bvh_of_a_single_triangle_and_of_a_deep_degenerate_mesh(path_lib):
    V = np.array([[0, 0, -1], [1, 0, -1], [0, 1, -1]], np.float64)
    bvh = path_lib.build_bvh(V, np.array([[0, 1, 2]], np.int32))
    t, k = path_lib.trace_host(bvh, np.zeros((2, 3)), np.array([[0.2, 0.2, -1.0], [-0.2, 0.2, -1.0]]))
    assert k.tolist() == [0, -1]
    assert t[0] == pytest.approx(1.0, rel=1e-6)
    # 5000 triangles with one and the same centroid: no SAH plane exists, the builder splits by count and bounds the depth
    Vd = np.concatenate([V] * 5000)
    bvh = path_lib.build_bvh(Vd, np.arange(3 * 5000, dtype=np.int32).reshape(-1, 3))
    assert bvh["depth"] <= path_lib.MAX_BVH_DEPTH
    t, k = path_lib.trace_host(bvh, np.zeros((1, 3)), np.array([[0.2, 0.2, -1.0]]))
    assert 0 <= k[0] < 5000 and t[0] == pytest.approx(1.0, rel=1e-6)


def brute_force(P, o, d, tmin=0.0):
    """fp64 Moller-Trumbore of every ray against every triangle P[T,3,3] -> (t, index, smallest barycentric margin of the hit)."""
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    t_out = np.full(o.shape[0], np.inf)
    k_out = np.full(o.shape[0], -1, np.int64)
    margin = np.full(o.shape[0], np.inf)
    for r0 in range(0, o.shape[0], 256):
        oo, dd = o[r0:r0 + 256, None, :], d[r0:r0 + 256, None, :]
        pv = np.cross(dd, e2[None])
        det = (e1[None] * pv).sum(-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            idet = 1.0 / det
            tv = oo - P[None, :, 0]
            u = (tv * pv).sum(-1) * idet
            qv = np.cross(tv, e1[None])
            v = (dd * qv).sum(-1) * idet
            t = (e2[None] * qv).sum(-1) * idet
        ok = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > tmin)
        t = np.where(ok, t, np.inf)
        k = t.argmin(1)
        rows = np.arange(k.shape[0])
        t_out[r0:r0 + 256] = t[rows, k]
        k_out[r0:r0 + 256] = np.where(np.isfinite(t[rows, k]), k, -1)
        margin[r0:r0 + 256] = np.minimum(np.minimum(u, v), 1 - u - v)[rows, k]
    return t_out, k_out, margin


def test_host_closest_hit_matches_brute_force(mesh_and_bvh, path_lib):
    V, T, bvh = mesh_and_bvh
    H, W = step_depth().shape
    rng = np.random.default_rng(7)
    P = V[T].astype(np.float32).astype(np.float64)          # the fp32 geometry the BVH holds
    # camera rays through jittered pixel positions (the render's rays; exact pixel centres pass through vertices)
    f = (W / 2.0) / math.tan(math.radians(35.0) / 2.0)
    x = rng.uniform(-0.5, W - 0.5, 4000)
    y = rng.uniform(-0.5, H - 0.5, 4000)
    dc = np.stack([(x - (W - 1) / 2) / f, -(y - (H - 1) / 2) / f, -np.ones_like(x)], -1)
    dc /= np.linalg.norm(dc, axis=-1, keepdims=True)
    oc = np.zeros_like(dc)
    # 10 k random rays leaving points on the surface (offset along the face normal, as the render spawns them)
    ks = rng.integers(0, T.shape[0], 10000)
    b = rng.dirichlet([1, 1, 1], 10000)
    p = (P[ks] * b[:, :, None]).sum(1)
    nrm = np.cross(P[ks, 1] - P[ks, 0], P[ks, 2] - P[ks, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=-1, keepdims=True), 1e-30)
    nrm *= np.where((nrm * P[ks, 0]).sum(-1, keepdims=True) > 0, -1.0, 1.0)
    ds = rng.normal(size=(10000, 3))
    ds /= np.linalg.norm(ds, axis=-1, keepdims=True)
    os_ = p + 1e-5 * (1 + np.abs(p).max(-1, keepdims=True)) * np.where((ds * nrm).sum(-1, keepdims=True) > 0, 1.0, -1.0) * nrm
    o = np.concatenate([oc, os_]).astype(np.float32)
    d = np.concatenate([dc, ds]).astype(np.float32)
    t_h, k_h = path_lib.trace_host(bvh, o, d)
    t_b, k_b, margin = brute_force(P, o.astype(np.float64), d.astype(np.float64))
    hit_h = _agrees_with_brute_force(P, o, d, t_h, k_h, t_b, k_b, margin)
    assert hit_h[:4000].mean() > 0.9 and 0.05 < hit_h[4000:].mean() < 0.95


def _agrees_with_brute_force(P, o, d, t_h, k_h, t_b, k_b, margin):
    """trace_host's (t_h, k_h) against the fp64 brute force's (t_b, k_b, margin) of the same rays; -> which rays trace_host hit."""
    hit_h, hit_b = k_h >= 0, k_b >= 0
    near_edge = margin < 1e-5
    # the same misses, except rays that graze an edge within fp32 rounding
    bad_miss = (hit_h != hit_b) & ~near_edge
    assert not bad_miss.any(), np.nonzero(bad_miss)[0][:10]
    both = hit_h & hit_b
    # t to 1e-5 relative; for the short rays between nearby surfaces relative to the coordinates' magnitude, because fp32
    # Moller-Trumbore errs by a few ulp of the coordinates, not of t
    scale = np.maximum(t_b[both], np.abs(o[both]).max(-1))
    assert np.all(np.abs(t_h[both] - t_b[both]) <= 1e-5 * scale), np.abs(t_h[both] - t_b[both]).max()
    # the same triangle, except exact ties (a shared edge or vertex: the other triangle is hit at the same t)
    diff = both & (k_h != k_b)
    tie = np.zeros_like(diff)
    if diff.any():
        _, _, m_h = brute_force(P[k_h[diff]][:, None].reshape(-1, 3, 3), o[diff].astype(np.float64), d[diff].astype(np.float64))
        tie[diff] = (np.abs(t_h[diff] - t_b[diff]) <= 1e-5 * t_b[diff]) & (near_edge[diff] | (m_h < 1e-5))
    assert not (diff & ~tie).any(), np.nonzero(diff & ~tie)[0][:10]
    return hit_h


# ---- real size: the indoor2 mesh (512 x 512 depth, 522 k triangles) ------------------------------------------------------------
@pytest.fixture(scope="module")
def indoor2_bvh(path_lib, golden_dir):
    from materialist_amd import mesh

    depth = np.load(os.path.join(golden_dir, "indoor2.npz"))["depth_pred_f32"]
    depth = 2 * depth.max() - depth                                                  # inverse_img_w_mi.py:722
    rm = mesh.reference_mesh(depth, 35.0)
    return rm["vertices"], rm["triangles"], path_lib.build_bvh(rm["vertices"], rm["triangles"]), depth.shape


def test_indoor2_bvh_covers_every_triangle_once_and_nests_its_boxes(indoor2_bvh, path_lib):
    """The invariants of test_bvh_covers_every_triangle_once_and_nests_its_boxes, vectorised, on a mesh of the pipeline's size."""
    V, T, bvh, _ = indoor2_bvh
    boxes, child, count = _nodes(bvh)
    tf, ids = _tris(bvh)
    n = bvh["n_nodes"]
    assert boxes.shape[0] == n and T.shape[0] > 500000
    inner = count < 0
    # a tree: every node but the root is the child of exactly one inner slot
    c = child[inner]
    assert np.all((c > 0) & (c < n))
    assert np.array_equal(np.bincount(c, minlength=n), np.r_[0, np.ones(n - 1, np.int64)])
    # every child box of an inner node lies inside the box its parent stores for it
    parent_box = boxes[inner]                                      # [n-1, 6]
    for s2 in range(2):
        used = count[c, s2] != 0
        kid = boxes[c, s2]
        assert np.all(kid[used, :3] >= parent_box[used, :3]) and np.all(kid[used, 3:] <= parent_box[used, 3:]), s2
    # every triangle in exactly one leaf, inside its leaf's box
    leaf = ~inner
    b, cnt = child[leaf].astype(np.int64), count[leaf].astype(np.int64)
    k = np.repeat(b - np.cumsum(cnt) + cnt, cnt) + np.arange(cnt.sum())
    assert np.array_equal(np.bincount(ids[k], minlength=T.shape[0]), np.ones(T.shape[0], np.int64)), "every triangle in exactly one leaf"
    lb = np.repeat(boxes[leaf], cnt, axis=0)
    v = np.stack([tf[k, 0, :3], tf[k, 0, :3] + tf[k, 1, :3], tf[k, 0, :3] + tf[k, 2, :3]], 1)
    assert np.all(v >= lb[:, None, :3] - 1e-6) and np.all(v <= lb[:, None, 3:] + 1e-6)
    # depth: the deepest slot's level, as the builder reports it, within the stack the kernel has
    level, frontier, max_level = np.zeros(n, np.int64), np.array([0]), 0
    while frontier.size:
        max_level = max(max_level, int(level[frontier[0]]) + 1)
        kids = child[frontier][inner[frontier]]
        level[kids] = level[frontier[0]] + 1
        frontier = kids
    assert max_level == bvh["depth"] <= path_lib.MAX_BVH_DEPTH, (max_level, bvh["depth"])
    P = V[T[ids]]
    np.testing.assert_allclose(tf[:, 0, :3], P[:, 0], rtol=1e-6, atol=1e-6)
    nrm = np.cross(tf[:, 1, :3].astype(np.float64), tf[:, 2, :3].astype(np.float64))
    assert np.all((nrm * P[:, 0]).sum(-1) <= 1e-12)


def test_indoor2_host_closest_hit_matches_brute_force(indoor2_bvh, path_lib):
    """trace_host on 128 rays against a float64 brute force over all 522 k triangles (tests/path_fp64.TorchBrute, no BVH): camera
    rays, rays spawned from the surface as the render spawns them, and rays that graze the surface they leave."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import path_fp64 as pf

    V, T, bvh, (H, W) = indoor2_bvh
    rng = np.random.default_rng(17)
    P = V[T].astype(np.float32).astype(np.float64)
    f = (W / 2.0) / math.tan(math.radians(35.0) / 2.0)
    x, y = rng.uniform(-0.5, W - 0.5, 48), rng.uniform(-0.5, H - 0.5, 48)
    dc = np.stack([(x - (W - 1) / 2) / f, -(y - (H - 1) / 2) / f, -np.ones_like(x)], -1)
    dc /= np.linalg.norm(dc, axis=-1, keepdims=True)
    ks = rng.integers(0, T.shape[0], 80)
    p = (P[ks] * rng.dirichlet([1, 1, 1], 80)[:, :, None]).sum(1)
    nrm = np.cross(P[ks, 1] - P[ks, 0], P[ks, 2] - P[ks, 0])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=-1, keepdims=True), 1e-30)
    nrm *= np.where((nrm * P[ks, 0]).sum(-1, keepdims=True) > 0, -1.0, 1.0)
    ds = rng.normal(size=(80, 3))
    # the last 32: grazing, a tangent of the surface tipped 0.06 to 3 degrees to its front side
    tan = ds[48:] - (ds[48:] * nrm[48:]).sum(-1, keepdims=True) * nrm[48:]
    tan /= np.linalg.norm(tan, axis=-1, keepdims=True)
    ds[48:] = tan + np.tan(np.radians(rng.uniform(0.06, 3.0, 32)))[:, None] * nrm[48:]
    ds /= np.linalg.norm(ds, axis=-1, keepdims=True)
    os_ = p + 1e-5 * (1 + np.abs(p).max(-1, keepdims=True)) * np.where((ds * nrm).sum(-1, keepdims=True) > 0, 1.0, -1.0) * nrm
    o = np.concatenate([np.zeros_like(dc), os_]).astype(np.float32)
    d = np.concatenate([dc, ds]).astype(np.float32)
    t_h, k_h = path_lib.trace_host(bvh, o, d)
    t_b, k_b, margin = pf.TorchBrute(P).hits(o.astype(np.float64), d.astype(np.float64))
    hit_h = _agrees_with_brute_force(P, o, d, t_h, k_h, t_b, k_b, margin)
    assert hit_h[:48].mean() > 0.9 and 0.05 < hit_h[48:].mean() < 0.95


def test_envmap_tables_integrate_to_one_and_sample_by_luminance(path_lib):
    from materialist_amd import sh

    rng = np.random.default_rng(3)
    env = rng.gamma(1.0, 1.0, (16, 32, 3)).astype(np.float32)
    env[2, 5] = 40.0
    tab = path_lib.env_tables(env)
    omega = sh.envmap_solid_angles(16, 32)
    assert abs(float((tab["pdf"].astype(np.float64) * omega).sum()) - 1.0) < 1e-6
    lum = env.astype(np.float64) @ np.array([0.2126, 0.7152, 0.0722])
    np.testing.assert_allclose(tab["pdf"], lum / (lum * omega).sum(), rtol=1e-6)
    assert tab["row_cdf"][0] == 0 and tab["row_cdf"][-1] == 1 and np.all(np.diff(tab["row_cdf"]) >= 0)
    assert np.all(tab["col_cdf"][:, 0] == 0) and np.all(tab["col_cdf"][:, -1] == 1)
    # sampled directions lie in the texel they report, with that texel's pdf; texel frequencies follow pdf x solid angle
    u = rng.random((200000, 4)).astype(np.float32)
    d, p, k = path_lib.env_sample_host(tab, u)
    np.testing.assert_allclose(np.linalg.norm(d, axis=-1), 1.0, atol=1e-5)
    np.testing.assert_array_equal(p, tab["pdf"].reshape(-1)[k])
    th = np.arccos(np.clip(d[:, 1], -1, 1))
    ph = np.mod(np.arctan2(d[:, 0], -d[:, 2]), 2 * np.pi)
    row, col = np.minimum((th / np.pi * 16).astype(int), 15), np.minimum((ph / (2 * np.pi) * 32).astype(int), 31)
    assert np.mean(row * 32 + col == k) > 0.999
    freq = np.bincount(k, minlength=512) / k.shape[0]
    expect = (tab["pdf"] * omega).reshape(-1)
    assert np.abs(freq - expect).max() < 5 * np.sqrt(expect.max() / k.shape[0])


def test_envmap_tables_of_a_single_texel(path_lib):
    env = np.zeros((8, 16, 3), np.float32)
    env[5, 11] = [0.0, 2.0, 1.0]
    tab = path_lib.env_tables(env)
    u = np.random.default_rng(0).random((20000, 4)).astype(np.float32)
    u[:4] = [[0, 0, 0, 0], [0.9999999, 0.9999999, 0.9999999, 0.9999999], [0, 0.9999999, 0.5, 0.5], [0.9999999, 0, 0.5, 0.5]]
    _, p, k = path_lib.env_sample_host(tab, u)
    assert np.all(k == 5 * 16 + 11)
    from materialist_amd import sh

    assert p[0] == pytest.approx(1.0 / sh.envmap_solid_angles(8, 16)[5, 11], rel=1e-6)
    # a 1 x 1 envmap: the whole sphere is one cell of density 1/(4 pi)
    tab1 = path_lib.env_tables(np.full((1, 1, 3), 0.5, np.float32))
    d1, p1, k1 = path_lib.env_sample_host(tab1, u)
    assert np.all(k1 == 0) and np.allclose(p1, 1 / (4 * np.pi), rtol=1e-6)
    assert abs(float(d1[:, 1].mean())) < 0.03     # uniform in cos theta
    # an envmap without light has no emitter sampling
    tab0 = path_lib.env_tables(np.zeros((4, 8, 3), np.float32))
    assert tab0["total"] == 0 and tab0["row_cdf"][-1] == 0
    assert np.all(path_lib.env_sample_host(tab0, u[:8])[2] == -1)
