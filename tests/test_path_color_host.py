"""Host side of vertex-coloured inserted objects ("Vertex-coloured inserted objects"): the colour routine the
kernel runs (on the CPU) against fp64, the colour guide's CPU twin against the restatement's first hit, the fp64 restatement
`path_color_fp64` against a closed form in expectation, against `path_rough_fp64` with uniform colours and over the library's fp32
traversal, the PLY reader, the tables, the scene file, the refusals of every entry and the routing.  No GPU needed."""
import ctypes
import json
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import path_color_fp64 as pc  # noqa: E402
import path_fp64 as pf  # noqa: E402
import path_light_fp64 as pl  # noqa: E402
import path_objects_fp64 as pob  # noqa: E402
import path_oi_fp64 as po  # noqa: E402
import path_oi_pbr_fp64 as pp  # noqa: E402
import path_oi_smooth_fp64 as ps  # noqa: E402
import path_rough_fp64 as pr  # noqa: E402
import path_testlib as tl  # noqa: E402

FOV = pf.FOV
SEEDS = list(range(100, 164))      # the 64 fixed seeds of the scene in expectation
UV_TOL = 1e-5                      # tests/test_path_oi_smooth_host.py's bound on u and v, on lanes of its conditioning
C_TOL = 2 * UV_TOL + 2.0 ** -22    # |c1 - c0| <= 1 and |c2 - c0| <= 1: u's and v's error, plus the roundings of three fp32 operations on values <= 1
NEW = {"matpbr_path_render_objects_colors", "matpbr_path_object_color_host", "matpbr_path_feature_colors", "matpbr_path_feature_colors_host"}


@pytest.fixture(scope="module")
def path_lib():
    return tl.load()


_report = tl.reporter("path color", "test_path_color_host")


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


# ---- 0: the symbols ----------------------------------------------------------------------------------------------------------------------
def test_symbols(path_lib):
    with open(os.path.join(ROOT, "include", "matpbr_path.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(matpbr_path_\w+)\s*\(", text))
    assert NEW <= declared and set(path_lib.COLOR_SYMBOLS) == NEW and NEW <= set(path_lib.LATE_SYMBOLS)
    lib = path_lib.load()
    for name in NEW:
        fn = path_lib.symbol(name, lib)
        assert fn.argtypes == path_lib.SIGNATURES[name][1] and fn.restype == path_lib.SIGNATURES[name][0], name
    assert lib.matpbr_path_version() == 3 == path_lib.VERSION
    assert "#define MATPBR_PATH_OBJECT_COLORED 0x200" in text and path_lib.OBJECT_COLORED == 0x200
    assert ctypes.sizeof(path_lib.PathObject) == 24
    assert path_lib.SIGNATURES["matpbr_path_render_objects_colors"][1] == path_lib.SIGNATURES["matpbr_path_render_objects_rough"][1] + [ctypes.c_void_p]
    assert path_lib.OBJECT_ENTRIES["matpbr_path_render_objects_colors"] == 9 and path_lib.OBJECT_ENTRIES["matpbr_path_render_objects_rough"] == 8

    class Old:
        pass

    for name in NEW:
        with pytest.raises(path_lib.PathError, match=name):
            path_lib.symbol(name, Old())


# ---- 1: the colour routine -------------------------------------------------------------------------------------------------------------------
def _hits(N, rng):
    """`tests/test_path_oi_smooth_host.py`'s conditioning (unit-order edges at 40-140 degrees, rays at least 0.2 in cosine off the plane)
    with hit points inside, on the three edges (u = 0, v = 0, u + v = 1) and at the three corners -> fp32 tri, o, d."""
    v0 = rng.uniform(-1, 1, (N, 3))
    e1 = _unit(rng.normal(size=(N, 3)))
    t = _unit(np.cross(e1, rng.normal(size=(N, 3))))
    ang = np.radians(rng.uniform(40, 140, N))
    e2 = (np.cos(ang)[:, None] * e1 + np.sin(ang)[:, None] * t) * rng.uniform(0.5, 1.5, (N, 1))
    e1 = e1 * rng.uniform(0.5, 1.5, (N, 1))
    bu = rng.uniform(0.0, 1.0, N)
    bv = rng.uniform(0.0, 1.0, N) * (1.0 - bu)
    where = np.arange(N) % 8                                       # 0-1 inside; 2: u = 0; 3: v = 0; 4: u + v = 1; 5-7: the corners
    bu = np.where(where == 2, 0.0, bu)
    bv = np.where(where == 3, 0.0, bv)
    bv = np.where(where == 4, 1.0 - bu, bv)
    bu = np.where(where == 5, 0.0, np.where(where == 6, 1.0, np.where(where == 7, 0.0, bu)))
    bv = np.where(where == 5, 0.0, np.where(where == 6, 0.0, np.where(where == 7, 1.0, bv)))
    p = v0 + bu[:, None] * e1 + bv[:, None] * e2
    ng = _unit(np.cross(e1, e2))
    d = _unit(rng.normal(size=(N, 3)))
    c = (d * ng).sum(-1)
    d = _unit(np.where((np.abs(c) < 0.2)[:, None], d + np.sign(c + 1e-30)[:, None] * 0.5 * ng, d))
    o = p - rng.uniform(0.5, 3.0, (N, 1)) * d
    return np.stack([v0, e1, e2], 1).astype(np.float32), o.astype(np.float32), d.astype(np.float32), where


def test_color_host_against_fp64(path_lib):
    """10240 hits, inside, on every edge and at every corner; corner colours random, equal, 0 and 1.  u, v within 1e-5 (the smooth
    normal's bound, on its conditioning); c within that bound summed over u and v plus 2^-22 (|c1 - c0| <= 1); equal corners give
    their colour exactly; every c lies in [0, 1]."""
    rng = np.random.default_rng(31)
    N = 10240
    tri, o, d, where = _hits(N, rng)
    col = rng.random((N, 3, 3)).astype(np.float32)
    kind = (np.arange(N) // 8) % 4                                 # 0: random; 1: equal corners; 2: corner values 0 and 1; 3: random
    col[kind == 1] = col[kind == 1][:, :1]
    col[kind == 2] = rng.integers(0, 2, (int((kind == 2).sum()), 3, 3)).astype(np.float32)
    u, v, c = path_lib.object_color_host(tri, col, o, d)
    t64 = tri.astype(np.float64)
    P = np.stack([t64[:, 0], t64[:, 0] + t64[:, 1], t64[:, 0] + t64[:, 2]], 1)
    eu, ev = ps.barycentrics(P, o.astype(np.float64), d.astype(np.float64))
    ec = pc.vertex_color(col.astype(np.float64), eu, ev)
    worst_uv = max(float(np.abs(u - eu).max()), float(np.abs(v - ev).max()))
    worst_c = float(np.abs(c - ec).max())
    _report(f"colour routine vs fp64 on {N} hits: max abs error of u, v (bound {UV_TOL:.0e}) / of c (bound {C_TOL:.3e})", f"{worst_uv:.3e} / {worst_c:.3e}")
    assert worst_uv <= UV_TOL and worst_c <= C_TOL
    assert all((where == w).sum() >= N // 8 for w in range(8))
    eq = kind == 1
    assert eq.sum() >= 2000 and np.array_equal(c[eq].view(np.uint32), col[eq][:, 0].view(np.uint32))
    assert c.min() >= 0.0 and c.max() <= 1.0 and (c == 0.0).any() and (c == 1.0).any()
    # outside the triangle by rounding and beyond: the clamp holds, and a ray in the triangle's plane (u, v not numbers) gives a colour in [0, 1]
    far = o + np.float32(3.0) * tri[:, 1]
    assert np.all((path_lib.object_color_host(tri, col, far, d)[2] >= 0) & (path_lib.object_color_host(tri, col, far, d)[2] <= 1))
    flat = path_lib.object_color_host(tri[:4], col[:4], tri[:4, 0], tri[:4, 1])[2]
    assert np.all((flat >= 0) & (flat <= 1))


# ---- 2: the colour guide ---------------------------------------------------------------------------------------------------------------------
def _groove(H, W):
    from materialist_amd import mesh

    rm = mesh.reference_mesh(pf.groove_scene(H, W), FOV)
    rng = np.random.default_rng(11)
    a, r, m = pf.groove_maps(H, W, rng)
    return rm, a, r, m, pf.groove_env(rng)


def test_feature_colors_host_against_the_first_hit(path_lib):
    """`matpbr_path_feature_colors_host` on the table scene at 24 x 20: the interpolated colour of the restatement's first hit where
    the centre ray lands on a coloured object, exactly (1, 1, 1) everywhere else.  Bound 1e-4: on an icosphere triangle of edge
    e = 0.05 at distance D = 1.1, u and v carry fp32 roundings of D / e = 22 times 2^-24 over a few dozen operations, about 4e-5 each."""
    H, W = 20, 24
    objects = pc.table_scene()
    rm = _groove(H, W)[0]
    V, T, table = pob.merged(rm["vertices"], rm["triangles"], objects)
    Vm, Tm, tb, tint = path_lib.merge_objects(rm["vertices"], rm["triangles"], objects, colors=True)
    n_scene = rm["triangles"].shape[0]
    assert [t.kind for t in tb] == [0x302, 0x203, 2, 0x101] and tint.shape == (Tm.shape[0] - n_scene, 3, 3) and tint.dtype == np.float32
    got = path_lib.feature_colors_host(path_lib.build_bvh(Vm, Tm, n_scene), H, W, FOV, tb, tint, n_scene)
    f = (W / 2.0) / math.tan(math.radians(FOV) / 2.0)
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = _unit(np.stack([(j - (W - 1) / 2) / f, -(i - (H - 1) / 2) / f, -np.ones((H, W))], -1).reshape(-1, 3))
    o = np.zeros_like(d)
    P = V[T]
    t, k = pf.brute(P, o, d)
    ref = np.ones((H * W, 3))
    colored = np.zeros(T.shape[0], bool)
    cc = np.ones((T.shape[0], 3, 3))
    for e in table[:2]:
        sl = slice(e["first_tri"], e["first_tri"] + e["n_tri"])
        colored[sl], cc[sl] = True, e["corner_colors"]
    on = (k >= 0) & colored[np.maximum(k, 0)]
    bu, bv = ps.barycentrics(P[k[on]], o[on], d[on])
    ref[on] = pc.vertex_color(cc[k[on]], bu, bv)
    ref = ref.reshape(H, W, 3)
    on = on.reshape(H, W)
    per_object = [int((on & (k.reshape(H, W) >= e["first_tri"]) & (k.reshape(H, W) < e["first_tri"] + e["n_tri"])).sum()) for e in table[:2]]
    worst = float(np.abs(got - ref)[on].max())
    _report(f"colour guide vs the first hit: pixels on the coloured sphere / cube {per_object}, max abs error (bound 1e-4)", f"{worst:.3e}")
    assert min(per_object) >= 4 and worst <= 1e-4
    assert np.all(got[~on] == 1.0) and float(got[on].std()) > 0.05
    # a table without a coloured object: (1, 1, 1) everywhere, obj_col may be None
    Vu, Tu, tbu, none = path_lib.merge_objects(rm["vertices"], rm["triangles"], pc.table_scene(flagged=False), colors=True)
    assert none is None
    assert np.all(path_lib.feature_colors_host(path_lib.build_bvh(Vu, Tu, n_scene), H, W, FOV, tbu, None, n_scene) == 1.0)


# ---- 3: the restatement against a closed form --------------------------------------------------------------------------------------------------
def test_restatement_affine_colours_in_a_furnace(path_lib):
    """`path_light_fp64.furnace_scene`'s emitting box around a diffuse cube whose camera-facing face is perpendicular to the view axis
    and whose corner colours are an affine function of world position, max_depth 2: on that face the map from pixel to surface is
    affine, so the box-filtered pixel is L p (.) rho(hit of the centre ray).  64 seeds x spp 16 at 12 x 10, 5 standard errors + 1e-3."""
    H, W = 10, 12
    objects = pc.furnace_scene()
    expected, covered = furnace_expected(objects, H, W)
    assert covered.sum() >= 12                                     # a handful of pixels and more
    Vs, Ts = pp.FAR_TRIANGLE
    V, T, table = pob.merged(Vs, Ts, objects)
    env = np.zeros((4, 8, 3), np.float32)
    vals = pob.replay_mean(H, W, 16, SEEDS, 2, V, T, env, path_lib.env_tables(env), table)
    ok, excess = pl.within_five_sigma(vals, expected, covered)
    spread = float(expected[covered].max() - expected[covered].min())
    _report(f"affine colours in a furnace: worst |mean - L p rho| / (5 se + 1e-3) over {int(covered.sum())} pixels; the expectation's spread", f"{excess:.3f}; {spread:.3f}")
    assert ok and spread > 0.1                                     # the colour does vary across the covered pixels


def furnace_expected(objects, H, W):
    """-> (L p (.) rho at the centre ray's hit [H,W,3], the pixels whose footprint lies wholly on the cube's camera-facing face)."""
    cube = objects[1]
    inside, _ = tl.footprints([cube], H, W)
    f = (W / 2.0) / math.tan(math.radians(FOV) / 2.0)
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.stack([(j - (W - 1) / 2) / f, -(i - (H - 1) / 2) / f, -np.ones((H, W))], -1)
    z = cube["vertices"][:, 2].max()                               # the face towards the camera, perpendicular to the view axis
    hit = d * (z / -1.0)
    half = pc.FURNACE_CUBE[1] / 2
    on_face = (np.abs(hit[..., 0] - pc.FURNACE_CUBE[0][0]) < half) & (np.abs(hit[..., 1] - pc.FURNACE_CUBE[0][1]) < half)
    assert np.array_equal(inside, inside & on_face)                # from the origin only that face is seen
    return pl.FURNACE_L * np.asarray(pc.FURNACE_P) * pc.furnace_color(hit), inside


# ---- 4: uniform colours ------------------------------------------------------------------------------------------------------------------------
COLOUR_RECORD = ("colored_camera", "colored_indirect")             # what the record holds of the flags themselves, not of the paths


def test_uniform_colours_are_the_uncoloured_object(path_lib, oracle64):
    """With every corner (1, 1, 1) the restatement equals its render of the unflagged table bit for bit."""
    H, W = 20, 24
    rm, a, r, m, env = _groove(H, W)
    tab = path_lib.env_tables(env)
    V, T, flagged = pob.merged(rm["vertices"], rm["triangles"], pc.table_scene(uniform=True))
    _, _, plain = pob.merged(rm["vertices"], rm["triangles"], pc.table_scene(flagged=False))
    for max_depth, seed in ((2, 0), (6, 1), (16, 2)):
        got, rec = pob.replay_objects(oracle64, V, T, a, r, m, env, tab, H, W, max_depth, seed, flagged)
        ref, rec0 = pob.replay_objects(oracle64, V, T, a, r, m, env, tab, H, W, max_depth, seed, plain)
        assert np.array_equal(got, ref) and rec["colored_camera"][:, :2].any(0).all(), (max_depth, seed)
        assert all(np.array_equal(rec0[k], rec[k]) for k in rec0 if isinstance(rec0[k], np.ndarray) and k not in COLOUR_RECORD)
    # and the colours do something: the coloured table differs on the coloured objects' pixels
    _, _, coloured = pob.merged(rm["vertices"], rm["triangles"], pc.table_scene())
    tinted, rec = pob.replay_objects(oracle64, V, T, a, r, m, env, tab, H, W, 16, 2, coloured)
    on = rec["colored_camera"].any(-1).reshape(H, W)
    assert (np.abs(tinted - ref).max(-1)[on] > 0).mean() > 0.5


# ---- 5: traversal agreement --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_on", [True, False])
def test_restatement_over_fp32_and_fp64_traversal(path_lib, oracle64, env_on):
    """The GPU criterion's ground: over the library's fp32 traversal and over the fp64 brute force the restatement disagrees in NO pixel
    of the GPU test's renders (the groove at 24 x 20 with `path_color_fp64.table_scene`; max_depth 2, 6, 16; seeds 0-2; the envmap on
    and zero), and every render holds a camera hit on each coloured object and an indirect hit on one."""
    H, W = 20, 24
    objects = pc.table_scene()
    rm, a, r, m, env = _groove(H, W)
    if not env_on:
        env = np.zeros_like(env)
    V, T, table = pob.merged(rm["vertices"], rm["triangles"], objects)
    Vm, Tm, tb = path_lib.merge_objects(rm["vertices"], rm["triangles"], objects)
    bvh = path_lib.build_bvh(Vm, Tm, rm["triangles"].shape[0])

    def closest(o, d):
        t, k = path_lib.trace_host(bvh, o, d)
        return np.where(k < 0, np.inf, t.astype(np.float64)), k.astype(np.int64)

    tab = path_lib.env_tables(env)
    for max_depth in (2, 6, 16):
        for seed in (0, 1, 2):
            args = (oracle64, V, T, a, r, m, env, tab, H, W, max_depth, seed, table)
            L64, rec = pob.replay_objects(*args)
            L32, _ = pob.replay_objects(*args, closest=closest)
            assert rec["colored_camera"][:, 0].any() and rec["colored_camera"][:, 1].any() and rec["colored_indirect"].any(), (max_depth, seed)
            if not env_on:                                          # this table holds no light: without the envmap there is no emitter, the
                assert not L64.any() and not L32.any()              # criterion's denominator is 0 and both renders are black, exactly
                continue
            err = (np.abs(L32 - L64) / np.maximum(np.abs(L64), np.abs(L64).mean())).max(-1)
            assert int((err > 1e-3).sum()) == 0, (max_depth, seed, np.argwhere(err > 1e-3)[:10])


# ---- 6: the reader, the tables, the scene file, the refusals, the routing ----------------------------------------------------------------------
def _write_ply(path, V, T, C=None, fmt="ascii", ctype="uchar", names=("red", "green", "blue")):
    """A PLY as a modelling tool writes it: float x y z, optionally colours of `ctype` named `names`, uchar-counted int faces."""
    np_t = {"uchar": "u1", "ushort": "<u2", "float": "<f4", "double": "<f8"}[ctype]
    props = [("x", "float", "<f4"), ("y", "float", "<f4"), ("z", "float", "<f4")] + ([(n, ctype, np_t) for n in names] if C is not None else [])
    head = f"ply\nformat {fmt} 1.0\nelement vertex {len(V)}\n" + "".join(f"property {t} {n}\n" for n, t, _ in props)
    head += f"element face {len(T)}\nproperty list uchar int vertex_indices\nend_header\n"
    cols = [V[:, 0], V[:, 1], V[:, 2]] + ([C[:, 0], C[:, 1], C[:, 2]] if C is not None else [])
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii"))
        if fmt == "ascii":
            for row in zip(*cols):
                fh.write((" ".join(repr(float(x)) if isinstance(x, (float, np.floating)) else str(int(x)) for x in row) + "\n").encode())
            for t in T:
                fh.write(f"3 {t[0]} {t[1]} {t[2]}\n".encode())
        else:
            rec = np.empty(len(V), dtype=[(n, t) for n, _, t in props])
            for (n, _, _), c in zip(props, cols):
                rec[n] = c
            fh.write(rec.tobytes())
            faces = np.empty(len(T), dtype=[("n", "u1"), ("v", "<i4", (3,))])
            faces["n"], faces["v"] = 3, T
            fh.write(faces.tobytes())


def test_ply_reader_colours(tmp_path):
    from materialist_amd import mesh

    V, T = po.cube((0.0, 0.0, -1.0), 0.2, (0.1, 0.2, 0.3))
    V = V.astype(np.float32)
    rng = np.random.default_rng(3)
    C8 = rng.integers(0, 256, (8, 3))
    C8[0], C8[1] = 0, 255
    Cf = rng.random((8, 3)).astype(np.float32)
    for fmt in ("ascii", "binary_little_endian"):
        p = str(tmp_path / f"{fmt}.ply")
        _write_ply(p, V, T, C8, fmt, "uchar")
        Vr, Tr, C = mesh.read_ply_any(p, colors=True)
        assert np.array_equal(Vr, V.astype(np.float64)) and np.array_equal(Tr, T) and C.dtype == np.float64
        assert np.array_equal(C, C8 / 255.0) and C.min() == 0.0 and C.max() == 1.0
        Vr, Tr, Nn, C = mesh.read_ply_any(p, normals=True, colors=True)
        assert Nn is None and np.array_equal(C, C8 / 255.0)
        assert len(mesh.read_ply_any(p)) == 2 and len(mesh.read_ply_any(p, normals=True)) == 3      # the existing shapes
        _write_ply(p, V, T, Cf, fmt, "float", ("r", "g", "b"))
        assert np.array_equal(mesh.read_ply_any(p, colors=True)[2], Cf.astype(np.float64))         # float: as written
        _write_ply(p, V, T, C8 * 257, fmt, "ushort")
        assert np.array_equal(mesh.read_ply_any(p, colors=True)[2], C8 * 257 / 65535.0)
        _write_ply(p, V, T, None, fmt)
        assert mesh.read_ply_any(p, colors=True)[2] is None
    mesh.write_ply(str(tmp_path / "own.ply"), V, T)
    assert mesh.read_ply_any(str(tmp_path / "own.ply"), colors=True)[2] is None


def test_merge_objects_and_the_value_errors(path_lib):
    Vs, Ts = pp.FAR_TRIANGLE
    objects = pc.table_scene()
    V, T, table, corner, records, lt, tint = path_lib.merge_objects(Vs, Ts, objects, normals=True, pbr=True, lights=True, colors=True)
    assert [t.kind for t in table] == [0x302, 0x203, 2, 0x101] and lt is None and corner is not None
    assert tint.dtype == np.float32 and tint.shape == (T.shape[0] - 1, 3, 3)
    for k, ob in enumerate(objects):
        sl = slice(table[k].first_tri - 1, table[k].first_tri - 1 + table[k].n_tri)
        want = pc.corner_colors(ob)
        assert np.array_equal(tint[sl], want.astype(np.float32) if want is not None else np.zeros((table[k].n_tri, 3, 3), np.float32))
    assert tuple(records[1].a) == tuple(np.float32(pc.PBR_BASE["albedo"])) and tuple(table[0].p) == tuple(np.float32(pc.DIFFUSE_BASE["reflectance"]))
    # the existing return shapes: without colors= nothing follows, and a table without "colors" gives None
    assert len(path_lib.merge_objects(Vs, Ts, objects)) == 3 and len(path_lib.merge_objects(Vs, Ts, objects, normals=True, pbr=True, lights=True)) == 6
    assert path_lib.merge_objects(Vs, Ts, pc.table_scene(flagged=False), colors=True)[3] is None
    assert path_lib.object_bsdf(pc.PBR_BASE)[0] == 3 and path_lib.object_bsdf(pc.DIFFUSE_BASE)[0] == 2      # the BSDFs carry no flag: the object does
    Vc, Tc = po.cube((0.0, 0.0, -1.0), 0.2, (0.0, 0.0, 0.0))
    good = np.full((8, 3), 0.5)

    def merge(colors, bsdf=po.DIFFUSE_08):
        return path_lib.merge_objects(Vs, Ts, [{"vertices": Vc, "triangles": Tc, "bsdf": po.DIFFUSE_08},
                                               {"vertices": Vc + (0.5, 0, 0), "triangles": Tc, "bsdf": bsdf, "colors": colors}], colors=True)

    assert merge(good)[3].shape == (24, 3, 3) and not merge(good)[3][:12].any()
    for spoil, pattern in (((3, 1, np.nan), r"object 1.*vertex 3"), ((5, 0, 1.5), r"object 1.*vertex 5"), ((0, 2, -0.1), r"object 1.*vertex 0"),
                           ((7, 2, np.inf), r"object 1.*vertex 7")):
        bad = good.copy()
        bad[spoil[0], spoil[1]] = spoil[2]
        with pytest.raises(ValueError, match=pattern):
            merge(bad)
    with pytest.raises(ValueError, match=r"object 1.*\[Nv,3\]"):
        merge(good[:7])
    for bsdf in (po.GLASS, pl.QUAD_LIGHT, pr.FROSTED_02):
        with pytest.raises(ValueError, match=r"object 1.*(diffuse|pbr)"):
            merge(good, bsdf)
    # the entries from before the flag are handed tables without it: the light tables of a scene with a light and a coloured object
    Vq, Tq = pl.quad(pl.LIGHT_QUAD)
    lt = path_lib.merge_objects(Vs, Ts, [{"vertices": Vc, "triangles": Tc, "bsdf": po.DIFFUSE_08, "colors": good},
                                         {"vertices": Vq, "triangles": Tq, "bsdf": pl.QUAD_LIGHT}], pbr=True, lights=True)[4]
    assert lt["header"].n_lights == 1 and lt["header"].object[0] == 1


def test_refusals_of_every_entry(path_lib):
    """By return code: the new entries refuse what they cannot take, and every entry from before the flag refuses it as an unknown kind."""
    lib = path_lib.load()
    P_ = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    tab = lambda t: ctypes.cast(t, ctypes.c_void_p)
    raw = np.zeros(20, np.float32)
    one = raw[(-raw.ctypes.data % 16) // 4:][:12]
    one[2] = 1.0
    io = np.zeros(3, np.int32)
    C = path_lib.OBJECT_COLORED
    obj = lambda k, p=(0.5, 0.5, 0.5), first=1: (path_lib.PathObject * 1)(path_lib.PathObject(k, first, 12, (ctypes.c_float * 3)(*p)))
    rec = (path_lib.PathObjectPbr * 1)(path_lib.PathObjectPbr((ctypes.c_float * 3)(0.5, 0.5, 0.5), 0.5, 0.0))
    frame = [P_(one)] * 5 + [4, 4, 35.0] + [P_(one)] * 4 + [2, 4, 1, 4, 0, 1, P_(one), None, None]
    render = lib.matpbr_path_render_objects_colors
    # the flag on kinds 1, 4, 5 (with and without the smooth flag), a coloured object without obj_col, a range below n_scene_tri
    for k, p in ((1, (1.5, 1.0, 0.0)), (4, (1.0, 1.0, 1.0)), (5, (1.5, 1.0, 0.1)), (0x101, (1.5, 1.0, 0.0)), (0x105, (1.5, 1.0, 0.1)), (0, (0.5,) * 3), (6, (0.5,) * 3)):
        assert render(*frame, tab(obj(k | C, p)), 1, P_(one), 1, tab(rec), None, None, None, P_(one)) == -1, k
    for k in (2, 3, 0x102, 0x103):
        assert render(*frame, tab(obj(k | C)), 1, P_(one), 1, tab(rec), None, None, None, None) == -1, k       # obj_col == NULL
        assert render(*frame, tab(obj(k | C)), 1, P_(one), 2, tab(rec), None, None, None, P_(one)) == -1, k    # below n_scene_tri
    assert render(*frame, tab(obj(3 | C)), 1, None, 1, None, None, None, None, P_(one)) == -1                   # kind 3 without records
    assert render(*frame, tab(obj(0x102 | C)), 1, None, 1, None, None, None, None, P_(one)) == -1               # smooth without normals
    assert render(*frame, tab(obj(2 | C, (0.5, 1.5, 0.5))), 1, None, 1, None, None, None, None, P_(one)) == -1  # level 1's bounds hold
    assert render(*frame, tab(obj(5, (1.5, 1.0, 0.01))), 1, None, 1, None, None, None, None, None) == -1        # level 5's
    assert render(*frame, None, 1, None, 1, None, None, None, None, None) == -1
    # every entry from before the flag refuses it
    for k in (2 | C, 3 | C, 0x102 | C):
        t = tab(obj(k))
        assert lib.matpbr_path_render_objects(*frame, t, 1) == -1
        assert lib.matpbr_path_render_objects_normals(*frame, t, 1, P_(one), 1) == -1
        assert lib.matpbr_path_render_objects_pbr(*frame, t, 1, P_(one), 1, tab(rec)) == -1
        assert lib.matpbr_path_render_objects_lights(*frame, t, 1, P_(one), 1, tab(rec), None, None, None) == -1
        assert lib.matpbr_path_render_objects_rough(*frame, t, 1, P_(one), 1, tab(rec), None, None, None) == -1
        assert lib.matpbr_path_features(P_(one), P_(one), 4, 4, 35.0, t, 1, P_(one), 1, None, P_(one), None) == -1
        assert lib.matpbr_path_features_host(P_(one), P_(one), 4, 4, 35.0, t, 1, P_(one), 1, None, P_(one)) == -1
        assert lib.matpbr_path_object_lookup_host(t, 1, tab(rec), P_(io), 1, P_(io), P_(one), P_(one), P_(one)) == -1
        assert lib.matpbr_path_object_sample_host(t, P_(one), P_(one), P_(one), 1, P_(one), P_(one), P_(one), P_(io)) == -1
        head, n = path_lib.PathLights(), ctypes.c_long(0)
        assert lib.matpbr_path_light_tables(P_(np.zeros(9)), 3, P_(np.zeros(3, np.int32)), 1, t, 1, tab(rec), ctypes.cast(ctypes.byref(head), ctypes.c_void_p),
                                            None, None, 0, ctypes.cast(ctypes.byref(n), ctypes.c_void_p)) == -1
    # the colour routine and the guide
    host = lambda *a: lib.matpbr_path_object_color_host(*a)
    full = [P_(one), P_(one), P_(one), P_(one), 1, P_(one), P_(one), P_(one)]
    for k in (0, 1, 2, 3, 5, 6, 7):
        assert host(*(None if j == k else x for j, x in enumerate(full))) == -1, k
    assert host(*full[:4], -1, *full[5:]) == -1 and host(*full[:4], 0, *full[5:]) == 0
    for fn, tail in ((lib.matpbr_path_feature_colors, (None,)), (lib.matpbr_path_feature_colors_host, ())):
        ok = [P_(one), P_(one), 4, 4, 35.0, tab(obj(2 | C)), 1, 1, P_(one), P_(one)]
        for j, v in ((0, None), (1, None), (2, 0), (3, -1), (4, 0.0), (4, 180.0), (4, float("nan")), (5, None), (6, 9), (6, -1), (7, -1), (7, 2), (8, None),
                     (9, None), (5, tab(obj(1 | C, (1.5, 1.0, 0.0)))), (5, tab(obj(4 | C))), (5, tab(obj(5 | C, (1.5, 1.0, 0.1)))), (5, tab(obj(7)))):
            assert fn(*(v if i == j else x for i, x in enumerate(ok)), *tail) == -1, (fn.__name__, j, v)
    with pytest.raises(ValueError, match="same rows"):
        path_lib.object_color_host(np.zeros((2, 3, 3)), np.zeros((1, 3, 3)), np.zeros((2, 3)), np.zeros((2, 3)))
    assert "coloured object without corner colours" in lib.matpbr_path_strerror(-1).decode()


class _Host:
    """torch.from_numpy's result for a tracer built without a device: keeps the array, `.to()` returns itself."""

    def __init__(self, x):
        self.x = x

    def to(self, *a, **k):
        return self

    def data_ptr(self):
        return self.x.ctypes.data


def test_a_table_without_colours_leaves_every_route_alone(path_lib, monkeypatch):
    """`PathTracer` without a coloured object asks for no new symbol and holds no colour buffer; with one it asks for the new render
    entry and the guide, counts it, and `object_args()` grows a ninth value whose first eight are what they were."""
    asked = []
    real = path_lib.symbol
    monkeypatch.setattr(path_lib, "symbol", lambda name, lib=None: (asked.append(name), real(name, lib))[1])
    monkeypatch.setattr(path_lib.torch, "from_numpy", lambda x: _Host(x))
    Vs, Ts = pp.FAR_TRIANGLE
    for objects in (pr.table_scene(), pl.table_scene(), pp.table_scene(), ps.table_scene(), po.two_cubes(), pc.table_scene(flagged=False), None):
        del asked[:]
        tracer = path_lib.PathTracer(Vs, Ts, 4, 4, FOV, device="cpu", objects=objects)
        assert not NEW & set(asked) and tracer.obj_col is None and tracer.stats["n_colored_objects"] == 0
        args = tracer.object_args()
        assert len(args) == 9 and args[8] is None
    del asked[:]
    tracer = path_lib.PathTracer(Vs, Ts, 4, 4, FOV, device="cpu", objects=pc.table_scene())
    assert {"matpbr_path_render_objects_colors", "matpbr_path_feature_colors"} <= set(asked) and "matpbr_path_render_objects_rough" not in asked
    st = tracer.stats
    assert st["n_colored_objects"] == 2 and st["n_pbr_objects"] == 1 and st["n_smooth_objects"] == 2 and st["n_rough_objects"] == 0
    assert tracer.obj_col is not None and tracer.pbr is not None and tracer.object_args()[8] == tracer.obj_col.x.ctypes.data
    plain = path_lib.PathTracer(Vs, Ts, 4, 4, FOV, device="cpu", objects=pc.table_scene(flagged=False))
    assert [type(x) for x in plain.object_args()[:8]] == [type(x) for x in tracer.object_args()[:8]]
    with pytest.raises(ValueError, match="objects"):
        tracer.render_bwd(None, None, None, None, None)


def test_scene_file_command_line_and_guide(path_lib, tmp_path):
    import torch

    import render_final
    from materialist_amd import mesh, relight
    from materialist_amd.imageio_hdr import write_hdr

    a = render_final.parse_args(["--save_name", "case", "--mode", "oi", "--oi_colors", "vertex_linear"])
    assert a.oi_colors == "vertex_linear" and render_final.parse_args(["--save_name", "case", "--mode", "oi"]).oi_colors == "none"
    with pytest.raises(SystemExit):
        render_final.parse_args(["--save_name", "case", "--mode", "oi", "--oi_colors", "srgb"])
    Vc, Tc = po.cube((0.0, 0.0, -1.0), 0.2, (0.1, 0.2, 0.3))
    C8 = np.random.default_rng(4).integers(0, 256, (8, 3))
    os.makedirs(tmp_path / "lists")
    _write_ply(str(tmp_path / "lists" / "bowl.ply"), Vc.astype(np.float32), Tc, C8, "binary_little_endian")
    mesh.write_ply(str(tmp_path / "lists" / "grey.ply"), Vc, Tc)
    path = str(tmp_path / "lists" / "bowl.json")

    def write(objects):
        with open(path, "w") as f:
            json.dump({"objects": objects}, f)

    for colors in ("none", "vertex", "vertex_linear"):
        write([{"ply": "bowl.ply", "bsdf": pc.PBR_BASE, "colors": colors}, {"ply": "bowl.ply", "bsdf": po.DIFFUSE_08}])
        got = relight.load_oi_scene(path)
        assert [e["colors"] for e in got] == [colors, "none"] and got[0]["normals"] == "flat"
    write([{"ply": "bowl.ply", "bsdf": po.DIFFUSE_08, "colors": "srgb"}])
    with pytest.raises(ValueError, match=r"bowl.json: objects\[0\].*'colors' must be"):
        relight.load_oi_scene(path)
    for bsdf in (po.GLASS, pl.QUAD_LIGHT, pr.FROSTED_02):
        write([{"ply": "bowl.ply", "bsdf": bsdf, "colors": "vertex"}])
        with pytest.raises(ValueError, match=r"bowl.json: objects\[0\].*'colors' must be 'none'"):
            relight.load_oi_scene(path)
    # the decoding, and a file without colours
    C = C8 / 255.0
    assert np.array_equal(relight._object_colors("bowl.ply", C, "vertex_linear"), C)
    assert np.allclose(relight._object_colors("bowl.ply", C, "vertex"), C ** 2.2, rtol=0, atol=1e-15) and not np.array_equal(C ** 2.2, C)
    os.makedirs(tmp_path / "case" / "best_results")
    write_hdr(str(tmp_path / "case" / "best_results" / "envmap.hdr"), np.ones((4, 8, 3), np.float32))
    for colors in ("vertex", "vertex_linear"):
        write([{"ply": "grey.ply", "bsdf": po.DIFFUSE_08, "colors": colors}])
        with pytest.raises(ValueError, match=r"grey\.ply.*colours"):
            relight.render_oi("case", input_path=str(tmp_path), save_path=str(tmp_path), objects_file=path)
    mesh.write_ply(str(tmp_path / "case" / "oi2.ply"), Vc, Tc)
    with pytest.raises(ValueError, match=r"oi2\.ply.*colours"):
        relight.render_oi("case", input_path=str(tmp_path), save_path=str(tmp_path), object_colors="vertex")
    with pytest.raises(ValueError, match="object_colors"):
        relight.render_oi("case", input_path=str(tmp_path), save_path=str(tmp_path), object_colors="srgb")
    # the guide: a coloured object's constant times the colour feature; the call without it is what it was
    geom = torch.zeros(1, 3, 8)
    geom[..., 7] = torch.tensor([[1.0, 2.0, 0.0]])
    tint = torch.tensor([[[0.5, 0.25, 1.0], [0.5, 0.5, 0.5], [1.0, 1.0, 1.0]]])
    bsdfs = [pc.PBR_BASE, po.GLASS]
    plain = relight.albedo_guide(geom, torch.full((1, 3, 3), 0.25), bsdfs).numpy()
    guide = relight.albedo_guide(geom, torch.full((1, 3, 3), 0.25), bsdfs, tint).numpy()
    assert np.allclose(plain[0, 0], pc.PBR_BASE["albedo"]) and np.allclose(guide[0, 0], np.float32(pc.PBR_BASE["albedo"]) * np.float32([0.5, 0.25, 1.0]))
    assert np.all(guide[0, 1] == 1.0) and np.all(guide[0, 2] == 0.25) and np.array_equal(plain[0, 1:], guide[0, 1:])
