"""Host side of UV-textured inserted objects ("Textured inserted objects"): the coordinate and the fetch the
kernel runs (on the CPU) against fp64, the tint guide's CPU twin against the restatement's first hit, the fp64 restatement
`path_texture_fp64` against a closed form in expectation, against `path_color_fp64` with uniform images and over the library's fp32
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
import path_texture_fp64 as px  # noqa: E402

FOV = pf.FOV
SEEDS = list(range(100, 164))      # the 64 fixed seeds of the scene in expectation
UV_TOL = 1e-5                      # tests/test_path_oi_smooth_host.py's bound on u and v, on lanes of its conditioning
MARGIN = 4.0                       # the library may err 4 x the fp32 transcription's own error (tests/test_path_rough_host.py's margin)
NEW = {"matpbr_path_render_objects_textures", "matpbr_path_object_texture_host", "matpbr_path_feature_tints", "matpbr_path_feature_tints_host"}
SIZES = ((1, 1), (2, 3), (5, 4))   # w x h


@pytest.fixture(scope="module")
def path_lib():
    return tl.load()


_report = tl.reporter("path texture", "test_path_texture_host")


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _texels(*images):
    """Images [h,w,3] one after another as the library takes them -> ([n,4] float32, the first texel of each)."""
    first, rows = [], []
    for im in images:
        first.append(sum(r.shape[0] for r in rows))
        rows.append(np.concatenate([np.asarray(im, np.float32).reshape(-1, 3), np.zeros((im.shape[0] * im.shape[1], 1), np.float32)], -1))
    return np.concatenate(rows), first


def _record(path_lib, base=None, orm=None, first=(0, 0)):
    r = path_lib.PathObjectTex()
    if base is not None:
        r.base_first, r.base_w, r.base_h = first[0], base.shape[1], base.shape[0]
    if orm is not None:
        r.orm_first, r.orm_w, r.orm_h = first[1], orm.shape[1], orm.shape[0]
    return r


# ---- 0: the symbols ----------------------------------------------------------------------------------------------------------------------
def test_symbols(path_lib):
    with open(os.path.join(ROOT, "include", "matpbr_path.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(matpbr_path_\w+)\s*\(", text))
    assert NEW <= declared and set(path_lib.TEXTURE_SYMBOLS) == NEW and NEW <= set(path_lib.LATE_SYMBOLS)
    assert not NEW & set(path_lib.COLOR_SYMBOLS) and all(path_lib._FEATURE[n] == "textured inserted objects" for n in NEW)
    lib = path_lib.load()
    for name in NEW:
        fn = path_lib.symbol(name, lib)
        assert fn.argtypes == path_lib.SIGNATURES[name][1] and fn.restype == path_lib.SIGNATURES[name][0], name
    assert lib.matpbr_path_version() == 3 == path_lib.VERSION
    assert "#define MATPBR_PATH_OBJECT_TEXTURED 0x400" in text and path_lib.OBJECT_TEXTURED == 0x400
    assert ctypes.sizeof(path_lib.PathObjectTex) == 32 and ctypes.sizeof(path_lib.PathObject) == 24
    assert path_lib.SIGNATURES["matpbr_path_render_objects_textures"][1] == \
        path_lib.SIGNATURES["matpbr_path_render_objects_colors"][1] + [ctypes.c_void_p] * 3 + [ctypes.c_long]
    assert path_lib.OBJECT_ENTRIES["matpbr_path_render_objects_textures"] == 13 and path_lib.OBJECT_ENTRIES["matpbr_path_render_objects_colors"] == 9

    class Old:
        pass

    for name in NEW:
        with pytest.raises(path_lib.PathError, match=name):
            path_lib.symbol(name, Old())


# ---- (a): the coordinate and the fetch ------------------------------------------------------------------------------------------------------
def _hits(N, rng):
    """`tests/test_path_color_host.py`'s hits: unit-order edges at 40-140 degrees, rays at least 0.2 in cosine off the plane, hit points
    inside, on the three edges and at the three corners -> fp32 tri, o, d, where."""
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
    return np.stack([v0, e1, e2], 1).astype(np.float32), o.astype(np.float32), d.astype(np.float32), where, bu, bv


def _coordinates(N, rng, bu, bv, w, h):
    """Corner coordinates whose interpolation at (bu, bv) lands on a target (s, t) in [-2, 3]^2.  The targets, by lane: 0 random; 1 an
    exact texel centre; 2 an exact texel edge; 3 integers (the seam).  On every other lane of kinds 1-3 the three corners carry the
    target itself, so that the hit reads exactly that coordinate whatever u and v round to -> (uv [N,3,2] fp32, kind, constant)."""
    kind = (np.arange(N) // 8) % 4
    whole = rng.integers(-2, 3, (N, 2)).astype(np.float64)
    cell = np.stack([rng.integers(0, w, N), rng.integers(0, h, N)], -1)
    size = np.array([w, h], np.float64)
    target = rng.uniform(-2.0, 3.0, (N, 2))
    target = np.where((kind == 1)[:, None], whole + (cell + 0.5) / size, target)
    target = np.where((kind == 2)[:, None], whole + cell / size, target)
    target = np.where((kind == 3)[:, None], whole, target)
    d1, d2 = rng.uniform(-1.0, 1.0, (N, 2)), rng.uniform(-1.0, 1.0, (N, 2))
    constant = (kind > 0) & ((np.arange(N) // 32) % 2 == 0)
    d1[constant], d2[constant] = 0.0, 0.0
    st0 = target - bu[:, None] * d1 - bv[:, None] * d2
    return np.stack([st0, st0 + d1, st0 + d2], 1).astype(np.float32), kind, constant


def _tri_uv32(tri, o, d):
    """The library's tri_uv in numpy float32, each operation rounded once (no contraction)."""
    f = np.float32
    v0, e1, e2 = tri[:, 0].astype(f), tri[:, 1].astype(f), tri[:, 2].astype(f)
    dot = lambda a, b: (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]
    pv = np.cross(d, e2).astype(f)
    idet = f(1) / dot(e1, pv)
    tv = o - v0
    qv = np.cross(tv, e1).astype(f)
    return dot(tv, pv) * idet, dot(d, qv) * idet


def test_texture_host_against_fp64(path_lib):
    """10240 hits (inside, on every edge, at every corner) per pair of images of 1 x 1, 2 x 3 and 5 x 4 texels, coordinates in [-2, 3]
    with exact texel centres, exact texel edges and integers among them.  u, v within 1e-5.  base and orm within 4 x the error that a
    numpy-float32 transcription of the restatement makes against fp64 on the same lanes, no lane excluded (bilinear repeat is
    continuous); constant, all-0 and all-1 images are exact; every value lies in [0, 1]."""
    rng = np.random.default_rng(41)
    N = 10240
    tri, o, d, where, bu, bv = _hits(N, rng)
    t64 = tri.astype(np.float64)
    P = np.stack([t64[:, 0], t64[:, 0] + t64[:, 1], t64[:, 0] + t64[:, 2]], 1)
    eu, ev = ps.barycentrics(P, o.astype(np.float64), d.astype(np.float64))
    u32, v32 = _tri_uv32(tri, o, d)
    assert all((where == w).sum() >= N // 8 for w in range(8))
    worst = {"uv": 0.0, "lib": 0.0, "f32": 0.0}
    for (bw, bh), (ow, oh) in zip(SIZES, SIZES[1:] + SIZES[:1]):
        base, orm = px.image(bh, bw, 51 + bw), px.image(oh, ow, 61 + ow)
        texels, first = _texels(base, orm)
        uv, kind, constant = _coordinates(N, rng, bu, bv, bw, bh)
        u, v, st, cb, co = path_lib.object_texture_host(tri, uv, o, d, _record(path_lib, base, orm, first), texels)
        s64, t64_ = px.texture_st(uv.astype(np.float64), eu, ev)
        s32, t32 = px.texture_st(uv, u32, v32, np.float32)
        lib_err = f32_err = 0.0
        for img, got in ((base, cb), (orm, co)):
            ref = px.texture_fetch(img, s64, t64_)[0]
            lib_err = max(lib_err, float(np.abs(got - ref).max()))
            f32_err = max(f32_err, float(np.abs(px.texture_fetch(img, s32, t32, np.float32)[0].astype(np.float64) - ref).max()))
            assert got.min() >= 0.0 and got.max() <= 1.0
        uv_err = max(float(np.abs(u - eu).max()), float(np.abs(v - ev).max()))
        _report(f"texture fetch vs fp64 on {N} hits, base {bw} x {bh}, orm {ow} x {oh}: max abs error of u, v (bound {UV_TOL:.0e}) / of base, orm / "
                f"of the fp32 transcription (the bound is {MARGIN:g} x it)", f"{uv_err:.3e} / {lib_err:.3e} / {f32_err:.3e}")
        assert uv_err <= UV_TOL and f32_err > 0 and lib_err <= MARGIN * f32_err
        # a constant-coordinate lane reads exactly its target: the fetch at an exact centre is that texel, bit for bit
        centre = constant & (kind == 1)
        assert centre.sum() >= 500
        sc, tc = uv[centre, 0, 0].astype(np.float64), uv[centre, 0, 1].astype(np.float64)
        exact = np.abs((sc - np.floor(sc)) * bw - 0.5 - np.round((sc - np.floor(sc)) * bw - 0.5)) + \
            np.abs((tc - np.floor(tc)) * bh - 0.5 - np.round((tc - np.floor(tc)) * bh - 0.5)) == 0
        assert exact.sum() >= 50                                    # fp32 holds many of the centres exactly (every one of 1 x 1 and 2 x .)
        ix = np.floor((sc - np.floor(sc)) * bw).astype(int)[exact]
        iy = np.floor((1.0 - (tc - np.floor(tc))) * bh).astype(int)[exact] % bh
        assert np.array_equal(cb[centre][exact], base.astype(np.float32)[iy, ix])
        for k in worst:
            worst[k] = max(worst[k], {"uv": uv_err, "lib": lib_err, "f32": f32_err}[k])
    _report("texture fetch vs fp64, the three pairs together: worst error of base, orm / of the fp32 transcription", f"{worst['lib']:.3e} / {worst['f32']:.3e}")
    # constant images, all 0 and all 1: exact, at every coordinate
    uv, _, _ = _coordinates(N, rng, bu, bv, 5, 4)
    for value in (np.float32([0.3, 0.7, 0.123456789]), np.float32([0, 0, 0]), np.float32([1, 1, 1])):
        base, orm = np.broadcast_to(value, (4, 5, 3)), np.broadcast_to(value[::-1], (3, 2, 3))
        texels, first = _texels(base, orm)
        _, _, _, cb, co = path_lib.object_texture_host(tri, uv, o, d, _record(path_lib, base, orm, first), texels)
        assert np.all(cb == value) and np.all(co == value[::-1])
    # an image the record does not have gives (1, 1, 1); a coordinate that is not finite gives the fetch (0, 0, 0)
    base = px.image(4, 5, 7)
    texels, _ = _texels(base)
    _, _, _, cb, co = path_lib.object_texture_host(tri[:64], uv[:64], o[:64], d[:64], _record(path_lib, base), texels)
    assert np.all(co == 1.0) and cb.std() > 0.05
    _, _, _, cb, co = path_lib.object_texture_host(tri[:64], uv[:64], o[:64], d[:64], _record(path_lib, None, base), texels)
    assert np.all(cb == 1.0) and co.std() > 0.05
    bad = uv[:4].copy()
    bad[0, 0, 0], bad[1, 1, 1], bad[2, 2, 0] = np.nan, np.inf, -np.inf
    _, _, st, cb, _ = path_lib.object_texture_host(tri[:4], bad, o[:4], d[:4], _record(path_lib, base), texels)
    assert not np.isfinite(st[:3]).all(-1).any() and np.all(cb[:3] == 0.0) and np.isfinite(st[3]).all()
    flat = path_lib.object_texture_host(tri[:4], uv[:4], tri[:4, 0], tri[:4, 1], _record(path_lib, base), texels)[3]   # rays in the plane
    assert np.all((flat >= 0) & (flat <= 1))
    # the corners of the image, and the seam of both axes: a wide and a tall image through the same routine
    wide = np.zeros((1, 512, 3), np.float32)
    wide[0, 0], wide[0, -1] = 0.25, 0.75
    tall = wide.reshape(512, 1, 3)                                  # row 0 (the top row) 0.25, the bottom row 0.75
    texels, first = _texels(wide, tall)
    corner_st = np.float32([[1.0 - 0.5 / 512, 0.3], [0.5 / 512, 0.3], [0.0, 0.0], [-2.0 ** -30, -2.0 ** -30], [1.0, 7.0], [0.3, 1.0 - 0.5 / 512], [0.3, 0.5 / 512]])
    cuv = np.repeat(corner_st[:, None], 3, 1)
    n = len(corner_st)
    _, _, st, cb, co = path_lib.object_texture_host(tri[:n], cuv, o[:n], d[:n], _record(path_lib, wide, tall, first), texels)
    assert np.array_equal(st, corner_st)
    assert np.all(cb[0] == 0.75) and np.all(cb[1] == 0.25) and np.all(co[5] == 0.25) and np.all(co[6] == 0.75)   # the last and the first texel of each axis
    assert np.all(cb[2:5] == 0.5) and np.all(co[2:5] == 0.5)       # the seam blends the first and the last texel equally, from either side


# ---- (b): the tint guide ----------------------------------------------------------------------------------------------------------------------
def _groove(H, W):
    from materialist_amd import mesh

    rm = mesh.reference_mesh(pf.groove_scene(H, W), FOV)
    rng = np.random.default_rng(11)
    a, r, m = pf.groove_maps(H, W, rng)
    return rm, a, r, m, pf.groove_env(rng)


def test_feature_tints_host_against_the_first_hit(path_lib):
    """`matpbr_path_feature_tints_host` on the table scene at 24 x 20: c_vertex (.) c_base of the restatement's first hit where the centre
    ray lands on a coloured or textured object, within 1e-4 (the colour guide's bound on u and v, times the images' slopes: texel
    differences <= 1 over 1 / w of a coordinate that spans <= 3.4 across a face, a factor the measured figure shows), exactly
    (1, 1, 1) everywhere else."""
    H, W = 20, 24
    objects = px.table_scene()
    rm = _groove(H, W)[0]
    V, T, table = pob.merged(rm["vertices"], rm["triangles"], objects)
    Vm, Tm, tb, tint, tex = path_lib.merge_objects(rm["vertices"], rm["triangles"], objects, colors=True, textures=True)
    n_scene = rm["triangles"].shape[0]
    assert [t.kind for t in tb] == [0x502, 0x403, 0x602, 2, 0x101]
    got = path_lib.feature_tints_host(path_lib.build_bvh(Vm, Tm, n_scene), H, W, FOV, tb, tint, tex, n_scene)
    f = (W / 2.0) / math.tan(math.radians(FOV) / 2.0)
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = _unit(np.stack([(j - (W - 1) / 2) / f, -(i - (H - 1) / 2) / f, -np.ones((H, W))], -1).reshape(-1, 3))
    o = np.zeros_like(d)
    P = V[T]
    t, k = pf.brute(P, o, d)
    ref = np.ones((H * W, 3))
    per_object = []
    on = np.zeros(H * W, bool)
    for e in table[:3]:
        sel = (k >= e["first_tri"]) & (k < e["first_tri"] + e["n_tri"])
        per_object.append(int(sel.sum()))
        on |= sel
        bu, bv = ps.barycentrics(P[k[sel]], o[sel], d[sel])
        local = k[sel] - e["first_tri"]
        if e.get("corner_colors") is not None:
            ref[sel] *= pc.vertex_color(e["corner_colors"][local], bu, bv)
        s_, t_ = px.texture_st(e["corner_uv"][local], bu, bv)
        ref[sel] *= px.texture_fetch(e["texture"], s_, t_)[0]
    worst = float(np.abs(got.reshape(-1, 3) - ref)[on].max())
    _report(f"tint guide vs the first hit: pixels on the textured sphere / PBR cube / coloured and textured cube {per_object}, max abs error (bound 1e-4)",
            f"{worst:.3e}")
    assert min(per_object) >= 4 and worst <= 1e-4
    assert np.all(got.reshape(-1, 3)[~on] == 1.0) and float(got.reshape(-1, 3)[on].std()) > 0.05
    # a table without a textured object: the colour guide's bits, the textures may be None
    plain = px.table_scene(flagged=False)
    Vu, Tu, tbu, tint_u, none = path_lib.merge_objects(rm["vertices"], rm["triangles"], plain, colors=True, textures=True)
    assert none is None and tint_u is not None
    bvh = path_lib.build_bvh(Vu, Tu, n_scene)
    assert np.array_equal(path_lib.feature_tints_host(bvh, H, W, FOV, tbu, tint_u, None, n_scene),
                          path_lib.feature_colors_host(bvh, H, W, FOV, tbu, tint_u, n_scene))


# ---- (c): the restatement against a closed form --------------------------------------------------------------------------------------------------
def furnace_expected(objects, H, W):
    """-> (L p (.) T(s, t at the centre ray's hit) [H,W,3], the pixels whose four corner rays hit the quad)."""
    quad = objects[1]
    f = (W / 2.0) / math.tan(math.radians(FOV) / 2.0)
    z = quad["vertices"][0, 2]
    (cx, cy, _), half = px.FURNACE_QUAD
    covered = np.ones((H, W), bool)
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for di in (-0.5, 0.5):
        for dj in (-0.5, 0.5):
            x, y = (j + dj - (W - 1) / 2) / f * -z, -(i + di - (H - 1) / 2) / f * -z
            covered &= (np.abs(x - cx) < half) & (np.abs(y - cy) < half)
    hit = np.stack([(j - (W - 1) / 2) / f * -z, -(i - (H - 1) / 2) / f * -z, np.full((H, W), z)], -1)
    st = px.furnace_st(hit)
    return pl.FURNACE_L * np.asarray(px.FURNACE_P) * px.furnace_value(st[..., 0], st[..., 1]), covered


def test_restatement_affine_texels_in_a_furnace(path_lib):
    """`path_light_fp64.furnace_scene`'s emitting box of radiance L around a camera-facing diffuse quad at constant depth, max_depth 2:
    the quad's (s, t) are affine in position and stay inside the texel centres' hull, its 5 x 4 texels are affine in their indices, so
    the bilinear fetch is that affine function and the box-filtered pixel is L p (.) T(s, t at the pixel centre).  64 seeds x spp 16 at
    12 x 10, 5 standard errors + 1e-3."""
    H, W = 10, 12
    objects = px.furnace_scene()
    w, h = px.FURNACE_WH
    assert objects[1]["uv"][:, 0].min() >= 0.5 / w and objects[1]["uv"][:, 0].max() <= 1 - 0.5 / w
    assert objects[1]["uv"][:, 1].min() >= 0.5 / h and objects[1]["uv"][:, 1].max() <= 1 - 0.5 / h
    expected, covered = furnace_expected(objects, H, W)
    assert covered.sum() >= 12
    # the fetch is the affine function: at random points of the quad, to fp64 rounding of the fp32 texels
    q = np.random.default_rng(5).uniform(-1, 1, (256, 3)) * px.FURNACE_QUAD[1] + np.asarray(px.FURNACE_QUAD[0])
    st = px.furnace_st(q)
    assert np.abs(px.texture_fetch(px.furnace_texels(), st[:, 0], st[:, 1])[0] - px.furnace_value(st[:, 0], st[:, 1])).max() < 1e-6
    Vs, Ts = pp.FAR_TRIANGLE
    V, T, table = pob.merged(Vs, Ts, objects)
    # the library's tables of this scene are the restatement's: the quad's coordinates per corner and its 20 texels
    obj_uv, recs, texels = path_lib.merge_objects(Vs, Ts, objects, textures=True)[3]
    assert (recs[1].base_first, recs[1].base_w, recs[1].base_h, recs[1].orm_w) == (0, w, h, 0) and recs[0].base_w == 0
    assert np.array_equal(obj_uv[12:], table[1]["corner_uv"].astype(np.float32)) and np.array_equal(texels[:, :3].reshape(h, w, 3), table[1]["texture"].astype(np.float32))
    env = np.zeros((4, 8, 3), np.float32)
    vals = pob.replay_mean(H, W, 16, SEEDS, 2, V, T, env, path_lib.env_tables(env), table)
    ok, excess = pl.within_five_sigma(vals, expected, covered)
    spread = float(expected[covered].max() - expected[covered].min())
    _report(f"affine texels in a furnace: worst |mean - L p T| / (5 se + 1e-3) over {int(covered.sum())} pixels; the expectation's spread", f"{excess:.3f}; {spread:.3f}")
    assert ok and spread > 0.1


# ---- uniform images -----------------------------------------------------------------------------------------------------------------------------
# what the record holds of the flags and the fetches themselves, not of the paths
TEXTURE_RECORD = ("textured_camera", "textured_indirect", "fetch_wraps_columns", "fetch_wraps_rows", "orm_roughness_floor")


def test_uniform_images_are_the_untextured_object(path_lib, oracle64):
    """With every image (1, 1, 1) the restatement equals its render of the unflagged table bit for bit."""
    H, W = 20, 24
    rm, a, r, m, env = _groove(H, W)
    tab = path_lib.env_tables(env)
    V, T, flagged = pob.merged(rm["vertices"], rm["triangles"], px.table_scene(uniform=True))
    lib_tex = path_lib.merge_objects(rm["vertices"], rm["triangles"], px.table_scene(uniform=True), textures=True)[3]
    assert np.all(lib_tex[2][:, :3] == 1.0) and np.all(lib_tex[2][:, 3] == 0.0) and lib_tex[2].shape[0] == 36   # the library's texels of this table: ones
    _, _, plain = pob.merged(rm["vertices"], rm["triangles"], px.table_scene(flagged=False))
    for max_depth, seed in ((2, 0), (6, 1), (16, 2)):
        got, rec = pob.replay_objects(oracle64, V, T, a, r, m, env, tab, H, W, max_depth, seed, flagged)
        ref, rec0 = pob.replay_objects(oracle64, V, T, a, r, m, env, tab, H, W, max_depth, seed, plain)
        assert np.array_equal(got, ref) and rec["textured_camera"][:, :3].any(0).all(), (max_depth, seed)
        assert all(np.array_equal(rec0[k], rec[k]) for k in rec0 if isinstance(rec0[k], np.ndarray) and k not in TEXTURE_RECORD)
    _, _, textured = pob.merged(rm["vertices"], rm["triangles"], px.table_scene())
    tinted, rec = pob.replay_objects(oracle64, V, T, a, r, m, env, tab, H, W, 16, 2, textured)
    on = rec["textured_camera"].any(-1).reshape(H, W)
    assert (np.abs(tinted - ref).max(-1)[on] > 0).mean() > 0.5


def test_restatement_is_the_recorded_texture_restatement(path_lib, oracle64):
    """On the textured table (the groove at 12 x 10, max_depth 6, seed 1) the walk returns the bits the texture restatement returned
    before the walks were folded into one (`path_testlib.recorded_walk`), in the render and in every array of its record."""
    H, W = 10, 12
    rm, a, r, m, env = _groove(H, W)
    V, T, table = pob.merged(rm["vertices"], rm["triangles"], px.table_scene())
    rec0 = tl.recorded_walk("texture")
    ref = rec0.pop("L")
    got, rec = pob.replay_objects(oracle64, V, T, a, r, m, env, path_lib.env_tables(env), H, W, 6, 1, table)
    assert ref.any() and np.array_equal(ref, got)
    assert len(rec0) == 25 and all(np.array_equal(rec0[k], rec[k]) for k in rec0)


# ---- (g): traversal agreement --------------------------------------------------------------------------------------------------------------------
EVENTS = ("textured_indirect", "fetch_wraps_columns", "fetch_wraps_rows", "orm_roughness_floor")


@pytest.mark.parametrize("env_on", [True, False])
def test_restatement_over_fp32_and_fp64_traversal(path_lib, oracle64, env_on):
    """The GPU criterion's ground: over the library's fp32 traversal and over the fp64 brute force the restatement disagrees in NO pixel
    of the GPU test's 18 renders (the groove at 24 x 20 with `path_texture_fp64.table_scene`; max_depth 2, 6, 16; seeds 0-2; the envmap
    on and zero), and every render holds every recorded event."""
    H, W = 20, 24
    objects = px.table_scene()
    rm, a, r, m, env = _groove(H, W)
    if not env_on:
        env = np.zeros_like(env)
    V, T, table = pob.merged(rm["vertices"], rm["triangles"], objects)
    Vm, Tm, tb, tex = path_lib.merge_objects(rm["vertices"], rm["triangles"], objects, textures=True)
    assert tex is not None and [t.kind & path_lib.OBJECT_TEXTURED for t in tb] == [0x400, 0x400, 0x400, 0, 0]
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
            assert rec["textured_camera"][:, :3].any(0).all() and all(rec[e].any() for e in EVENTS), (max_depth, seed, {e: int(rec[e].sum()) for e in EVENTS})
            if not env_on:                                          # this table holds no light: without the envmap there is no emitter, the
                assert not L64.any() and not L32.any()              # criterion's denominator is 0 and both renders are black, exactly
                continue
            err = (np.abs(L32 - L64) / np.maximum(np.abs(L64), np.abs(L64).mean())).max(-1)
            assert int((err > 1e-3).sum()) == 0, (max_depth, seed, np.argwhere(err > 1e-3)[:10])


# ---- (e): the reader -----------------------------------------------------------------------------------------------------------------------------
def _write_ply(path, V, T, UV=None, fmt="ascii", ctype="float", names=("s", "t")):
    """A PLY as a modelling tool writes it: float x y z, optionally texture coordinates of `ctype` named `names`, uchar-counted int faces."""
    np_t = {"float": "<f4", "double": "<f8"}[ctype]
    props = [("x", "float", "<f4"), ("y", "float", "<f4"), ("z", "float", "<f4")] + ([(n, ctype, np_t) for n in names] if UV is not None else [])
    head = f"ply\nformat {fmt} 1.0\nelement vertex {len(V)}\n" + "".join(f"property {t} {n}\n" for n, t, _ in props)
    head += f"element face {len(T)}\nproperty list uchar int vertex_indices\nend_header\n"
    cols = [V[:, 0], V[:, 1], V[:, 2]] + ([UV[:, 0], UV[:, 1]] if UV is not None else [])
    with open(path, "wb") as fh:
        fh.write(head.encode("ascii"))
        if fmt == "ascii":
            for row in zip(*cols):
                fh.write((" ".join(repr(float(x)) for x in row) + "\n").encode())
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


def test_ply_reader_texture_coordinates(tmp_path):
    from materialist_amd import mesh

    V, T = po.cube((0.0, 0.0, -1.0), 0.2, (0.1, 0.2, 0.3))
    V = V.astype(np.float32)
    UV = np.random.default_rng(3).uniform(-2, 3, (8, 2))
    for fmt in ("ascii", "binary_little_endian"):
        p = str(tmp_path / f"{fmt}.ply")
        for names in (("s", "t"), ("u", "v"), ("texture_u", "texture_v")):
            for ctype in ("float", "double"):
                _write_ply(p, V, T, UV, fmt, ctype, names)
                Vr, Tr, Ur = mesh.read_ply_any(p, uv=True)
                want = UV if ctype == "double" or fmt == "ascii" else UV.astype(np.float32).astype(np.float64)   # ascii: the digits as written
                assert np.array_equal(Vr, V.astype(np.float64)) and np.array_equal(Tr, T) and Ur.dtype == np.float64 and Ur.shape == (8, 2)
                assert np.array_equal(Ur, want), (fmt, names, ctype)
        got = mesh.read_ply_any(p, normals=True, colors=True, uv=True)
        assert len(got) == 5 and got[2] is None and got[3] is None and got[4] is not None
        assert len(mesh.read_ply_any(p)) == 2 and len(mesh.read_ply_any(p, colors=True)) == 3      # the existing shapes
        _write_ply(p, V, T, None, fmt)
        assert mesh.read_ply_any(p, uv=True)[2] is None
    mesh.write_ply(str(tmp_path / "own.ply"), V, T)
    assert mesh.read_ply_any(str(tmp_path / "own.ply"), uv=True)[2] is None


# ---- (d): the tables, the value errors, the refusals -----------------------------------------------------------------------------------------------
def test_merge_objects_and_the_value_errors(path_lib):
    Vs, Ts = pp.FAR_TRIANGLE
    objects = px.table_scene()
    V, T, table, corner, records, lt, tint, tex = path_lib.merge_objects(Vs, Ts, objects, normals=True, pbr=True, lights=True, colors=True, textures=True)
    assert [t.kind for t in table] == [0x502, 0x403, 0x602, 2, 0x101] and lt is None and tint is not None
    obj_uv, recs, texels = tex
    assert obj_uv.dtype == np.float32 and obj_uv.shape == (T.shape[0] - 1, 3, 2) and texels.dtype == np.float32 and texels.shape == (20 + 6 + 6 + 4, 4)
    assert [(r.base_first, r.base_w, r.base_h, r.orm_first, r.orm_w, r.orm_h) for r in recs] == \
        [(0, 5, 4, 0, 0, 0), (20, 2, 3, 26, 3, 2), (32, 2, 2, 0, 0, 0), (0, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 0)]
    assert np.all(texels[:, 3] == 0) and np.array_equal(texels[:20, :3], objects[0]["texture"].reshape(-1, 3).astype(np.float32))
    assert np.array_equal(texels[26:32, :3], objects[1]["orm_texture"].reshape(-1, 3).astype(np.float32))
    for k, ob in enumerate(objects):
        sl = slice(table[k].first_tri - 1, table[k].first_tri - 1 + table[k].n_tri)
        want = px.corner_uv(ob)
        assert np.array_equal(obj_uv[sl], want.astype(np.float32) if want is not None else np.zeros((table[k].n_tri, 3, 2), np.float32))
    # the existing return shapes: without textures= nothing follows, and a table without images gives None
    assert len(path_lib.merge_objects(Vs, Ts, objects)) == 3 and len(path_lib.merge_objects(Vs, Ts, objects, normals=True, pbr=True, lights=True, colors=True)) == 7
    assert path_lib.merge_objects(Vs, Ts, px.table_scene(flagged=False), textures=True)[3] is None
    Vc, Tc = po.cube((0.0, 0.0, -1.0), 0.2, (0.0, 0.0, 0.0))
    uv, img = np.full((8, 2), 0.5), np.full((2, 3, 3), 0.5)

    def merge(bsdf=po.DIFFUSE_08, **extra):
        return path_lib.merge_objects(Vs, Ts, [{"vertices": Vc, "triangles": Tc, "bsdf": po.DIFFUSE_08},
                                               {"vertices": Vc + (0.5, 0, 0), "triangles": Tc, "bsdf": bsdf, **extra}], textures=True)

    got = merge(uv=uv, texture=img)[3]
    assert got[0].shape == (24, 3, 2) and not got[0][:12].any() and got[2].shape == (6, 4) and got[1][1].base_w == 3 and got[1][0].base_w == 0
    assert merge(pc.PBR_BASE, uv=uv, orm_texture=img)[3][1][1].orm_h == 2
    with pytest.raises(ValueError, match=r"object 1.*'uv' without an image"):
        merge(uv=uv)
    with pytest.raises(ValueError, match=r"object 1.*'texture' without 'uv'"):
        merge(texture=img)
    with pytest.raises(ValueError, match=r"object 1.*'orm_texture' without 'uv'"):
        merge(pc.PBR_BASE, orm_texture=img)
    for bsdf in (po.GLASS, pl.QUAD_LIGHT, pr.FROSTED_02):
        for extra in ({"uv": uv, "texture": img}, {"uv": uv}, {"texture": img}):
            with pytest.raises(ValueError, match=r"object 1.*(diffuse|pbr)"):
                merge(bsdf, **extra)
    with pytest.raises(ValueError, match=r"object 1.*'orm_texture'.*diffuse"):
        merge(uv=uv, texture=img, orm_texture=img)
    for spoil, pattern in (((3, 1, np.nan), r"object 1.*vertex 3"), ((5, 0, 64.5), r"object 1.*vertex 5"), ((0, 1, -65.0), r"object 1.*vertex 0"),
                           ((7, 0, np.inf), r"object 1.*vertex 7")):
        bad = uv.copy()
        bad[spoil[0], spoil[1]] = spoil[2]
        with pytest.raises(ValueError, match=pattern):
            merge(uv=bad, texture=img)
    merge(uv=np.full((8, 2), -64.0), texture=img)
    with pytest.raises(ValueError, match=r"object 1.*\[Nv,2\]"):
        merge(uv=uv[:7], texture=img)
    for spoil, pattern in (((1, 2, 0, np.nan), r"object 1.*texture.*row 1, column 2"), ((0, 0, 1, 1.5), r"object 1.*row 0, column 0"),
                           ((1, 1, 2, -0.1), r"object 1.*row 1, column 1")):
        bad = img.copy()
        bad[spoil[0], spoil[1], spoil[2]] = spoil[3]
        with pytest.raises(ValueError, match=pattern):
            merge(uv=uv, texture=bad)
        with pytest.raises(ValueError, match=pattern.replace("texture", "orm_texture")):
            merge(pc.PBR_BASE, uv=uv, orm_texture=bad)
    for shape in ((2, 3), (2, 3, 4), (0, 3, 3)):
        with pytest.raises(ValueError, match=r"object 1.*\[h,w,3\]"):
            merge(uv=uv, texture=np.zeros(shape))
    # the entries from before the flag are handed tables without it: the light tables of a scene with a light and a textured object
    Vq, Tq = pl.quad(pl.LIGHT_QUAD)
    lt = path_lib.merge_objects(Vs, Ts, [{"vertices": Vc, "triangles": Tc, "bsdf": po.DIFFUSE_08, "uv": uv, "texture": img},
                                         {"vertices": Vq, "triangles": Tq, "bsdf": pl.QUAD_LIGHT}], pbr=True, lights=True)[4]
    assert lt["header"].n_lights == 1 and lt["header"].object[0] == 1


def test_refusals_of_every_entry(path_lib):
    """By return code, with host-only pointers: the new entries refuse what they cannot take (every invalid argument of the header), and
    every entry from before the flag refuses it as an unknown kind."""
    lib = path_lib.load()
    P_ = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    tab = lambda t: ctypes.cast(t, ctypes.c_void_p)
    raw = np.zeros(40, np.float32)
    one = raw[(-raw.ctypes.data % 16) // 4:][:24]                  # 16-byte aligned: six texels
    one[2] = 1.0
    io = np.zeros(3, np.int32)
    X, C, S = path_lib.OBJECT_TEXTURED, path_lib.OBJECT_COLORED, path_lib.OBJECT_SMOOTH
    obj = lambda k, p=(0.5, 0.5, 0.5), first=1: (path_lib.PathObject * 1)(path_lib.PathObject(k, first, 12, (ctypes.c_float * 3)(*p)))
    rec = (path_lib.PathObjectPbr * 1)(path_lib.PathObjectPbr((ctypes.c_float * 3)(0.5, 0.5, 0.5), 0.5, 0.0))
    tex = lambda *v: (path_lib.PathObjectTex * 1)(path_lib.PathObjectTex(*v))
    good = tex(0, 2, 3)
    frame = [P_(one)] * 5 + [4, 4, 35.0] + [P_(one)] * 4 + [2, 4, 1, 4, 0, 1, P_(one), None, None]
    render = lib.matpbr_path_render_objects_textures
    tail = lambda t=good, uv=P_(one), tx=P_(one), n=6: (uv, tab(t) if t is not None else None, tx, n)
    # the flag on kinds 1, 4, 5 (with and without the other flags), and on no kind
    for k, p in ((1, (1.5, 1.0, 0.0)), (4, (1.0, 1.0, 1.0)), (5, (1.5, 1.0, 0.1)), (0x101, (1.5, 1.0, 0.0)), (0x105, (1.5, 1.0, 0.1)), (0, (0.5,) * 3), (6, (0.5,) * 3)):
        assert render(*frame, tab(obj(k | X, p)), 1, P_(one), 1, tab(rec), None, None, None, P_(one), *tail()) == -1, k
    for k in (2, 3, 2 | S, 3 | S, 2 | C, 3 | C | S):
        head = (*frame, tab(obj(k | X)), 1, P_(one), 1, tab(rec), None, None, None, P_(one))
        assert render(*head, *tail(uv=None)) == -1 and render(*head, *tail(t=None)) == -1 and render(*head, *tail(tx=None)) == -1, k   # a pointer NULL
        assert render(*head, *tail(tx=ctypes.c_void_p(one.ctypes.data + 4))) == -1, k                                                # texels misaligned
        assert render(*head, *tail(tex())) == -1, k                                                                                  # no image
        for bad in (tex(0, 2, 3, 0, 0, 0, (ctypes.c_int32 * 2)(1, 0)), tex(0, 2, 3, 0, 0, 0, (ctypes.c_int32 * 2)(0, -1)),           # reserved
                    tex(-1, 2, 3), tex(1, 2, 3), tex(0, 3, 3), tex(0, 2, -3), tex(0, -2, 3), tex(0, 2, 0), tex(0, 8193, 1), tex(0, 1, 8193),
                    tex(2 ** 31 - 1, 2, 3)):
            assert render(*head, *tail(bad)) == -1, (k, bad[0].base_first, bad[0].base_w, bad[0].base_h)
        assert render(*head, *tail(n=5)) == -1 and render(*head, *tail(n=0)) == -1 and render(*head, *tail(n=-6)) == -1, k           # against n_texels
        orm = tex(0, 0, 0, 0, 3, 2)
        if k & 0xFF == 2:
            assert render(*head, *tail(orm)) == -1 and render(*head, *tail(tex(0, 2, 3, 0, 3, 2))) == -1, k                          # orm on kind 2
        else:
            for bad in (tex(0, 0, 0, 1, 3, 2), tex(0, 0, 0, -1, 3, 2), tex(0, 2, 3, 0, 3, 3), tex(0, 2, 3, 0, 8193, 1)):
                assert render(*head, *tail(bad)) == -1, k
        assert render(*frame, tab(obj(k | X)), 1, P_(one), 2, tab(rec), None, None, None, P_(one), *tail()) == -1, k                 # below n_scene_tri
    assert render(*frame, tab(obj(3 | X)), 1, None, 1, None, None, None, None, None, *tail()) == -1                                  # kind 3 without records
    assert render(*frame, tab(obj(2 | X | S)), 1, None, 1, None, None, None, None, None, *tail()) == -1                              # smooth without normals
    assert render(*frame, tab(obj(2 | X | C)), 1, None, 1, None, None, None, None, None, *tail()) == -1                              # coloured without colours
    assert render(*frame, tab(obj(2 | X, (0.5, 1.5, 0.5))), 1, None, 1, None, None, None, None, None, *tail()) == -1                 # level 1's bounds hold
    assert render(*frame, None, 1, None, 1, None, None, None, None, None, None, None, None, 0) == -1
    # every entry from before the flag refuses it
    for k in (2 | X, 3 | X, 2 | S | X, 2 | C | X):
        t = tab(obj(k))
        assert lib.matpbr_path_render_objects(*frame, t, 1) == -1
        assert lib.matpbr_path_render_objects_normals(*frame, t, 1, P_(one), 1) == -1
        assert lib.matpbr_path_render_objects_pbr(*frame, t, 1, P_(one), 1, tab(rec)) == -1
        assert lib.matpbr_path_render_objects_lights(*frame, t, 1, P_(one), 1, tab(rec), None, None, None) == -1
        assert lib.matpbr_path_render_objects_rough(*frame, t, 1, P_(one), 1, tab(rec), None, None, None) == -1
        assert lib.matpbr_path_render_objects_colors(*frame, t, 1, P_(one), 1, tab(rec), None, None, None, P_(one)) == -1
        assert lib.matpbr_path_features(P_(one), P_(one), 4, 4, 35.0, t, 1, P_(one), 1, None, P_(one), None) == -1
        assert lib.matpbr_path_features_host(P_(one), P_(one), 4, 4, 35.0, t, 1, P_(one), 1, None, P_(one)) == -1
        assert lib.matpbr_path_feature_colors(P_(one), P_(one), 4, 4, 35.0, t, 1, 1, P_(one), P_(one), None) == -1
        assert lib.matpbr_path_feature_colors_host(P_(one), P_(one), 4, 4, 35.0, t, 1, 1, P_(one), P_(one)) == -1
        assert lib.matpbr_path_object_lookup_host(t, 1, tab(rec), P_(io), 1, P_(io), P_(one), P_(one), P_(one)) == -1
        assert lib.matpbr_path_object_sample_host(t, P_(one), P_(one), P_(one), 1, P_(one), P_(one), P_(one), P_(io)) == -1
        head, n = path_lib.PathLights(), ctypes.c_long(0)
        assert lib.matpbr_path_light_tables(P_(np.zeros(9)), 3, P_(np.zeros(3, np.int32)), 1, t, 1, tab(rec), ctypes.cast(ctypes.byref(head), ctypes.c_void_p),
                                            None, None, 0, ctypes.cast(ctypes.byref(n), ctypes.c_void_p)) == -1
    # the fetch routine
    host = lib.matpbr_path_object_texture_host
    full = [P_(one), P_(one), P_(one), P_(one), 1, tab(good), P_(one), 6, P_(one), P_(one), P_(one), P_(one), P_(one)]
    for k in (0, 1, 2, 3, 5, 6, 8, 9, 10, 11, 12):
        assert host(*(None if j == k else x for j, x in enumerate(full))) == -1, k
    for j, v in ((4, -1), (7, 5), (7, 0), (5, tab(tex())), (5, tab(tex(0, 2, 3, 0, 0, 0, (ctypes.c_int32 * 2)(0, 1)))), (5, tab(tex(1, 2, 3))), (5, tab(tex(0, 0, 0, 0, 2, 4))),
                 (6, ctypes.c_void_p(one.ctypes.data + 8))):
        assert host(*(v if i == j else x for i, x in enumerate(full))) == -1, (j, v)
    assert host(*full[:4], 0, *full[5:]) == 0 and host(*full) == 0 and host(*full[:5], tab(tex(0, 2, 3, 0, 3, 2)), *full[6:]) == 0
    # the guide
    for fn, end in ((lib.matpbr_path_feature_tints, (None,)), (lib.matpbr_path_feature_tints_host, ())):
        ok = [P_(one), P_(one), 4, 4, 35.0, tab(obj(2 | X)), 1, 1, None, P_(one), tab(good), P_(one), 6, P_(one)]
        for j, v in ((0, None), (1, None), (2, 0), (3, -1), (4, 0.0), (4, 180.0), (4, float("nan")), (5, None), (6, 9), (6, -1), (7, -1), (7, 2), (9, None), (10, None),
                     (11, None), (12, 5), (13, None), (10, tab(tex())), (10, tab(tex(0, 0, 0, 0, 2, 3))), (5, tab(obj(2 | X | C))),
                     (5, tab(obj(1 | X, (1.5, 1.0, 0.0)))), (5, tab(obj(4 | X))), (5, tab(obj(5 | X, (1.5, 1.0, 0.1)))), (5, tab(obj(7)))):
            assert fn(*(v if i == j else x for i, x in enumerate(ok)), *end) == -1, (fn.__name__, j, v)
    with pytest.raises(ValueError, match="same rows"):
        path_lib.object_texture_host(np.zeros((2, 3, 3)), np.zeros((1, 3, 2)), np.zeros((2, 3)), np.zeros((2, 3)), good[0], np.zeros((6, 4)))
    assert "textured object without coordinates" in lib.matpbr_path_strerror(-1).decode()


# ---- (f): the routing ----------------------------------------------------------------------------------------------------------------------------
class _Host:
    """torch.from_numpy's result for a tracer built without a device: keeps the array, `.to()` returns itself."""

    def __init__(self, x):
        self.x = x
        self.shape = x.shape

    def to(self, *a, **k):
        return self

    def data_ptr(self):
        return self.x.ctypes.data


def test_routing(path_lib, monkeypatch):
    """`PathTracer` without a textured object asks for no new symbol, holds no texture and keeps its nine object arguments; with one it
    asks for the new render entry and the guide, counts it, builds the 13-value tail whose first nine are what they were, routes
    `render` to the new entry and hides the flag from the three older entries that read the table."""
    asked, calls = [], []
    real = path_lib.symbol

    table_at = {"matpbr_path_light_tables": 4, "matpbr_path_features": 5, "matpbr_path_feature_colors": 5, "matpbr_path_feature_tints": 5}

    def spy(name, lib=None):
        asked.append(name)
        if name in table_at:                                        # record the kinds of the table the entry is handed
            def fake(*args):
                table, n = args[table_at[name]], args[table_at[name] + 1]
                kinds = [ctypes.cast(table, ctypes.POINTER(path_lib.PathObject))[k].kind for k in range(n)]
                calls.append((name, kinds, args))
                return real(name, lib)(*args) if name == "matpbr_path_light_tables" else 0
            return fake
        return real(name, lib)

    monkeypatch.setattr(path_lib, "symbol", spy)
    monkeypatch.setattr(path_lib.torch, "from_numpy", lambda x: _Host(x))
    Vs, Ts = pp.FAR_TRIANGLE
    for objects in (pc.table_scene(), pr.table_scene(), pl.table_scene(), pp.table_scene(), ps.table_scene(), po.two_cubes(), px.table_scene(flagged=False), None):
        del asked[:]
        tracer = path_lib.PathTracer(Vs, Ts, 4, 4, FOV, device="cpu", objects=objects)
        assert not NEW & set(asked) and tracer.textures is None and tracer.stats["n_textured_objects"] == 0
        assert len(tracer.object_args()) == 9
    del asked[:], calls[:]
    Vq, Tq = pl.quad(pl.LIGHT_QUAD)
    objects = px.table_scene() + [{"vertices": Vq, "triangles": Tq, "bsdf": pl.QUAD_LIGHT}]
    tracer = path_lib.PathTracer(Vs, Ts, 4, 4, FOV, device="cpu", objects=objects)
    assert {"matpbr_path_render_objects_textures", "matpbr_path_feature_tints", "matpbr_path_render_objects_colors", "matpbr_path_feature_colors"} <= set(asked)
    st = tracer.stats
    assert st["n_textured_objects"] == 3 and st["n_colored_objects"] == 1 and st["n_pbr_objects"] == 1 and st["n_smooth_objects"] == 2 and st["n_lights"] == 1
    kinds = [t.kind for t in tracer.objects]
    assert kinds == [0x502, 0x403, 0x602, 2, 0x101, 4]
    assert calls and calls[0][0] == "matpbr_path_light_tables" and calls[0][1] == [0x102, 0x003, 0x002, 2, 0x101, 4]     # the light tables: no flag
    args = tracer.object_args()
    uv, recs, texels = tracer.textures
    assert len(args) == 13 and args[8] == tracer.obj_col.x.ctypes.data and args[9] == uv.x.ctypes.data and args[11] == texels.x.ctypes.data
    assert args[12] == 36 == texels.x.shape[0] and ctypes.cast(args[10], ctypes.POINTER(path_lib.PathObjectTex))[1].orm_first == 26
    plain = path_lib.PathTracer(Vs, Ts, 4, 4, FOV, device="cpu", objects=[{k: v for k, v in ob.items() if k not in ("uv", "texture", "orm_texture")} for ob in objects])
    assert [type(x) for x in plain.object_args()] == [type(x) for x in args[:9]] and args[1] == 6 and args[3] == 1
    assert len(tl.object_tail(tracer, "matpbr_path_render_objects_textures")) == 13 and len(tl.object_tail(tracer, "matpbr_path_render_objects_colors")) == 9
    # the three older entries see the table without the flag; the new guide sees it
    monkeypatch.setattr(path_lib.torch, "empty", lambda *a, **k: _Host(np.zeros(a, np.float32)))
    monkeypatch.setattr(path_lib.torch.cuda, "current_stream", lambda *a: type("S", (), {"cuda_stream": None})())
    del calls[:]
    tracer.features()
    tracer.feature_colors()
    tracer.feature_tints()
    assert [(c[0], c[1]) for c in calls] == [("matpbr_path_features", [0x102, 0x003, 0x002, 2, 0x101, 4]),
                                             ("matpbr_path_feature_colors", [0x102, 0x003, 0x202, 2, 0x101, 4]),
                                             ("matpbr_path_feature_tints", kinds)]
    plain_value = lambda x: x.value if isinstance(x, ctypes.c_void_p) else x
    assert [plain_value(x) for x in calls[2][2][8:13]] == [tracer.obj_col.x.ctypes.data, *(plain_value(x) for x in args[9:13])]
    with pytest.raises(ValueError, match="objects"):
        tracer.render_bwd(None, None, None, None, None)


def test_scene_file_command_line_and_images(path_lib, tmp_path):
    import torch
    from PIL import Image

    import render_final
    from materialist_amd import mesh, relight
    from materialist_amd.imageio_exr import write_exr
    from materialist_amd.imageio_hdr import write_hdr

    a = render_final.parse_args(["--save_name", "case", "--mode", "oi", "--oi_texture", "wood.png"])
    assert a.oi_texture == "wood.png" and render_final.parse_args(["--save_name", "case", "--mode", "oi"]).oi_texture is None
    Vc, Tc = po.cube((0.0, 0.0, -1.0), 0.2, (0.1, 0.2, 0.3))
    UV = np.random.default_rng(4).uniform(-1, 2, (8, 2))
    os.makedirs(tmp_path / "lists")
    _write_ply(str(tmp_path / "lists" / "crate.ply"), Vc.astype(np.float32), Tc, UV, "binary_little_endian")
    mesh.write_ply(str(tmp_path / "lists" / "grey.ply"), Vc, Tc)
    px8 = np.random.default_rng(5).integers(0, 256, (3, 2, 3), dtype=np.uint8)
    Image.fromarray(px8, "RGB").save(str(tmp_path / "lists" / "wood.png"))
    Image.fromarray(px8[..., 0], "L").save(str(tmp_path / "lists" / "grey.png"))
    lin = np.random.default_rng(6).random((2, 2, 3)).astype(np.float32)
    write_exr(str(tmp_path / "lists" / "lin.exr"), lin)
    write_exr(str(tmp_path / "lists" / "hot.exr"), lin * 3)
    path = str(tmp_path / "lists" / "crate.json")

    def write(objects):
        with open(path, "w") as f:
            json.dump({"objects": objects}, f)

    write([{"ply": "crate.ply", "bsdf": pc.PBR_BASE, "texture": "wood.png", "orm_texture": "lin.exr"}, {"ply": "crate.ply", "bsdf": po.DIFFUSE_08}])
    got = relight.load_oi_scene(path)
    assert got[0]["texture"] == str(tmp_path / "lists" / "wood.png") and got[0]["orm_texture"] == str(tmp_path / "lists" / "lin.exr")
    assert got[1]["texture"] is None and got[1]["orm_texture"] is None and got[0]["colors"] == "none"
    write([{"ply": "crate.ply", "bsdf": po.DIFFUSE_08, "texture": "none.png"}])
    with pytest.raises(ValueError, match=r"crate.json: objects\[0\].*no such texture"):
        relight.load_oi_scene(path)
    write([{"ply": "crate.ply", "bsdf": po.DIFFUSE_08, "orm_texture": "wood.png"}])
    with pytest.raises(ValueError, match=r"crate.json: objects\[0\].*'orm_texture' belongs to a 'pbr'"):
        relight.load_oi_scene(path)
    for bsdf in (po.GLASS, pl.QUAD_LIGHT, pr.FROSTED_02):
        write([{"ply": "crate.ply", "bsdf": bsdf, "texture": "wood.png"}])
        with pytest.raises(ValueError, match=r"crate.json: objects\[0\].*'texture' belongs to a 'diffuse' or a 'pbr'"):
            relight.load_oi_scene(path)
    # the decoding: a PNG of display values through the 2.2 power, an orm image never decoded, an .exr as written and inside [0, 1]
    assert np.allclose(relight._object_image(str(tmp_path / "lists" / "wood.png"), True), (px8 / 255.0) ** 2.2, rtol=0, atol=1e-15)
    assert np.array_equal(relight._object_image(str(tmp_path / "lists" / "wood.png"), False), px8 / 255.0)
    assert np.array_equal(relight._object_image(str(tmp_path / "lists" / "grey.png"), False), np.repeat(px8[..., :1] / 255.0, 3, -1))
    assert np.array_equal(relight._object_image(str(tmp_path / "lists" / "lin.exr"), True), lin.astype(np.float64))
    with pytest.raises(ValueError, match=r"hot\.exr.*\[0, 1\]"):
        relight._object_image(str(tmp_path / "lists" / "hot.exr"), True)
    # a file without coordinates, on both routes
    os.makedirs(tmp_path / "case" / "best_results")
    write_hdr(str(tmp_path / "case" / "best_results" / "envmap.hdr"), np.ones((4, 8, 3), np.float32))
    write([{"ply": "grey.ply", "bsdf": po.DIFFUSE_08, "texture": "wood.png"}])
    with pytest.raises(ValueError, match=r"grey\.ply.*texture coordinates"):
        relight.render_oi("case", input_path=str(tmp_path), save_path=str(tmp_path), objects_file=path)
    mesh.write_ply(str(tmp_path / "case" / "oi2.ply"), Vc, Tc)
    with pytest.raises(ValueError, match=r"oi2\.ply.*texture coordinates"):
        relight.render_oi("case", input_path=str(tmp_path), save_path=str(tmp_path), object_texture=str(tmp_path / "lists" / "wood.png"))
    # the guide takes the tints where it takes the colours
    geom = torch.zeros(1, 3, 8)
    geom[..., 7] = torch.tensor([[1.0, 2.0, 0.0]])
    tint = torch.tensor([[[0.5, 0.25, 1.0], [0.5, 0.5, 0.5], [1.0, 1.0, 1.0]]])
    guide = relight.albedo_guide(geom, torch.full((1, 3, 3), 0.25), [pc.PBR_BASE, po.GLASS], tint).numpy()
    assert np.allclose(guide[0, 0], np.float32(pc.PBR_BASE["albedo"]) * np.float32([0.5, 0.25, 1.0])) and np.all(guide[0, 1] == 1.0)
