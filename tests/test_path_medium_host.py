"""Media inside glass objects on the CPU ("Media inside glass"): the fp64 walk of tests/path_medium_fp64.py
against the shared one where no object holds a medium, the two CPU twins of the library against fp64, the restatement over the
library's fp32 traversal against the brute force on the GPU test's renders, and every refusal from the C ABI up to the object list."""
import ctypes
import json

import numpy as np
import pytest

import path_fp64 as pf
import path_medium_fp64 as pm
import path_objects_fp64 as pob
import path_oi_fp64 as po
import path_rough_fp64 as pr
import path_testlib as tl

FOV = pf.FOV
_report = tl.reporter("path medium host", "test_path_medium_host")


@pytest.fixture(scope="module")
def path_lib():
    return tl.load()


def _groove(H, W):
    from materialist_amd import mesh

    rm = mesh.reference_mesh(pf.groove_scene(H, W), FOV)
    rng = np.random.default_rng(11)
    a, r, m = pf.groove_maps(H, W, rng)
    return rm, a, r, m, pf.groove_env(rng)


def _record(path_lib, sigma_a=(0.0, 0.0, 0.0), sigma_s=0.0, g=0.0, reserved=(0.0, 0.0, 0.0)):
    return path_lib.PathObjectMedium((ctypes.c_float * 3)(*sigma_a), sigma_s, g, (ctypes.c_float * 3)(*reserved))


def _segment(path_lib, rec, t, u9):
    t, u9 = np.ascontiguousarray(t, np.float32), np.ascontiguousarray(u9, np.float32)
    sc, dist, w = np.zeros(t.size, np.int32), np.zeros(t.size, np.float32), np.zeros((t.size, 3), np.float32)
    code = path_lib.symbol("matpbr_path_medium_segment_host")(path_lib._ref(rec), path_lib._ptr(t), path_lib._ptr(u9), t.size, path_lib._ptr(sc),
                                                              path_lib._ptr(dist), path_lib._ptr(w))
    return code, sc.astype(bool), dist, w


def _phase(path_lib, g, d, u):
    d, u = np.ascontiguousarray(d, np.float32), np.ascontiguousarray(u, np.float32)
    wi = np.zeros_like(d)
    code = path_lib.symbol("matpbr_path_phase_sample_host")(g, path_lib._ptr(d), path_lib._ptr(u), d.shape[0], path_lib._ptr(wi))
    return code, wi


def test_symbols(path_lib):
    lib = path_lib.load()
    assert path_lib.MEDIUM_SYMBOLS == ("matpbr_path_render_objects_media", "matpbr_path_render_objects_diff_media", "matpbr_path_medium_segment_host",
                                       "matpbr_path_phase_sample_host")
    for name in path_lib.MEDIUM_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.argtypes == path_lib.SIGNATURES[name][1] and fn.restype == path_lib.SIGNATURES[name][0], name
        assert name not in path_lib.LATE_SYMBOLS
    P, sig = ctypes.c_void_p, path_lib.SIGNATURES
    assert sig["matpbr_path_render_objects_media"][1] == sig["matpbr_path_render_objects_textures"][1] + [P]
    assert sig["matpbr_path_render_objects_diff_media"][1] == sig["matpbr_path_render_objects_ratio"][1] + [P]
    assert path_lib.OBJECT_MEDIUM == 0x800 and ctypes.sizeof(path_lib.PathObjectMedium) == 32
    assert not path_lib.OBJECT_MEDIUM & path_lib.OBJECT_FLAGS


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["rough table", "two cubes"])
def test_the_walk_without_a_medium_is_the_shared_walk(path_lib, oracle64, scene):
    """On a table without a medium `replay_medium` returns the bits of `path_objects_fp64.replay_objects`, in the render and in every
    key the two records share, and none of the medium's keys is set."""
    H, W = 10, 12
    rm, a, r, m, env = _groove(H, W)
    objects = pr.table_scene() if scene == "rough table" else po.two_cubes()
    V, T, table = pob.merged(rm["vertices"], rm["triangles"], objects)
    V2, T2, table2 = pm.merged(rm["vertices"], rm["triangles"], objects)
    assert np.array_equal(V, V2) and np.array_equal(T, T2)
    tab = path_lib.env_tables(env)
    for max_depth, seed in ((6, 1), (16, 2)):
        ref, rec0 = pob.replay_objects(oracle64, V, T, a, r, m, env, tab, H, W, max_depth, seed, table)
        got, rec1 = pm.replay_medium(oracle64, V2, T2, a, r, m, env, tab, H, W, max_depth, seed, table2)
        assert np.array_equal(ref.view(np.uint64), got.view(np.uint64)), (scene, max_depth, seed)
        shared = [k for k in rec1 if k in rec0]
        assert len(shared) >= 20 and all(np.array_equal(rec0[k], rec1[k]) for k in shared)
        assert not any(rec1[k].any() for k in pm.RECORD_KEYS)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_segment_twin_against_fp64(path_lib):
    """`matpbr_path_medium_segment_host` in both branches.  Where the flight is sampled, dist = fl(fl(-logf(1 - u)) / sigma_s): 1 - u
    is exact for a 24-bit u, logf is within 1 ulp (the libm bound the project's other twins use) and the division rounds once, so
    |dist / s64 - 1| <= 2^-23 + 2^-24 + their product < 3.01 * 2^-24.  The weight is expf(fl(-sigma_a dist)) over the twin's own
    dist: the product rounds once, which moves the exponent x = sigma_a dist <= 20 by at most x 2^-24 and so the result by a
    relative e^(20 * 2^-24) - 1 < 20.001 * 2^-24, and expf is within 1 ulp = 2^-23: in all < 22.01 * 2^-24 relative.  The decision
    s < t is exact in the twin's own s: t one ulp above it scatters, t equal to it or one ulp below does not."""
    rng = np.random.default_rng(5)
    N = 4096
    u = (rng.integers(0, 1 << 24, N).astype(np.float64) * 2.0 ** -24)
    u[:2] = 0.0, 1.0 - 2.0 ** -24
    worst_d = worst_w = 0.0
    for sigma_a, sigma_s in (((0.5, 1.0, 2.0), 3.0), ((0.0, 0.0, 0.0), 0.25), ((1.2, 0.0, 0.3), 0.0), ((0.3, 0.7, 1.1), 17.0)):
        rec = _record(path_lib, sigma_a, sigma_s, 0.3)
        sa = np.asarray(np.float32(sigma_a), np.float64)
        t_max = 20.0 / max(sa.max(), 1e-30)
        if sigma_s == 0.0:                                        # no flight: the hit is reached, and u9 is not read
            t = np.float32(rng.uniform(0.0, min(t_max, 50.0), N))
            code, sc, dist, w = _segment(path_lib, rec, t, np.full(N, np.nan))
            assert code == 0 and not sc.any() and np.array_equal(dist, t)
        else:
            code, _, s32, _ = _segment(path_lib, rec, np.full(N, np.float32(3e38)), u)    # the twin's own flights
            assert code == 0
            s64 = pm.flight(float(np.float32(sigma_s)), u)
            assert s32[0] == 0.0 and np.isfinite(s32).all()
            rel = np.abs(s32[1:].astype(np.float64) / s64[1:] - 1.0)
            worst_d = max(worst_d, float(rel.max()))
            assert rel.max() <= 3.01 * 2.0 ** -24, (sigma_s, rel.max())
            # s within an ulp of t on either side, and far from it on either side
            for t, want in ((np.nextafter(s32, np.float32(np.inf)), True), (s32, False), (np.nextafter(s32, np.float32(-np.inf)), False),
                            (s32 * np.float32(2.0) + np.float32(1e-3), True), (s32 * np.float32(0.5), False)):
                keep = (t > 0) & (sa.max() * np.minimum(t, s32).astype(np.float64) <= 20.0)
                code, sc, dist, w = _segment(path_lib, rec, t[keep], u[keep])
                assert code == 0 and np.array_equal(sc, np.full(int(keep.sum()), want)), (sigma_s, want)
                assert np.array_equal(dist, s32[keep] if want else t[keep])
            t = np.float32(rng.uniform(0.0, min(t_max, 4.0 / sigma_s), N))
            code, sc, dist, w = _segment(path_lib, rec, t, u)
            assert code == 0 and sc.any() and not sc.all()
            assert np.array_equal(dist, np.where(sc, s32, t))
        assert (sa.max() * dist.astype(np.float64) <= 20.0).all()
        ref = np.exp(-sa[None, :] * dist.astype(np.float64)[:, None])
        rel = np.abs(w.astype(np.float64) / ref - 1.0)
        worst_w = max(worst_w, float(rel.max()))
        assert rel.max() <= 22.01 * 2.0 ** -24, (sigma_a, sigma_s, rel.max())
        if not any(sigma_a):                                      # a medium without absorption multiplies by exactly 1
            assert np.array_equal(w, np.ones_like(w))
    _report("segment twin: worst |dist / fp64 - 1| and |weight / fp64 - 1| in units of 2^-24 (bounds 3.01, 22.01)",
            f"{worst_d * 2 ** 24:.3f} {worst_w * 2 ** 24:.3f}")


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [-0.99, -0.5, 0.0, 5e-4, 0.5, 0.99])
def test_phase_sampler(path_lib, g):
    """2^16 stratified u over a 256 x 256 grid, one random unit d per lane.  Unit length: the frame is orthonormal and cos^2 + sin^2 =
    1, each up to a few fp32 roundings, and the three-term sums add a few more: 32 ulp = 1.9e-6 bounds them.  The mean of d . wi is g:
    Henyey-Greenstein has E cos = g and E cos^2 = (1 + 2 g^2) / 3, so an iid mean has sigma = sqrt((1 - g^2) / (3 N)), and a stratified
    one no more; |g| = 5e-4 samples the isotropic law, whose mean 0 lies inside the same 5 sigma.  At g = 0 the forward hemisphere's
    count is binomial(N, 1/2) at the most: N / 2 within 5 sqrt(N) / 2."""
    rng = np.random.default_rng(17)
    n = 256
    N = n * n
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    u = np.stack([(i + rng.random((n, n))) / n, (j + rng.random((n, n))) / n], -1).reshape(N, 2)
    u = np.minimum(np.float32(u), np.float32(1.0 - 2.0 ** -24))
    d = rng.normal(size=(N, 3))
    d = np.float32(d / np.linalg.norm(d, axis=-1, keepdims=True))
    d[:4] = (0, 0, 1), (0, 0, -1), (1, 0, 0), (0, -1, 0)          # the frame's poles and two axes
    code, wi = _phase(path_lib, g, d, u)
    assert code == 0 and np.isfinite(wi).all()
    ln = np.linalg.norm(wi.astype(np.float64), axis=-1)
    assert np.abs(ln - 1.0).max() <= 32 * 2.0 ** -24, np.abs(ln - 1.0).max()
    cos = (wi.astype(np.float64) * d.astype(np.float64)).sum(-1)
    sigma = np.sqrt((1.0 - g * g) / (3.0 * N))
    _report(f"phase sampler g = {g}: mean d . wi - g in sigma, max | |wi| - 1 | in ulp", f"{(cos.mean() - g) / sigma:+.3f} {np.abs(ln - 1).max() * 2 ** 24:.2f}")
    assert abs(cos.mean() - g) <= 5.0 * sigma, (g, cos.mean())
    if g == 0.0:
        assert abs(int((cos > 0).sum()) - N // 2) <= 5.0 * np.sqrt(N) / 2.0
    assert path_lib.symbol("matpbr_path_phase_sample_host")(1.0, path_lib._ptr(d), path_lib._ptr(u), 4, path_lib._ptr(wi)) == -1
    assert path_lib.symbol("matpbr_path_phase_sample_host")(float("nan"), path_lib._ptr(d), path_lib._ptr(u), 4, path_lib._ptr(wi)) == -1


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
MEDIUM_SEEDS = (0, 1, 2)


def test_restatement_over_fp32_and_fp64_traversal(path_lib, oracle64):
    """The GPU criterion's ground: over the library's fp32 traversal and over the fp64 brute force the restatement agrees within 1e-3
    in at least 0.99 of the pixels (rough glass's criterion, `path_testlib.parity`) of each of the GPU test's renders (the groove at
    24 x 20 with `path_medium_fp64.table_scene`; max_depth 2, 6, 16; three seeds), and across the renders every kind of path through
    a medium occurs."""
    H, W = 20, 24
    objects = pm.table_scene()
    rm, a, r, m, env = _groove(H, W)
    V, T, table = pm.merged(rm["vertices"], rm["triangles"], objects)
    s = path_lib.merge_scene(rm["vertices"], rm["triangles"], objects, lights=True)
    n_scene = rm["triangles"].shape[0]
    M = path_lib.OBJECT_MEDIUM
    assert [t.kind for t in s.table] == [0x101 | M, 5 | M, 4, 2] and s.lights["header"].n_lights == 1
    assert [tuple(x.sigma_a) + (x.sigma_s, x.g) for x in s.media] == [(4.0, 9.0, 16.0, 0.0, 0.0), (0.5, 1.0, 2.0, 6.0, 0.5), (0.0,) * 5, (0.0,) * 5]
    bvh = path_lib.build_bvh(s.V, s.T, n_scene)

    def closest(o, d):
        t, k = path_lib.trace_host(bvh, o, d)
        return np.where(k < 0, np.inf, t.astype(np.float64)), k.astype(np.int64)

    tab = path_lib.env_tables(env)
    seen = {k: 0 for k in pm.RECORD_KEYS}
    for max_depth in (2, 6, 16):
        for seed in MEDIUM_SEEDS:
            args = (oracle64, V, T, a, r, m, env, tab, H, W, max_depth, seed, table)
            L64, rec = pm.replay_medium(*args)
            L32, _ = pm.replay_medium(*args, closest=closest)
            assert rec["n_e"] == 2
            frac, err = tl.parity(L32, L64)
            _report(f"restatement over fp32 traversal, max_depth {max_depth} seed {seed}: share of pixels within 1e-3",
                    f"{frac:.4f} ({int((err > 1e-3).sum())} flipped paths)")
            assert frac >= 0.99, (max_depth, seed, frac, np.argwhere(err > 1e-3)[:10])
            for k in pm.RECORD_KEYS:
                seen[k] += int(rec[k].sum())
    _report("pixels with " + " / ".join(pm.RECORD_KEYS) + " (9 renders)", " / ".join(str(seen[k]) for k in pm.RECORD_KEYS))
    assert all(seen[k] > 0 for k in pm.RECORD_KEYS), seen


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
def _raw_frame():
    """The 21 leading arguments of a render entry with non-null dummies, which a refusing call never reads."""
    d = ctypes.c_void_p(64)
    return (d, d, d, d, d, 4, 4, 35.0, d, d, d, d, 2, 4, 1, 2, 0, 1, d, None, None)


def test_the_library_refuses(path_lib):
    """Invalid argument (-1) before anything is read or launched: the flag on kinds 2, 3 and 4; a bad record; `media` NULL with a
    flagged object; a flagged table at every level below 8; the superset entry with exactly one of photo and through."""
    M, S = path_lib.OBJECT_MEDIUM, path_lib.OBJECT_SMOOTH
    media_entry, diff_entry = path_lib.symbol("matpbr_path_render_objects_media"), path_lib.symbol("matpbr_path_render_objects_diff_media")
    d = ctypes.c_void_p(64)
    good = (path_lib.PathObjectMedium * 1)(_record(path_lib, (1.0, 2.0, 3.0), 0.5, 0.2))
    pbr = (path_lib.PathObjectPbr * 1)(path_lib.PathObjectPbr((ctypes.c_float * 3)(0.5, 0.5, 0.5), 0.5, 0.0))

    def table(kind, p=(1.49, 1.000277, 0.1)):
        return (path_lib.PathObject * 1)(path_lib.PathObject(kind, 10, 4, (ctypes.c_float * 3)(*p)))

    def level8(tb, media, nrm=d):
        return media_entry(*_raw_frame(), tb, 1, nrm, 10, ctypes.cast(pbr, ctypes.c_void_p), None, None, None, None, None, None, None, 0,
                           None if media is None else ctypes.cast(media, ctypes.c_void_p))

    for kind, p in ((2, (0.5, 0.5, 0.5)), (3, (0, 0, 0)), (4, (1, 1, 1)), (2 | S, (0.5, 0.5, 0.5)), (1 | M | path_lib.OBJECT_COLORED, (1.5, 1.0, 0.0))):
        assert level8(table(kind | M, p), good) == -1, kind
    for kind in (1, 5, 1 | S, 5 | S):
        assert level8(table(kind | M), None) == -1, kind           # a flagged object without records
    bad = [dict(sigma_a=(-1e-6, 0, 0)), dict(sigma_a=(0, float("nan"), 0)), dict(sigma_a=(0, 0, float("inf"))), dict(sigma_s=-1.0),
           dict(sigma_s=float("inf")), dict(sigma_s=float("nan")), dict(g=0.9901), dict(g=-1.0), dict(g=float("nan")), dict(reserved=(0, 1e-30, 0))]
    t_, u_ = np.float32([1.0]), np.float32([0.5])
    assert _segment(path_lib, _record(path_lib), t_, u_)[0] == 0                       # all zero is valid
    assert _segment(path_lib, _record(path_lib, (1, 2, 3), 4.0, 0.99), t_, u_)[0] == 0
    assert _segment(path_lib, _record(path_lib, (1, 2, 3), 4.0, -0.99), t_, u_)[0] == 0
    for kw in bad:
        rec = _record(path_lib, **kw)
        assert _segment(path_lib, rec, t_, u_)[0] == -1, kw
        assert level8(table(1 | M), (path_lib.PathObjectMedium * 1)(rec)) == -1, kw
    # levels 1-7 refuse a flagged table
    tb = table(1 | M)
    tail = (tb, 1, d, 10, ctypes.cast(pbr, ctypes.c_void_p), None, None, None, None, None, None, None, 0)
    for name, n in path_lib.OBJECT_ENTRIES.items():
        if name == "matpbr_path_render_objects_through":
            continue
        assert path_lib.symbol(name)(*_raw_frame(), *tail[:n]) == -1, name
    fr = _raw_frame()
    outs = (d, d, d, None)
    for name, own in (("matpbr_path_render_objects_diff", ()), ("matpbr_path_render_objects_through", (d, d)), ("matpbr_path_render_objects_ratio", (d, d, d))):
        assert path_lib.symbol(name)(*fr[:18], None, None, *tail, *outs, *own) == -1, name
    # the superset entry: exactly one of photo and through, a missing sum, no object
    media = ctypes.cast(good, ctypes.c_void_p)
    assert diff_entry(*fr[:18], None, None, *tail, *outs, d, None, None, media) == -1
    assert diff_entry(*fr[:18], None, None, *tail, *outs, None, d, d, media) == -1
    assert diff_entry(*fr[:18], None, None, *tail, d, None, d, None, None, None, None, media) == -1
    assert diff_entry(*fr[:18], None, None, *tail, *outs, None, None, None, None) == -1       # flagged, media NULL
    assert diff_entry(*fr[:18], None, None, tb, 0, *tail[2:], *outs, None, None, None, media) == -1


def test_object_bsdf_and_merge_scene(path_lib):
    """`object_medium`: both forms, color / at -> sigma_a = -ln(color) / at, the defaults, every refusal; `merge_scene`: the flag, the
    records and the count; the tables that the first-hit, light-table and move entries receive carry no medium flag."""
    om = path_lib.object_medium
    glass = dict(po.GLASS)
    assert om(glass) is None and om(dict(glass, medium=None)) is None
    assert om(dict(glass, medium={})) == (0.0, 0.0, 0.0, 0.0, 0.0)
    assert om(dict(glass, medium={"sigma_a": [1, 2, 3], "scatter": 4, "g": -0.5})) == (1.0, 2.0, 3.0, 4.0, -0.5)
    assert om(dict(glass, medium={"sigma_a": 2.5})) == (2.5, 2.5, 2.5, 0.0, 0.0)
    got = om(dict(pr.FROSTED_02, medium={"color": [0.9, 0.5, 1.0], "at": 0.25, "scatter": 2.0, "g": 0.7}))
    assert np.allclose(got[:3], [-np.log(0.9) / 0.25, -np.log(0.5) / 0.25, 0.0], rtol=1e-15, atol=0) and got[3:] == (2.0, 0.7)
    assert got[2] == 0.0 and not np.signbit(got[2])
    assert np.allclose(om(dict(glass, medium={"color": 0.5, "at": 2.0}))[:3], [np.log(2.0) / 2.0] * 3, rtol=1e-15)
    for bad, words in (({"sigma_a": [1, 2, 3], "color": [0.5] * 3, "at": 1.0}, "not both"), ({"sigma_a": 1.0, "at": 1.0}, "not both"),
                       ({"colour": [0.5] * 3}, "unknown key 'colour'"), ({"color": [0.5] * 3}, "go together"), ({"at": 1.0}, "go together"),
                       ({"color": [0.0, 0.5, 0.5], "at": 1.0}, "(0, 1]"), ({"color": [0.5, 1.5, 0.5], "at": 1.0}, "(0, 1]"),
                       ({"color": [0.5] * 3, "at": 0.0}, "'at' must be"), ({"color": [0.5] * 3, "at": float("inf")}, "'at' must be"),
                       ({"sigma_a": [-1, 0, 0]}, ">= 0"), ({"sigma_a": [0, float("nan"), 0]}, ">= 0"), ({"sigma_a": [1, 2]}, "3 values"),
                       ({"scatter": -0.5}, ">= 0"), ({"scatter": 1e39}, ">= 0"), ({"g": 0.995}, "g must lie"), ({"g": float("nan")}, "g must lie")):
        with pytest.raises(ValueError) as e:
            om(dict(glass, medium=bad))
        assert words in str(e.value), (bad, str(e.value))
    with pytest.raises(ValueError, match="must be a dict"):
        om(dict(glass, medium=[1, 2, 3]))
    for other in (po.DIFFUSE_08, {"type": "pbr"}, {"type": "area", "radiance": 1.0}):
        with pytest.raises(ValueError, match="a medium fills a 'dielectric' or a 'roughdielectric' object"):
            path_lib.object_bsdf(dict(other, medium={"sigma_a": 1.0}))
    assert path_lib.object_bsdf(dict(glass, medium={"sigma_a": 1.0})) == path_lib.object_bsdf(glass)       # the kind returned stays bare
    rm = _groove(10, 12)[0]
    objects = pm.table_scene()
    s = path_lib.merge_scene(rm["vertices"], rm["triangles"], objects, lights=True)
    M = path_lib.OBJECT_MEDIUM
    assert [bool(t.kind & M) for t in s.table] == [True, True, False, False] and len(s.media) == 4
    plain = path_lib.merge_scene(rm["vertices"], rm["triangles"], pr.table_scene())
    assert plain.media is None and not any(t.kind & M for t in plain.table)
    for flags in (0, path_lib.OBJECT_COLORED | path_lib.OBJECT_TEXTURED):
        hidden = path_lib._uncolored(s.table, flags)
        assert [t.kind for t in hidden] == [0x101, 5, 4, 2] and [t.first_tri for t in hidden] == [t.first_tri for t in s.table]
    assert path_lib._uncolored(plain.table, 0) is plain.table


def test_scene_file_medium_key(path_lib, tmp_path):
    """`relight.load_oi_scene`: the entry key "medium" in both forms travels in the entry's bsdf; an object that is not glass, both
    forms at once and an unknown sub-key are a ValueError naming the file and the entry."""
    from materialist_amd import mesh, relight

    V, T = po.cube((0.0, 0.0, -1.0), 0.1, (0.0, 0.0, 0.0))
    mesh.write_ply(str(tmp_path / "cube.ply"), V, T)
    listing = str(tmp_path / "list.json")

    def load(*entries):
        with open(listing, "w") as f:
            json.dump({"objects": [dict({"ply": "cube.ply"}, **e) for e in entries]}, f)
        return relight.load_oi_scene(listing)

    frosted = dict(pr.FROSTED_02)
    out = load({"bsdf": po.GLASS, "medium": {"color": [0.8, 0.4, 0.2], "at": 0.1}}, {"bsdf": frosted, "medium": {"sigma_a": [1, 2, 3], "scatter": 5.0, "g": 0.3}},
               {"bsdf": po.GLASS})
    assert out[0]["bsdf"]["medium"] == {"color": [0.8, 0.4, 0.2], "at": 0.1} and out[0]["bsdf"]["type"] == "dielectric"
    assert np.allclose(path_lib.object_medium(out[0]["bsdf"])[:3], -np.log([0.8, 0.4, 0.2]) / 0.1, rtol=1e-15)
    assert path_lib.object_medium(out[1]["bsdf"]) == (1.0, 2.0, 3.0, 5.0, 0.3) and "medium" not in out[2]["bsdf"]
    for k, entry, words in ((0, {"bsdf": po.DIFFUSE_08, "medium": {"sigma_a": 1.0}}, "a medium fills a 'dielectric' or a 'roughdielectric' object"),
                            (0, {"bsdf": {"type": "area", "radiance": 2.0}, "medium": {"sigma_a": 1.0}}, "a medium fills"),
                            (0, {"bsdf": po.GLASS, "medium": {"sigma_a": [1, 1, 1], "color": [0.5] * 3, "at": 1.0}}, "not both"),
                            (0, {"bsdf": po.GLASS, "medium": {"sigma": 1.0}}, "unknown key 'sigma'"),
                            (0, {"bsdf": po.GLASS, "medium": {"color": [0.5, 0.5, 2.0], "at": 1.0}}, "(0, 1]"),
                            (0, {"bsdf": po.GLASS, "medium": {"color": [0.5] * 3, "at": -1.0}}, "'at' must be"),
                            (0, {"bsdf": dict(po.GLASS, medium={"sigma_a": 1.0}), "medium": {"sigma_a": 1.0}}, "given twice"),
                            (0, {"bsdf": po.GLASS, "mediums": {}}, "unknown key 'mediums'")):
        with pytest.raises(ValueError) as e:
            load(entry)
        assert words in str(e.value) and listing in str(e.value) and f"objects[{k}]" in str(e.value), str(e.value)


def test_command_line_tint_options():
    """`render_final.py --oi_tint` parses to three channels in (0, 1] and refuses --oi_scene beside it, a channel outside the range and
    --oi_tint_at without it."""
    import render_final

    base = ["--save_name", "x", "--mode", "oi"]
    a = render_final.parse_args(base + ["--oi_tint", "0.9", "0.4", "0.1", "--oi_tint_at", "0.2"])
    assert a.oi_tint == [0.9, 0.4, 0.1] and a.oi_tint_at == 0.2
    assert render_final.parse_args(base).oi_tint is None
    for extra in (["--oi_tint", "0.9", "0.0", "0.1"], ["--oi_tint", "0.9", "1.4", "0.1"], ["--oi_tint_at", "0.2"], ["--oi_tint", "0.9", "0.4", "0.1", "--oi_tint_at", "0"],
                  ["--oi_tint", "0.9", "0.4", "0.1", "--oi_scene", "list.json"]):
        with pytest.raises(SystemExit):
            render_final.parse_args(base + extra)
    with pytest.raises(SystemExit):
        render_final.parse_args(["--save_name", "x", "--mode", "real", "--oi_tint", "0.9", "0.4", "0.1"])
