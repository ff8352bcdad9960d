"""Host side of smooth inserted objects ("Smooth inserted objects"): the interpolation and the shading sampler
the kernel runs (on the CPU) against fp64 and at their fallbacks, what the feature is for (the first refraction through an
icosphere against the analytic sphere's), the angle-weighted normals, the PLY reader's normals, the refusals, and the fp64
restatement over the library's fp32 traversal.  No GPU needed."""
import ctypes
import os
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
import path_oi_smooth_fp64 as ps  # noqa: E402
import path_testlib as tl  # noqa: E402

ETA = 1.49 / 1.000277
U_TRANSMIT = 0.99999994          # dim 6 just below 1: transmits wherever anything is transmitted


@pytest.fixture(scope="module")
def path_lib():
    return tl.load()


_report = tl.reporter("path oi smooth", "test_path_oi_smooth_host")


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _about(n, max_deg, rng):
    """unit vectors within max_deg of the unit vectors n [N,3], uniform in angle and azimuth"""
    h = np.where(np.abs(n[:, :1]) < 0.6, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    t = _unit(np.cross(n, h))
    b = np.cross(n, t)
    th, ph = np.radians(rng.uniform(0, max_deg, n.shape[0])), rng.uniform(0, 2 * np.pi, n.shape[0])
    return np.cos(th)[:, None] * n + (np.sin(th) * np.cos(ph))[:, None] * t + (np.sin(th) * np.sin(ph))[:, None] * b


def _triangles_and_rays(N, rng):
    """Well-conditioned lanes, every magnitude O(1): triangles with unit-order edges at 40-140 degrees, hit points inside, rays at
    least 0.2 in cosine off the plane -> fp32 records (v0, e1, e2), o, d and the fp64 values of the same fp32 numbers."""
    v0 = rng.uniform(-1, 1, (N, 3))
    e1 = _unit(rng.normal(size=(N, 3)))
    t = _unit(np.cross(e1, rng.normal(size=(N, 3))))
    ang = np.radians(rng.uniform(40, 140, N))
    e2 = (np.cos(ang)[:, None] * e1 + np.sin(ang)[:, None] * t) * rng.uniform(0.5, 1.5, (N, 1))
    e1 = e1 * rng.uniform(0.5, 1.5, (N, 1))
    bu = rng.uniform(0.02, 0.96, N)
    bv = rng.uniform(0.01, 1.0, N) * (0.98 - bu)
    p = v0 + bu[:, None] * e1 + bv[:, None] * e2
    ng = _unit(np.cross(e1, e2))
    d = _unit(rng.normal(size=(N, 3)))
    c = (d * ng).sum(-1)
    d = _unit(np.where((np.abs(c) < 0.2)[:, None], d + np.sign(c + 1e-30)[:, None] * 0.5 * ng, d))
    o = p - rng.uniform(0.5, 3.0, (N, 1)) * d
    tri = np.stack([v0, e1, e2], 1).astype(np.float32)
    return tri, o.astype(np.float32), d.astype(np.float32)


# ---- 1, 2: the interpolation -----------------------------------------------------------------------------------------------------------
def test_interpolation_matches_fp64(path_lib):
    """1e-5 absolute on u, v and the unit ns: fp32 rounding (6e-8) over a few dozen operations on O(1) magnitudes, with the
    conditioning of `_triangles_and_rays` (|d . ng| >= 0.2, edges at 40-140 degrees) bounding the amplification by about 20."""
    rng = np.random.default_rng(21)
    N = 4096
    tri, o, d = _triangles_and_rays(N, rng)
    t64 = tri.astype(np.float64)
    ng = _unit(np.cross(t64[:, 1], t64[:, 2]))
    cn = (np.stack([_about(ng, 50, rng) for _ in range(3)], 1) * rng.uniform(0.3, 3.0, (N, 3, 1))).astype(np.float32)   # any length
    u, v, ns = path_lib.object_normal_host(tri, cn, o, d)
    P = np.stack([t64[:, 0], t64[:, 0] + t64[:, 1], t64[:, 0] + t64[:, 2]], 1)
    eu, ev = ps.barycentrics(P, o.astype(np.float64), d.astype(np.float64))
    ens, cause = ps.shading_normal(cn.astype(np.float64), eu, ev, ng)
    assert not cause.any() and np.all(eu > 0) and np.all(ev > 0) and np.all(eu + ev < 1)
    worst = max(float(np.abs(u - eu).max()), float(np.abs(v - ev).max()), float(np.abs(ns - ens).max()))
    _report("interpolation (u, v, ns) vs fp64 on 4096 lanes: max abs error (bound 1e-5)", f"{worst:.3e}")
    assert worst <= 1e-5, worst
    # u belongs to the second input vertex and v to the third: a ray at a corner returns that corner's normal
    for corner, (cu, cv) in enumerate(((0.0, 0.0), (1.0, 0.0), (0.0, 1.0))):
        pc = t64[:, 0] + cu * t64[:, 1] + cv * t64[:, 2] + (1 / 3 - cu) * 1e-3 * t64[:, 1] + (1 / 3 - cv) * 1e-3 * t64[:, 2]
        oc = (pc - 2.0 * d.astype(np.float64)).astype(np.float32)
        nsc = path_lib.object_normal_host(tri, cn, oc, d)[2]
        assert np.abs(nsc - _unit(cn[:, corner].astype(np.float64))).max() < 1e-2, corner


def test_interpolation_falls_back_to_the_face_normal(path_lib):
    rng = np.random.default_rng(22)
    N = 512
    tri, o, d = _triangles_and_rays(N, rng)
    t64 = tri.astype(np.float64)
    ng64 = _unit(np.cross(t64[:, 1], t64[:, 2]))
    good = np.stack([_about(ng64, 40, rng) for _ in range(3)], 1).astype(np.float32)
    flat = path_lib.object_normal_host(tri, np.zeros_like(good), o, d)[2]                 # zero sum: the library's own ng, to the last bit
    assert np.abs(flat - ng64).max() < 1e-6
    nan = good.copy()
    nan[::3, 0, 1] = np.nan
    nan[1::3, 1] = np.inf
    nan[2::3, 2, 2] = -np.inf
    zero = good.copy()
    zero[:, 1:] = -0.0
    zero[:, 0] = 0.0
    huge = good * np.float32(3e38)                                  # the sum's squared length overflows
    opposite = -good                                                # ns . ng < 0
    for name, cn in (("nan", nan), ("zero", zero), ("overflow", huge), ("ns.ng<0", opposite)):
        ns = path_lib.object_normal_host(tri, cn, o, d)[2]
        assert np.array_equal(ns.view(np.uint32), flat.view(np.uint32)), name
    # corner normals that cancel at the hit point: n0 = n1 = n2 rotated so that the weighted sum is 0 only where u = v = 1/3
    tng = _unit(np.cross(ng64, [0.3, -0.5, 0.8]))
    cancel = np.stack([tng, -0.5 * tng + 0.75 ** 0.5 * np.cross(ng64, tng), -0.5 * tng - 0.75 ** 0.5 * np.cross(ng64, tng)], 1)
    centre = t64[:, 0] + (t64[:, 1] + t64[:, 2]) / 3
    ns = path_lib.object_normal_host(tri, cancel.astype(np.float32), (centre - 2.0 * d).astype(np.float32), d)[2]
    assert np.isfinite(ns).all()
    dots = (ns * ng64).sum(-1)                                      # in the tangent plane: ns . ng is rounding, and <= 0 falls back
    assert np.all((np.abs(dots - 1) < 1e-6) | (dots > 0))
    # perpendicular to ng exactly: ns . ng = 0 is a fallback too
    ez = np.tile(np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), (4, 1, 1))
    side = np.tile(np.float32([1, 0, 0]), (4, 3, 1))
    ns = path_lib.object_normal_host(ez, side, np.tile(np.float32([0.25, 0.25, 1]), (4, 1)), np.tile(np.float32([0, 0, -1]), (4, 1)))[2]
    assert np.array_equal(ns, np.tile(np.float32([0, 0, 1]), (4, 1)))
    # the third fallback lives in the sampler: ns and ng on opposite sides of wo -> the ng event
    n = np.float32([0, 0, 1])
    tilt = np.float32([-np.sin(1.0), 0, np.cos(1.0)])               # 57 degrees towards -x
    wo = _unit(np.float32([[np.cos(0.2), 0, np.sin(0.2)]])).repeat(64, 0)   # 11 degrees above the face on the +x side: ns . wo < 0
    assert (tilt * wo[0]).sum() < 0 < (n * wo[0]).sum()
    u = rng.random((64, 3)).astype(np.float32)
    for bsdf in (po.GLASS, po.DIFFUSE_08):
        got = path_lib.object_sample_shading_host(bsdf, n, tilt, wo, u)
        ref = path_lib.object_sample_host(bsdf, n, wo, u)
        for g, e in zip(got, ref):
            assert np.array_equal(g, e), bsdf["type"]


# ---- 3, 4: the shading sampler --------------------------------------------------------------------------------------------------------
def test_sampler_with_the_face_normal_is_the_flat_sampler(path_lib):
    rng = np.random.default_rng(23)
    n = _unit(np.float32([0.36, -0.48, 0.8]))
    N = 2048
    wo = _unit(rng.normal(size=(N, 3))).astype(np.float32)
    assert ((wo * n).sum(-1) > 0).sum() > 500 and ((wo * n).sum(-1) < 0).sum() > 500
    u = rng.random((N, 3)).astype(np.float32)
    for bsdf in (po.GLASS, {"type": "diffuse", "reflectance": (0.8, 0.55, 0.3)}):
        got = path_lib.object_sample_shading_host(bsdf, n, n, wo, u)
        ref = path_lib.object_sample_host(bsdf, n, wo, u)
        for name, g, e in zip(("wi", "weight", "pdf", "flags"), got, ref):
            assert np.array_equal(g.view(np.uint32), e.view(np.uint32)), (bsdf["type"], name)


def test_sampler_agrees_with_the_geometry(path_lib):
    """8192 random lanes, ns within 60 degrees of ng, wo on both sides (entering with eta = 1.49 / 1.000277, leaving with its
    reciprocal)."""
    rng = np.random.default_rng(24)
    N = 8192
    ng = _unit(rng.normal(size=(N, 3)))
    ns = _about(ng, 60, rng)
    wo = _unit(rng.normal(size=(N, 3)))
    ng32, ns32, wo32 = (_unit(x).astype(np.float32) for x in (ng, ns, wo))
    u = rng.random((N, 3)).astype(np.float32)
    g64, w64 = ng32.astype(np.float64), wo32.astype(np.float64)
    go = (g64 * w64).sum(-1)
    assert (go > 0.05).sum() > 3000 and (go < -0.05).sum() > 3000
    wi, w, pdf, flags = path_lib.object_sample_shading_host(po.GLASS, ng32, ns32, wo32, u)
    gi = (g64 * wi.astype(np.float64)).sum(-1)
    clear = np.abs(gi * go) > 1e-6                                   # a sign decided in fp32 is checked where fp64 cannot disagree
    crossed = gi * go < 0
    transmitted = (flags & 2) != 0
    assert np.all((flags & 1) == 1) and clear.mean() > 0.999
    assert np.array_equal(transmitted[clear], crossed[clear])
    assert transmitted.sum() > 2000 and (~transmitted).sum() > 300
    eta_ti2 = np.where(go > 0, 1 / ETA ** 2, ETA ** 2)
    assert np.all(w[~transmitted] == 1.0)
    np.testing.assert_allclose(w[transmitted], eta_ti2[transmitted, None].repeat(3, 1), rtol=1e-5)
    np.testing.assert_allclose(np.linalg.norm(wi, axis=-1), 1.0, atol=1e-5)
    # how often the event about ns had to be redone about ng (from the fp64 restatement of the same lanes)
    ns_eff = ps.shading_normal(np.repeat(ns32.astype(np.float64)[:, None], 3, 1), np.full(N, 1 / 3), np.full(N, 1 / 3), g64, w64)[0]
    redo = ps.sample_dielectric_shading(1.49, 1.000277, g64, ns_eff, w64, u[:, 0].astype(np.float64))[4]
    _report("dielectric lanes redone about ng / with ns replaced by ng (of 8192)", f"{int(redo.sum())} / {int((ns_eff == g64).all(-1).sum())}")
    assert redo.sum() > 50
    # diffuse: nothing is carried below the face, nothing from behind it
    rho = (0.8, 0.55, 0.3)
    wi, w, pdf, flags = path_lib.object_sample_shading_host({"type": "diffuse", "reflectance": rho}, ng32, ns32, wo32, u)
    gi = (g64 * wi.astype(np.float64)).sum(-1)
    carried = (w > 0).any(-1)
    assert np.all(flags == 0) and np.all(gi[carried] > 0) and np.all(go[carried] > 0)
    assert np.array_equal(w[carried], np.broadcast_to(np.float32(rho), w[carried].shape))
    below = (go > 0.05) & ~carried
    assert below.sum() > 100 and carried.sum() > 2000                # sampled about ns, some directions dip below ng: their paths end
    np.testing.assert_allclose(pdf[carried], np.maximum((wi[carried] * ns_eff[carried]).sum(-1), 0) / np.pi, atol=1e-5)
    # constructed: ns . wo > 0 and ng . wo > 0, but the mirror about ns dips below ng -> the ng event, bit for bit
    n = np.float32([0, 0, 1])
    tilt = np.float32([-np.sin(np.radians(50)), 0, np.cos(np.radians(50))])
    az = rng.uniform(-0.3, 0.3, 64)
    wo_c = np.stack([np.sin(np.radians(30)) * np.cos(az), np.sin(np.radians(30)) * np.sin(az), np.full(64, np.cos(np.radians(30)))], -1).astype(np.float32)
    mirror = 2 * (wo_c @ tilt)[:, None] * tilt - wo_c
    assert np.all(wo_c @ tilt > 0) and np.all(mirror[:, 2] < -0.1)
    uc = np.stack([np.zeros(64), rng.random(64), rng.random(64)], -1).astype(np.float32)   # dim 6 = 0: reflect
    got = path_lib.object_sample_shading_host(po.GLASS, n, tilt, wo_c, uc)
    ref = path_lib.object_sample_host(po.GLASS, n, wo_c, uc)
    for g, e in zip(got, ref):
        assert np.array_equal(g, e)
    assert np.all(got[0][:, 2] > 0) and np.all(got[3] == 1)


# ---- 5: what the feature is for --------------------------------------------------------------------------------------------------------
def _records_by_id(bvh):
    raw = bvh["tris"].reshape(-1, 48)
    ids = raw.view(np.int32).reshape(-1, 12)[:, 3]
    rec = np.empty((ids.size, 3, 3), np.float32)
    rec[ids] = raw.view(np.float32).reshape(-1, 3, 4)[:, :, :3]
    return rec


def test_first_refraction_through_an_icosphere(path_lib):
    """Level 2 (320 triangles), exact radial corner normals: the first refracted direction of camera rays against the analytic
    sphere's.  The flat facets' error is first order in the facet angle, the interpolated normal's second order."""
    centre, radius = np.array([0.02, -0.01, -1.2]), 0.25
    V, T, U = ps.icosphere(centre, radius, 2)
    assert T.shape[0] == 320
    bvh = path_lib.build_bvh(V, T, 0)
    H = W = 48
    f = (W / 2.0) / np.tan(np.radians(pf.FOV) / 2.0)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = _unit(np.stack([(x - (W - 1) / 2) / f, -(y - (H - 1) / 2) / f, -np.ones_like(x)], -1).reshape(-1, 3)).astype(np.float32)
    o = np.zeros_like(d)
    t, k = path_lib.trace_host(bvh, o, d)
    hit = k >= 0
    assert hit.sum() > 300
    d, o, k = d[hit], o[hit], k[hit]
    rec = _records_by_id(bvh)[k]
    u, v, ns = path_lib.object_normal_host(rec, U[T][k], o, d)
    ng = path_lib.object_normal_host(rec, np.zeros((k.size, 3, 3), np.float32), o, d)[2]     # zero normals: the face normal
    uu = np.tile(np.float32([U_TRANSMIT, 0.5, 0.5]), (k.size, 1))
    smooth = path_lib.object_sample_shading_host(po.GLASS, ng, ns, -d, uu)
    flat = path_lib.object_sample_shading_host(po.GLASS, ng, ng, -d, uu)
    # the analytic sphere: the nearer root of |t d - c|^2 = r^2
    d64 = d.astype(np.float64)
    b = d64 @ centre
    ts = b - np.sqrt(b * b - centre @ centre + radius * radius)
    nsph = (ts[:, None] * d64 - centre) / radius
    ref = po.sample_dielectric(1.49, 1.000277, nsph, -d64, np.full(k.size, U_TRANSMIT))
    ok = ref[3] & ((smooth[3] & 2) != 0) & ((flat[3] & 2) != 0)
    assert ok.sum() > 300
    ang = lambda w: np.degrees(np.arccos(np.clip((w.astype(np.float64) * ref[0]).sum(-1), -1, 1)))[ok]
    es, ef = ang(smooth[0]), ang(flat[0])
    line = (f"mean {es.mean():.3f} / {ef.mean():.3f} degrees (ratio {ef.mean() / es.mean():.1f}), 95th percentile "
            f"{np.percentile(es, 95):.3f} / {np.percentile(ef, 95):.3f} degrees (ratio {np.percentile(ef, 95) / np.percentile(es, 95):.1f}), {int(ok.sum())} rays")
    _report("first refraction through a 320-triangle icosphere, error against the analytic sphere, smooth / flat", line)
    assert es.mean() < ef.mean() and np.percentile(es, 95) < np.percentile(ef, 95)


# ---- 6: angle-weighted normals ---------------------------------------------------------------------------------------------------------
def test_angle_weighted_normals():
    from materialist_amd import mesh

    V, T, U = ps.icosphere((0.3, -0.2, -1.0), 0.4, 2)
    Nn = mesh.angle_weighted_normals(V, T)
    np.testing.assert_allclose(np.linalg.norm(Nn, axis=-1), 1.0, atol=1e-12)
    fn = _unit(np.cross(V[T[:, 1]] - V[T[:, 0]], V[T[:, 2]] - V[T[:, 0]]))
    cone = max(float(np.degrees(np.arccos(np.clip((fn * U[T[:, c]]).sum(-1), -1, 1))).max()) for c in range(3))
    off = np.degrees(np.arccos(np.clip((Nn * U).sum(-1), -1, 1)))
    _report("angle-weighted normals on the 320-triangle icosphere: largest angle to the radial direction / the cone's", f"{off.max():.3f} / {cone:.3f} degrees")
    assert off.max() <= cone + 1e-9                                   # a weighted mean of vectors stays inside their cone
    Vc, Tc = po.cube((0.1, 0.2, -1.0), 0.3, (0.0, 0.0, 0.0))
    Nc = mesh.angle_weighted_normals(Vc, Tc)
    np.testing.assert_allclose(Nc, _unit(Vc - Vc.mean(0)), atol=1e-12)   # the corner diagonal, whichever way each face is split
    # winding-oriented (not camera-oriented), and 0 where nothing adds up
    np.testing.assert_allclose(mesh.angle_weighted_normals(Vc, Tc[:, ::-1]), -Nc, atol=1e-12)
    lone = mesh.angle_weighted_normals(np.r_[Vc, [[9.0, 9.0, 9.0]]], Tc)
    assert np.all(lone[-1] == 0) and np.allclose(lone[:-1], Nc, atol=1e-12)
    fold = mesh.angle_weighted_normals(np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.array([[0, 1, 2], [0, 2, 1]]))
    assert np.all(fold == 0)


# ---- 7: the PLY reader -----------------------------------------------------------------------------------------------------------------
def test_read_ply_any_returns_the_files_normals(tmp_path):
    from materialist_amd import mesh

    V, T, U = ps.icosphere((0.0, 0.1, -1.0), 0.2, 0)
    V = V.astype(np.float32).astype(np.float64)
    Nn = (U * 2.5).astype(np.float32).astype(np.float64)             # as written: not normalised by the reader
    faces = "".join(f"3 {a} {b} {c}\n" for a, b, c in T.tolist())
    head = lambda fmt, props: (f"ply\nformat {fmt} 1.0\nelement vertex {V.shape[0]}\n" + "".join(f"property {t} {n}\n" for t, n in props) +
                               f"element face {T.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
    with_n = [("float", "x"), ("float", "y"), ("float", "z"), ("uchar", "red"), ("float", "nx"), ("float", "ny"), ("float", "nz"), ("double", "s")]
    without = [("float", "x"), ("float", "y"), ("float", "z"), ("uchar", "red")]
    paths = {}
    for name, props in (("with", with_n), ("without", without)):
        p = str(tmp_path / f"ascii_{name}.ply")
        with open(p, "w") as fh:
            fh.write(head("ascii", props))
            for v, n in zip(V.tolist(), Nn.tolist()):
                fh.write(f"{v[0]!r} {v[1]!r} {v[2]!r} 200" + (f" {n[0]!r} {n[1]!r} {n[2]!r} 0.25" if name == "with" else "") + "\n")
            fh.write(faces)
        paths["ascii_" + name] = p
        p = str(tmp_path / f"binary_{name}.ply")
        dt = np.dtype([(n, "<" + {"float": "f4", "uchar": "u1", "double": "f8"}[t]) for t, n in props])
        rec = np.zeros(V.shape[0], dt)
        rec["x"], rec["y"], rec["z"], rec["red"] = V[:, 0], V[:, 1], V[:, 2], 200
        if name == "with":
            rec["nx"], rec["ny"], rec["nz"], rec["s"] = Nn[:, 0], Nn[:, 1], Nn[:, 2], 0.25
        fr = np.empty(T.shape[0], dtype=[("n", "u1"), ("v", "<i4", (3,))])
        fr["n"], fr["v"] = 3, T
        with open(p, "wb") as fh:
            fh.write(head("binary_little_endian", props).encode("ascii") + rec.tobytes() + fr.tobytes())
        paths["binary_" + name] = p
    for key, p in paths.items():
        plain = mesh.read_ply_any(p)
        assert isinstance(plain, tuple) and len(plain) == 2, key      # the default call is today's
        assert np.array_equal(plain[0], V) and np.array_equal(plain[1], T) and plain[0].dtype == np.float64 and plain[1].dtype == np.int32
        got = mesh.read_ply_any(p, normals=True)
        assert len(got) == 3 and np.array_equal(got[0], V) and np.array_equal(got[1], T), key
        if key.endswith("without"):
            assert got[2] is None, key
        else:
            assert got[2].shape == V.shape and got[2].dtype == np.float64 and np.array_equal(got[2], Nn), key
    # a file with only two of the three components has no normals
    p = str(tmp_path / "two.ply")
    with open(p, "w") as fh:
        fh.write(head("ascii", [("float", "x"), ("float", "y"), ("float", "z"), ("float", "nx"), ("float", "ny")]))
        fh.write("".join(f"{v[0]!r} {v[1]!r} {v[2]!r} 0 1\n" for v in V.tolist()) + faces)
    assert mesh.read_ply_any(p, normals=True)[2] is None


# ---- 8: the refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_smooth_flag(path_lib, tmp_path):
    import render_final
    from materialist_amd import relight

    Vs = np.array([[0.0, 0.0, -2.0], [1.0, 0.0, -2.0], [0.0, 1.0, -2.0]])
    Ts = np.array([[0, 1, 2]], np.int32)
    V, T, U = ps.icosphere((0.0, 0.0, -1.0), 0.2, 0)
    ball = {"vertices": V, "triangles": T, "bsdf": po.GLASS}
    Vc, Tc = po.cube((0.3, 0.0, -1.0), 0.1, (0.1, 0.2, 0.3))
    flat = {"vertices": Vc, "triangles": Tc, "bsdf": po.DIFFUSE_08}
    # the table: the flag on the smooth object alone, corner normals in triangle order, normalised, zero for the flat object
    out = path_lib.merge_objects(Vs, Ts, [flat, dict(ball, normals=3.0 * U)], normals=True)
    assert len(out) == 4 and len(path_lib.merge_objects(Vs, Ts, [flat, dict(ball, normals=U)])) == 3
    table, corner = out[2], out[3]
    assert table[0].kind == path_lib.BSDF_DIFFUSE and table[1].kind == path_lib.BSDF_DIELECTRIC | path_lib.OBJECT_SMOOTH == 0x101
    assert (table[1].first_tri, table[1].n_tri) == (13, 20)
    assert corner.dtype == np.float32 and corner.shape == (32, 3, 3) and np.all(corner[:12] == 0)
    assert np.array_equal(corner[12:], U[T].astype(np.float32))
    assert path_lib.merge_objects(Vs, Ts, [flat, ball], normals=True)[3] is None
    for bad, word in ((U[:-1], "normals must be"), (U.reshape(-1), "normals must be"), (np.where(np.arange(12)[:, None] == 3, np.nan, U), "finite"),
                      (np.where(np.arange(12)[:, None] == 5, np.inf, U), "finite"), (np.where(np.arange(12)[:, None] == 7, 0.0, U), "zero length")):
        with pytest.raises(ValueError, match="object 1") as e:
            path_lib.merge_objects(Vs, Ts, [flat, dict(ball, normals=bad)])
        assert word in str(e.value), (word, str(e.value))
    # a zero normal at a vertex no triangle uses is nobody's business
    V2, U2 = np.r_[V, [[5.0, 5.0, 5.0]]], np.r_[U, [[0.0, 0.0, 0.0]]]
    assert path_lib.merge_objects(Vs, Ts, [dict(ball, vertices=V2, normals=U2)], normals=True)[3].shape == (20, 3, 3)
    # the C ABI: argument checks come before any GPU work
    lib = path_lib.load()
    one = np.zeros(1, np.float32)
    P = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    head = [P(one)] * 5 + [4, 4, 35.0] + [P(one)] * 4 + [2, 4, 1, 4, 0, 1, P(one), None, None]
    smooth = (path_lib.PathObject * 1)(path_lib.PathObject(0x101, 1, 20, (ctypes.c_float * 3)(1.49, 1.0, 0.0)))
    plain = (path_lib.PathObject * 1)(path_lib.PathObject(1, 1, 20, (ctypes.c_float * 3)(1.49, 1.0, 0.0)))
    tab = lambda t: ctypes.cast(t, ctypes.c_void_p)
    assert lib.matpbr_path_render_objects(*head, tab(smooth), 1) == -1                        # the flag is an unknown kind there
    assert lib.matpbr_path_render_objects_normals(*head, tab(smooth), 1, None, 1) == -1       # a flagged object needs its normals
    assert lib.matpbr_path_render_objects_normals(*head, tab(smooth), 1, P(one), 2) == -1     # a range that starts below n_scene_tri
    assert lib.matpbr_path_render_objects_normals(*head, tab(plain), 1, None, 2) == -1
    assert lib.matpbr_path_render_objects_normals(*head, tab(smooth), 1, P(one), -1) == -1
    bad_kind = (path_lib.PathObject * 1)(path_lib.PathObject(0x103, 1, 20, (ctypes.c_float * 3)(1.49, 1.0, 0.0)))
    assert lib.matpbr_path_render_objects_normals(*head, tab(bad_kind), 1, P(one), 1) == -1
    with pytest.raises(path_lib.PathError, match="matpbr_path_no_such_symbol"):
        path_lib.symbol("matpbr_path_no_such_symbol")
    # the command line and relight
    a = render_final.parse_args(["--save_name", "case", "--mode", "oi", "--oi_normals", "vertex"])
    assert a.oi_normals == "vertex" and render_final.parse_args(["--save_name", "case", "--mode", "oi"]).oi_normals == "flat"
    with pytest.raises(SystemExit):
        render_final.parse_args(["--save_name", "case", "--mode", "oi", "--oi_normals", "smooth"])
    os.makedirs(tmp_path / "case")
    (tmp_path / "case" / "oi.ply").write_text("ply\n")
    with pytest.raises(ValueError, match="object_normals"):
        relight.render_oi("case", input_path=str(tmp_path), save_path=str(tmp_path), object_normals="smooth")


# ---- 9: the restatement ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table(path_lib):
    """The GPU test's scene: the groove at 24 x 20 with `path_oi_smooth_fp64.table_scene` in front of it."""
    from materialist_amd import mesh

    H, W = 20, 24
    rm = mesh.reference_mesh(pf.groove_scene(H, W), pf.FOV)
    rng = np.random.default_rng(11)
    a, r, m = pf.groove_maps(H, W, rng)
    env = pf.groove_env(rng)
    objects = ps.table_scene()
    V, T, tab = pob.merged(rm["vertices"], rm["triangles"], objects)
    return {"rm": rm, "a": a, "r": r, "m": m, "env": env, "tab": path_lib.env_tables(env), "H": H, "W": W, "objects": objects, "V": V, "T": T,
            "table": tab}


def test_restatement_without_normals_is_the_flat_restatement(table, oracle64):
    g = table
    objects = po.two_cubes()
    V, T, tab = po.merged(g["rm"]["vertices"], g["rm"]["triangles"], objects)
    for seed, depth in ((0, 6), (4, 16)):
        args = (oracle64, V, T, g["a"], g["r"], g["m"], g["env"], g["tab"], g["H"], g["W"], depth, seed, tab)
        ref, rec0 = po.replay_oi(*args)
        got, rec1 = pob.replay_objects(*args)
        assert np.array_equal(ref, got)
        assert all(np.array_equal(rec0[k], rec1[k]) for k in ("transmitted", "diffuse_object", "blocked_by_object"))
        assert not any(rec1[k].any() for k in ("smooth_transmitted", "smooth_diffuse", "redo", "fallback"))


def test_restatement_over_fp32_and_fp64_traversal(table, path_lib, oracle64):
    """The GPU criterion's cap: the restatement over the library's fp32 traversal and over the fp64 brute force may differ in at
    most 1 % of the pixels of each of the six renders.  On this scene they differ in none (reported)."""
    g = table
    Vm, Tm, _, corner = path_lib.merge_objects(g["rm"]["vertices"], g["rm"]["triangles"], g["objects"], normals=True)
    n_scene = g["rm"]["triangles"].shape[0]
    assert corner.shape == (Tm.shape[0] - n_scene, 3, 3)
    # the corner normals the library holds are the restatement's
    got = np.concatenate([c if c is not None else np.zeros((len(ob["triangles"]), 3, 3)) for c, ob in
                          ((ps.corner_normals(ob), ob) for ob in g["objects"])])
    assert np.array_equal(corner.astype(np.float64), got)
    bvh = path_lib.build_bvh(Vm, Tm, n_scene)

    def closest(o, d):
        t, k = path_lib.trace_host(bvh, o, d)
        return np.where(k < 0, np.inf, t.astype(np.float64)), k.astype(np.int64)

    occluded = lambda o, d: path_lib.trace_host(bvh, o, d)[1] >= 0
    seen = {k: 0 for k in ("smooth_transmitted", "smooth_diffuse", "blocked_by_object", "redo", "fallback")}
    differ = []
    for max_depth in (6, 16):
        for seed in (0, 1, 2):
            args = (oracle64, g["V"], g["T"], g["a"], g["r"], g["m"], g["env"], g["tab"], g["H"], g["W"], max_depth, seed, g["table"])
            L64, rec = pob.replay_objects(*args)
            L32, _ = pob.replay_objects(*args, closest=closest, occluded=occluded)
            err = (np.abs(L32 - L64) / np.maximum(np.abs(L64), np.abs(L64).mean())).max(-1)
            differ.append(int((err > 1e-3).sum()))
            assert differ[-1] <= 0.01 * g["H"] * g["W"], (max_depth, seed, differ[-1])
            for k in ("smooth_transmitted", "smooth_diffuse", "blocked_by_object"):
                assert rec[k].any(), (k, max_depth, seed)           # the scene does what it is for, in every one of the renders
            for k in seen:
                seen[k] += int(rec[k].sum())
    assert seen["redo"] >= 1 and seen["fallback"] >= 1
    _report("restatement over fp32 vs fp64 traversal: pixels that differ in each of the six renders (cap 4 of 480)", differ)
    _report("pixels with a smooth transmitted vertex / a smooth diffuse vertex / a blocked emitter sample / a redo / a fallback (6 renders)",
            " / ".join(str(seen[k]) for k in seen))
