"""Host side of the denoiser ("Denoiser"): the per-pixel routines the kernels run (on the CPU) against the fp64
restatement at every pixel, the properties that follow from the definition, the first-hit features against the library's traversal
plus fp64 normals, the refusals, and the gain on a synthetic image.  No GPU needed."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import denoise_fp64 as dn  # noqa: E402
import path_fp64 as pf  # noqa: E402
import path_normal_fp64 as pn  # noqa: E402
import path_oi_smooth_fp64 as ps  # noqa: E402
import path_testlib as tl  # noqa: E402

FOV = pf.FOV


@pytest.fixture(scope="module")
def path_lib():
    return tl.load()


_report = tl.reporter("denoise", "test_denoise_host")


# ---- 1: single steps against fp64 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", dn.SHAPES)
def test_prepare_and_every_level_match_fp64(path_lib, H, W):
    """Every pixel: |c - c64| <= 1e-4 max|c_in|, |v - v64| <= 1e-4 max v_in.  A tap that matters has a total exponent of order 10,
    which fp32 carries to a few 1e-6, and the output is a ratio of such sums: 1e-4 leaves more than a decade.  Measured worst case
    over the four shapes: prepare 5.4e-8 / 3.0e-7, levels 1.1e-6 (colour) and 9.0e-7 (variance)."""
    x = dn.random_inputs(H, W)
    assert set(np.unique(x["geom"][..., 7])) == {-1.0, 0.0, 1.0, 2.0} and (x["cv"][..., 3] == 0).any()
    got = path_lib.denoise_prepare_host(x["A"], x["B"], x["geom"]).astype(np.float64)
    ref = dn.prepare(x["A"], x["B"], x["geom"])
    c_in = max(float(np.abs(x["A"]).max()), float(np.abs(x["B"]).max()))
    vraw = (dn.lum(x["A"]) - dn.lum(x["B"])) ** 2 / 4
    v_in = float(vraw.max())
    assert (vraw == 0).any()                                         # exact zeros among the raw variances
    ec, ev = float(np.abs(got[..., :3] - ref[..., :3]).max()) / c_in, float(np.abs(got[..., 3] - ref[..., 3]).max()) / v_in
    _report(f"prepare {H}x{W}: worst colour / variance error relative to the largest input", (ec, ev))
    assert ec <= 1e-4 and ev <= 1e-4
    c_in, v_in = float(np.abs(x["cv"][..., :3]).max()), float(x["cv"][..., 3].max())
    for l in range(5):
        got = path_lib.denoise_level_host(x["cv"], x["geom"], x["alb"], l).astype(np.float64)
        ref = dn.level(x["cv"], x["geom"], x["alb"], l)
        ec, ev = float(np.abs(got[..., :3] - ref[..., :3]).max()) / c_in, float(np.abs(got[..., 3] - ref[..., 3]).max()) / v_in
        _report(f"level {l} {H}x{W}: worst colour / variance error relative to the largest input", (ec, ev))
        assert ec <= 1e-4 and ev <= 1e-4, (l, ec, ev)
        moved = float(np.abs(ref[..., :3] - x["cv"][..., :3].astype(np.float64)).max()) / c_in
        _report(f"level {l} {H}x{W}: largest change of a colour relative to the largest input", moved)
        assert l > 0 or moved > 1e-2, (l, moved)                    # the level filters: neighbours carry weight


def _chain_host(path_lib, A, B, geom, alb, **params):
    cv = path_lib.denoise_prepare_host(A, B, geom)
    for l in range(params.get("levels", 5)):
        cv = path_lib.denoise_level_host(cv, geom, alb, l, **params)
    return cv[..., :3]


# ---- 2: properties -----------------------------------------------------------------------------------------------------------------------
def test_a_constant_image_is_a_fixed_point(path_lib):
    x = dn.random_inputs(36, 20)
    const = np.broadcast_to(np.float32([0.7, 0.25, 1.3]), (36, 20, 3))
    out = _chain_host(path_lib, const, const, x["geom"], x["alb"])
    worst = float(np.abs(out / const - 1).max())
    _report("constant image: worst relative change", worst)
    assert worst <= 1e-6


def test_equal_halves_return_the_input(path_lib):
    """A == B: every variance is 0 and the colour term's 1e-3 lum keeps each pixel within 1e-3 of the input's maximum."""
    s = dn.synthetic()
    t32 = s["truth"].astype(np.float32)
    out = _chain_host(path_lib, t32, t32, s["geom"], s["alb"])
    worst = float(np.abs(out - t32).max() / t32.max())
    _report("A == B on the synthetic image: worst change relative to the maximum", worst)
    assert worst <= 1e-3


@pytest.mark.parametrize("k", [3, -2])
def test_scaling_by_a_power_of_two_scales_the_output_exactly(path_lib, k):
    x = dn.random_inputs(24, 24)
    f = np.float32(2.0 ** k)
    one = _chain_host(path_lib, x["A"], x["B"], x["geom"], x["alb"])
    scaled = _chain_host(path_lib, x["A"] * f, x["B"] * f, x["geom"], x["alb"])
    assert np.array_equal((one * f).view(np.uint32), scaled.view(np.uint32))


def test_every_output_is_a_convex_combination_within_its_id(path_lib):
    H, W = 36, 20
    x = dn.random_inputs(H, W)
    ids = x["geom"][..., 7]
    assert len(np.unique(ids)) >= 3
    rng = np.random.default_rng(5)
    level_of = np.float32([0.1, 1.0, 5.0, 20.0])[(ids + 1).astype(int)][..., None]      # each id its own range of values
    A = (level_of * rng.gamma(0.5, 2.0, size=(H, W, 3))).astype(np.float32)              # strong noise
    B = (level_of * rng.gamma(0.5, 2.0, size=(H, W, 3))).astype(np.float32)
    out = _chain_host(path_lib, A, B, x["geom"], x["alb"]).astype(np.float64)
    mean = ((A.astype(np.float64) + B) / 2)
    worst = dn.convex_hull_violation(out, mean, ids)
    _report("convex hull per id under strong noise: worst excess relative to the largest input", worst)
    assert worst <= 1e-6
    assert float(np.abs(out - mean).max()) > 0.1 * float(mean.max())          # and it did filter


# ---- 3: features ---------------------------------------------------------------------------------------------------------------------------
def library_rays(H, W):
    """The rays through the pixel centres as the library forms them, in fp32: [H*W,3]."""
    th = math.tan(0.5 * FOV * 3.14159265358979323846 / 180.0)
    f_pix, cx, cy = np.float32((0.5 * W) / th), np.float32(0.5) * np.float32(W - 1), np.float32(0.5) * np.float32(H - 1)
    i, j = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    d = np.stack([(j - cx) / f_pix, -((i - cy) / f_pix), -np.ones_like(i)], -1).reshape(-1, 3)
    il = np.float32(1.0) / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    return (d * il[:, None]).astype(np.float32)


def feature_reference(pathtrace, oracle64, V, T, n_scene, table, corner, H, W, nrm_map=None):
    """geom in fp64 from the library's own closest hits (`trace_host`, rays through the pixel centres): the hit point on the winning
    triangle's plane, the footprint, and the normal the render shades the camera vertex with."""
    bvh = pathtrace.build_bvh(V, T, n_scene if table else None)
    d32 = library_rays(H, W)
    _, tri = pathtrace.trace_host(bvh, np.zeros_like(d32), d32)
    d = d32.astype(np.float64)
    V32 = np.asarray(V, np.float64).astype(np.float32).astype(np.float64)
    geom = np.zeros((H * W, 8))
    geom[:, 7] = -1
    hit = np.nonzero(tri >= 0)[0]
    P = V32[np.asarray(T)[tri[hit]]]
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    ng = np.cross(e1, e2)
    ng /= np.linalg.norm(ng, axis=-1, keepdims=True)
    scene = tri[hit] < n_scene
    ng[scene] *= -np.sign((ng[scene] * P[scene, 0]).sum(-1))[:, None]      # the depth mesh faces the camera
    t = (ng * P[:, 0]).sum(-1) / (ng * d[hit]).sum(-1)
    p = t[:, None] * d[hit]
    n = ng.copy()
    ids = np.zeros(hit.shape[0])
    for k, ob in enumerate(table):
        own = (tri[hit] >= ob.first_tri) & (tri[hit] < ob.first_tri + ob.n_tri)
        ids[own] = 1 + k
        if ob.kind & pathtrace.OBJECT_SMOOTH and own.any():
            cn = corner[tri[hit][own] - n_scene].astype(np.float64)
            u, v = ps.barycentrics(P[own], np.zeros((int(own.sum()), 3)), d[hit][own])
            n[own] = ps.shading_normal(cn, u, v, ng[own], -d[hit][own])[0]
    if nrm_map is not None:
        tp = pf.texel(oracle64, p[scene], H, W)
        n[scene] = nrm_map.reshape(-1, 3).astype(np.float64)[tp]
    geom[hit, :3], geom[hit, 3] = p, np.linalg.norm(p, axis=-1) * 2.0 * math.tan(math.radians(FOV) / 2.0) / W
    geom[hit, 4:7], geom[hit, 7] = n, ids
    return geom.reshape(H, W, 8), bvh


@pytest.mark.parametrize("H,W", [(20, 36), (9, 17), (36, 20), (17, 9)])
def test_features_match_the_traversal_and_fp64_normals(path_lib, oracle64, H, W):
    for name, V, T, n_scene, table, corner, nmap in dn.feature_scenes(path_lib, H, W):
        ref, bvh = feature_reference(path_lib, oracle64, V, T, n_scene, table, corner, H, W, nmap)
        got = path_lib.features_host(bvh, H, W, FOV, table, corner, n_scene, nmap)
        ids = set(np.unique(ref[..., 7]))
        assert ids >= ({0.0, 1.0, 2.0, 3.0} if table and min(H, W) > 9 else {0.0}), (name, ids)      # the scene shows what it is for
        dn.check_features(got, ref, f"{name} {H}x{W}", _report)


# ---- 4: argument checks -------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused(path_lib):
    lib = path_lib.load()
    x = dn.random_inputs(17, 9)
    P, ptr = ctypes.c_void_p, lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = np.empty((17, 9, 4), np.float32)
    good = path_lib.PathDenoise(5, 32.0, 1.0, 0.1, 4.0)
    level = lambda prm, cv=x["cv"], geom=x["geom"], alb=x["alb"], o=out, l=0: lib.matpbr_path_denoise_level_host(
        None if cv is None else ptr(cv), None if geom is None else ptr(geom), None if alb is None else ptr(alb), 17, 9,
        None if prm is None else ctypes.cast(ctypes.byref(prm), P), l, None if o is None else ptr(o))
    assert level(good) == 0
    bad = [path_lib.PathDenoise(0, 32.0, 1.0, 0.1, 4.0), path_lib.PathDenoise(9, 32.0, 1.0, 0.1, 4.0), path_lib.PathDenoise(5, 0.0, 1.0, 0.1, 4.0),
           path_lib.PathDenoise(5, 32.0, -1.0, 0.1, 4.0), path_lib.PathDenoise(5, 32.0, 1.0, float("nan"), 4.0),
           path_lib.PathDenoise(5, 32.0, 1.0, 0.1, float("inf"))]
    for prm in bad + [None]:
        assert level(prm) == -1, prm and (prm.levels, prm.sigma_n, prm.sigma_x, prm.sigma_a, prm.sigma_c)
    for kw in ({"cv": None}, {"geom": None}, {"alb": None}, {"o": None}, {"l": -1}, {"l": 8}):
        assert level(good, **kw) == -1, kw
    assert lib.matpbr_path_denoise_prepare_host(None, ptr(x["B"]), ptr(x["geom"]), 17, 9, ptr(out)) == -1
    assert lib.matpbr_path_denoise_prepare_host(ptr(x["A"]), ptr(x["B"]), ptr(x["geom"]), 17, 9, None) == -1
    assert lib.matpbr_path_denoise_prepare_host(ptr(x["A"]), ptr(x["B"]), ptr(x["geom"]), 0, 9, ptr(out)) == -1
    # the device entry points check before they launch anything: no GPU is touched by a refusal
    assert lib.matpbr_path_denoise(None, None, None, None, 17, 9, ctypes.cast(ctypes.byref(good), P), None, None, 0, None) == -1
    assert lib.matpbr_path_denoise(ptr(x["A"]), ptr(x["B"]), ptr(x["geom"]), ptr(x["alb"]), 17, 9, ctypes.cast(ctypes.byref(bad[0]), P), ptr(out),
                                   ptr(out), 1 << 20, None) == -1
    assert lib.matpbr_path_denoise(ptr(x["A"]), ptr(x["B"]), ptr(x["geom"]), ptr(x["alb"]), 17, 9, ctypes.cast(ctypes.byref(good), P), ptr(out),
                                   ptr(out), 16, None) == -1                       # a workspace too small
    assert lib.matpbr_path_denoise_workspace_bytes(17, 9) == 2 * 17 * 9 * 16 and lib.matpbr_path_denoise_workspace_bytes(0, 9) == 0
    assert lib.matpbr_path_features(None, None, 17, 9, 35.0, None, 0, None, 0, None, None, None) == -1
    assert lib.matpbr_path_features_host(None, None, 17, 9, 35.0, None, 0, None, 0, None, ptr(out)) == -1
    assert lib.matpbr_path_denoise_level(None, None, None, 17, 9, ctypes.cast(ctypes.byref(good), P), 0, None, None) == -1
    assert lib.matpbr_path_denoise_prepare(None, None, None, 17, 9, None, None) == -1


def test_the_python_wrappers_refuse_wrong_shapes_and_parameters(path_lib):
    x = dn.random_inputs(17, 9)
    with pytest.raises(ValueError, match="A must be"):
        path_lib.denoise_prepare_host(x["A"][:-1], x["B"], x["geom"])
    with pytest.raises(ValueError, match="geom must be"):
        path_lib.denoise_prepare_host(x["A"], x["B"], x["geom"][..., :7])
    with pytest.raises(ValueError, match="alb must be"):
        path_lib.denoise_level_host(x["cv"], x["geom"], x["alb"][:, :-1], 0)
    with pytest.raises(ValueError, match="cv must be"):
        path_lib.denoise_level_host(x["cv"][..., :3], x["geom"], x["alb"], 0)
    with pytest.raises(ValueError, match="level"):
        path_lib.denoise_level_host(x["cv"], x["geom"], x["alb"], 8)
    with pytest.raises(ValueError, match="levels"):
        path_lib.denoise_level_host(x["cv"], x["geom"], x["alb"], 0, levels=0)
    with pytest.raises(ValueError, match="sigma_a"):
        path_lib.denoise_level_host(x["cv"], x["geom"], x["alb"], 0, sigma_a=0.0)
    with pytest.raises(ValueError, match="normal must be"):
        from materialist_amd import mesh

        rm = mesh.reference_mesh(pf.groove_scene(17, 9), FOV)
        path_lib.features_host(path_lib.build_bvh(rm["vertices"], rm["triangles"]), 17, 9, FOV, normal=np.zeros((9, 17, 3), np.float32))


# ---- 5: the gain -----------------------------------------------------------------------------------------------------------------------------
def test_the_denoised_image_is_closer_to_the_truth(path_lib):
    """Relative RMSE of the plain average over the denoised one, at spp 4, 16 and 64: at least 2 (the fp64 prototype of the definition
    gave 5.0, 4.9, 4.8; the margin is for the fp32 host path and retuned defaults).  Measured with the fp32 host path and the
    defaults (5 levels, sigma 32 / 1 / 0.1 / 4): 5.04, 4.86, 4.78."""
    s = dn.synthetic()
    rng = np.random.default_rng(0)
    ratios = []
    for spp in (4, 16, 64):
        A, B = dn.noisy_halves(s["truth"], spp, rng)
        out = _chain_host(path_lib, A, B, s["geom"], s["alb"])
        plain, den = dn.rel_rmse((A.astype(np.float64) + B) / 2, s["truth"]), dn.rel_rmse(out, s["truth"])
        _report(f"synthetic 64x80 spp {spp}: relative RMSE plain, denoised, ratio", (plain, den, plain / den))
        ratios.append(plain / den)
    assert min(ratios) >= 2.0, ratios


def test_an_older_library_names_the_missing_symbol(path_lib):
    """The binding looks the denoiser's symbols up by name: a library built before them raises PathError naming the one asked for."""
    class Older:                                                     # a loaded library without the new entry points
        pass

    for name in path_lib.DENOISE_SYMBOLS:
        assert name in path_lib.SIGNATURES and hasattr(path_lib.load(), name)
        with pytest.raises(path_lib.PathError, match=name + ".*denoiser"):
            path_lib.symbol(name, Older())
