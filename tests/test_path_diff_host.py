"""The differential render on the CPU ("Differential render"; no GPU): the filtered traversal of
`matpbr_path_trace_scene_host` against a BVH of the scene alone, `matpbr_path_composite_host` against the same expression in numpy
float32, the header against the binding, and the refusals of `render_oi(composite=True)` and of the command line before any GPU work."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import path_diff_fp64 as pd  # noqa: E402
import path_fp64 as pf  # noqa: E402
import path_testlib as tl  # noqa: E402
import path_texture_fp64 as px  # noqa: E402

FOV = pf.FOV
_report = tl.reporter("path diff host", "test_path_diff_host")


@pytest.fixture(scope="module")
def path_lib():
    return tl.load()


# ---- 0 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_header_declares_what_the_binding_binds(path_lib):
    with open(os.path.join(ROOT, "include", "matpbr_path.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(matpbr_path_\w+)\s*\(", text))
    assert set(path_lib.DIFF_SYMBOLS) <= declared and set(path_lib.DIFF_SYMBOLS) <= set(path_lib.LATE_SYMBOLS)
    lib = path_lib.load()
    for name in path_lib.DIFF_SYMBOLS:
        fn = path_lib.symbol(name, lib)
        assert fn.argtypes == path_lib.SIGNATURES[name][1] and fn.restype == path_lib.SIGNATURES[name][0], name
    P = ctypes.c_void_p
    # matpbr_path_render_objects_textures' arguments without `out`, then fg, delta, alpha, rewalked
    tex = path_lib.SIGNATURES["matpbr_path_render_objects_textures"][1]
    assert path_lib.SIGNATURES["matpbr_path_render_objects_diff"][1] == tex[:18] + tex[19:] + [P] * 4
    assert path_lib.SIGNATURES["matpbr_path_trace_scene_host"][1] == path_lib.SIGNATURES["matpbr_path_trace_host"][1] + [ctypes.c_long, ctypes.c_int]
    assert path_lib.SIGNATURES["matpbr_path_composite"][1] == path_lib.SIGNATURES["matpbr_path_composite_host"][1] + [P]
    assert lib.matpbr_path_version() == path_lib.VERSION == 3
    # a library from before the feature: PathError through symbol(), naming the entry and the feature

    class Old:
        pass

    with pytest.raises(path_lib.PathError, match="matpbr_path_render_objects_diff.*differential render"):
        path_lib.symbol("matpbr_path_render_objects_diff", Old())


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_filtered_trace_is_the_trace_of_the_scene_alone(path_lib):
    """On the merged BVH of the texture scene over the groove at 24 x 20, for 4096 rays that start on the camera side of the sheet:
    with the limit at n_scene_tri the filtered traversal names the triangle and the bits of t that `trace_host` gives over a BVH of the
    scene alone, for at least 0.999 of the rays (the others are ties on shared edges, which another tree visits in another order);
    with the limit at the triangle count it is `trace_host` over the merged BVH exactly; any-hit agrees with closest-hit on occlusion."""
    from materialist_amd import mesh

    H, W = 20, 24
    rm = mesh.reference_mesh(pf.groove_scene(H, W), FOV)
    n_scene = rm["triangles"].shape[0]
    Vm, Tm, _ = path_lib.merge_objects(rm["vertices"], rm["triangles"], px.table_scene())
    merged, alone = path_lib.build_bvh(Vm, Tm, n_scene), path_lib.build_bvh(rm["vertices"], rm["triangles"])
    rng = np.random.default_rng(5)
    N = 4096
    # half the rays leave the camera as the render's do, half start between the camera and the sheet (z in [-1, 0]; the sheet lies
    # beyond z = -2) in any direction: bounce and shadow rays among the objects
    o = np.zeros((N, 3), np.float32)
    o[N // 2:] = np.stack([rng.uniform(-0.3, 0.3, N // 2), rng.uniform(-0.3, 0.3, N // 2), rng.uniform(-1.6, -0.8, N // 2)], -1)
    d = rng.normal(size=(N, 3))
    d[:N // 2] = np.stack([rng.uniform(-0.3, 0.3, N // 2), rng.uniform(-0.25, 0.25, N // 2), -np.ones(N // 2)], -1)
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    t_ref, k_ref = path_lib.trace_host(alone, o, d)
    t_got, k_got = path_lib.trace_scene_host(merged, o, d, n_scene)
    t_all, k_all = path_lib.trace_host(merged, o, d)
    assert (k_ref >= 0).mean() > 0.5 and (k_all >= n_scene).mean() > 0.05 and (k_got < n_scene).all()
    same = (k_got == k_ref) & (t_got.view(np.uint32) == t_ref.view(np.uint32))
    _report(f"filtered trace against the scene's own BVH over {N} rays ({int((k_all >= n_scene).sum())} of them stopped by an object unfiltered): "
            f"rays that differ (bound {N // 1000})", int((~same).sum()))
    assert same.mean() >= 0.999
    # the distances of the few that differ are still the same surface's
    assert np.allclose(t_got[~same], t_ref[~same], rtol=1e-5)
    t_lim, k_lim = path_lib.trace_scene_host(merged, o, d, Tm.shape[0])
    assert np.array_equal(k_lim, k_all) and np.array_equal(t_lim.view(np.uint32), t_all.view(np.uint32))
    t_big, k_big = path_lib.trace_scene_host(merged, o, d, 2 ** 40)
    assert np.array_equal(k_big, k_all) and np.array_equal(t_big.view(np.uint32), t_all.view(np.uint32))
    # any-hit: the same rays are occluded, each by a scene triangle that the ray does meet no nearer than the closest one
    t_any, k_any = path_lib.trace_scene_host(merged, o, d, n_scene, any=True)
    assert np.array_equal(k_any >= 0, k_got >= 0) and (k_any < n_scene).all()
    hit = k_any >= 0
    assert (t_any[hit] >= t_got[hit]).all()
    t_any_all, k_any_all = path_lib.trace_scene_host(merged, o, d, Tm.shape[0], any=True)
    assert np.array_equal(k_any_all >= 0, k_all >= 0)
    # a limit of 0 leaves nothing to hit; the refusals
    assert (path_lib.trace_scene_host(merged, o, d, 0)[1] == -1).all()
    with pytest.raises(path_lib.PathError):
        path_lib.trace_scene_host(merged, o, d, -1)
    fn = path_lib.symbol("matpbr_path_trace_scene_host")
    t, k = np.empty(N, np.float32), np.empty(N, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    args = [p(merged["nodes"]), p(merged["tris"]), p(o), p(d), N, 0.0, 3.0e38, p(t), p(k), n_scene, 0]
    assert fn(*args) == 0
    for j, bad in ((0, None), (1, None), (2, None), (3, None), (4, -1), (7, None), (8, None), (9, -1), (10, 2), (10, -1)):
        assert fn(*(bad if i == j else x for i, x in enumerate(args))) == -1, j


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
def _composite_numpy(fg, delta, alpha, photo, scale):
    sc, one, zero = np.float32(scale), np.float32(1), np.float32(0)
    return np.maximum(zero, (fg + delta) * sc + (one - alpha[..., None] * sc) * photo)


@pytest.mark.parametrize("shape", [(1, 1), (5, 7), (20, 24)])
def test_composite_host_is_the_expression_in_float32(path_lib, shape):
    H, W = shape
    rng = np.random.default_rng(H * 100 + W)
    for frames in (1, 3, 10):
        alpha = rng.uniform(0, frames, (H, W)).astype(np.float32)
        alpha.reshape(-1)[::3] = 0.0                                    # untouched, covered in every frame, fractions
        alpha.reshape(-1)[1::3] = frames
        fg = (rng.gamma(2.0, 0.5, (H, W, 3)) * alpha[..., None]).astype(np.float32)
        delta = rng.normal(0.0, 0.3, (H, W, 3)).astype(np.float32)      # shadows are negative
        delta[0, 0, 0] = -abs(delta[0, 0, 0]) - 0.01
        photo = rng.gamma(2.0, 0.5, (H, W, 3)).astype(np.float32)
        got = path_lib.composite_host(fg, delta, alpha, photo, 1.0 / frames)
        ref = _composite_numpy(fg, delta, alpha, photo, 1.0 / frames)
        assert got.dtype == np.float32 and got.shape == (H, W, 3)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), frames
        assert (delta < 0).any() and (got >= 0).all()
    # the clamp: a shadow deeper than the photograph is bright gives 0, not a negative value
    dark = path_lib.composite_host(np.zeros((H, W, 3), np.float32), np.full((H, W, 3), -5.0, np.float32), np.zeros((H, W), np.float32), photo, 1.0)
    assert not dark.view(np.uint32).any()
    # nothing touched: the photograph's bits
    zeros3, zeros1 = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32)
    for scale in (1.0, 0.1, 1.0 / 3):
        assert np.array_equal(path_lib.composite_host(zeros3, zeros3, zeros1, photo, scale).view(np.uint32), photo.view(np.uint32))


def test_composite_refusals(path_lib):
    H, W = 3, 4
    z3, z1 = np.zeros((H, W, 3), np.float32), np.zeros((H, W), np.float32)
    for scale in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="scale"):
            path_lib.composite_host(z3, z3, z1, z3, scale)
    with pytest.raises(ValueError, match="alpha"):
        path_lib.composite_host(z3, z3, z3, z3)
    with pytest.raises(ValueError, match="delta"):
        path_lib.composite_host(z3, z1, z1, z3)
    with pytest.raises(ValueError, match="photo"):
        path_lib.composite_host(z3, z3, z1, z1)
    out = np.empty((H, W, 3), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    host = path_lib.symbol("matpbr_path_composite_host")
    args = [p(z3), p(z3), p(z1), p(z3), H, W, 1.0, p(out)]
    assert host(*args) == 0
    cases = [(0, None), (1, None), (2, None), (3, None), (4, 0), (5, -2), (6, 0.0), (6, -0.5), (6, float("inf")), (6, float("nan")), (7, None)]
    for j, bad in cases:
        assert host(*(bad if i == j else x for i, x in enumerate(args))) == -1, (j, bad)
    # the device entry refuses the same before it launches anything (no GPU is touched by a refused call)
    dev = path_lib.symbol("matpbr_path_composite")
    for j, bad in cases:
        assert dev(*(bad if i == j else x for i, x in enumerate(args)), None) == -1, (j, bad)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
def _scene_with_cube(tmp):
    from materialist_amd import mesh

    scene = tl.synthetic_output(tmp)
    ob = pd.cube_object(pd.VISIBLE_CUBE)
    mesh.write_ply(os.path.join(scene, "oi2.ply"), ob["vertices"].astype(np.float32), ob["triangles"])
    return scene


def test_render_oi_composite_refuses_before_any_gpu_work(path_lib, tmp_path):
    """Every refusal is raised with device="nowhere": a call that reached the maps' upload or a tracer would fail on the device's name."""
    from PIL import Image

    from materialist_amd import relight
    from materialist_amd.imageio_exr import write_exr

    tmp = str(tmp_path)
    scene = _scene_with_cube(tmp)
    kw = dict(input_path=tmp, save_path=tmp, spp=4, n_iter=2, device="nowhere", composite=True)
    with pytest.raises(ValueError, match="gt_image.exr does not exist"):
        relight.render_oi("case", **kw)
    with pytest.raises(ValueError, match="elsewhere.exr does not exist"):
        relight.render_oi("case", photo_path=os.path.join(tmp, "elsewhere.exr"), **kw)
    photo = np.random.default_rng(1).uniform(0, 1, (32, 32, 3)).astype(np.float32)
    write_exr(os.path.join(scene, "gt_image.exr"), photo)
    with pytest.raises(ValueError, match="atrous"):
        relight.render_oi("case", denoise="atrous", **kw)
    for env_scale in (0.0, 0.5, 2.0):
        with pytest.raises(ValueError, match="env_scale 1"):
            relight.render_oi("case", env_scale=env_scale, **kw)
    small = os.path.join(tmp, "small.exr")
    write_exr(small, photo[:16])
    with pytest.raises(ValueError, match=r"must be \[32,32,3\]"):
        relight.render_oi("case", photo_path=small, **kw)
    png = os.path.join(tmp, "wide.png")
    Image.fromarray(np.zeros((32, 40, 3), np.uint8), "RGB").save(png)
    with pytest.raises(ValueError, match=r"must be \[32,32,3\]"):
        relight.render_oi("case", photo_path=png, **kw)
    bad = photo.copy()
    bad[3, 4, 1] = -0.25
    write_exr(os.path.join(tmp, "negative.exr"), bad)
    with pytest.raises(ValueError, match="finite and >= 0"):
        relight.render_oi("case", photo_path=os.path.join(tmp, "negative.exr"), **kw)
    # the photograph as the composite takes it: an .exr as written, a .png decoded as the pipeline decodes its input
    assert np.array_equal(relight._oi_photo(scene, None, False, 1.0), photo)
    ok = os.path.join(tmp, "ok.png")
    px8 = np.random.default_rng(2).integers(0, 256, (32, 32, 3), dtype=np.uint8)
    Image.fromarray(px8, "RGB").save(ok)
    assert np.allclose(relight._oi_photo(scene, ok, False, 1.0), (px8 / 255.0) ** 2.2, rtol=1e-5, atol=1e-7)
    # without `composite` nothing of this is looked at: the call goes on to the device's name
    with pytest.raises(Exception) as e:
        relight.render_oi("case", input_path=tmp, save_path=tmp, spp=4, n_iter=2, device="nowhere", photo_path=small)
    assert not isinstance(e.value, ValueError) or "photograph" not in str(e.value)


def test_cli_parses_and_refuses_before_any_gpu_work(tmp_path):
    sys.path.insert(0, ROOT)
    import render_final

    base = ["--save_name", "case", "--mode", "oi"]
    a = render_final.parse_args(base)
    assert a.oi_composite is False and a.oi_photo is None
    a = render_final.parse_args(base + ["--oi_composite", "--oi_photo", "shot.exr"])
    assert a.oi_composite is True and a.oi_photo == "shot.exr"
    for extra in (["--oi_composite", "--denoise", "atrous"], ["--oi_composite", "--env_scale", "0.5"], ["--oi_photo", "shot.exr"]):
        with pytest.raises(SystemExit):
            render_final.parse_args(base + extra)
    with pytest.raises(SystemExit):
        render_final.parse_args(["--save_name", "case", "--mode", "real", "--oi_composite"])
    # the whole command: a missing photograph ends it with the refusal, before a device is asked for
    tmp = str(tmp_path)
    _scene_with_cube(tmp)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "render_final.py"), "--save_name", "case", "--input_path", tmp, "--save_path", tmp,
                          "--mode", "oi", "--spp", "4", "--oi_iters", "2", "--oi_composite"], capture_output=True, text=True, timeout=600)
    assert res.returncode != 0 and "gt_image.exr does not exist" in res.stderr
