"""Relighting in the photograph on the GPU (libmatpbr_path.so's `matpbr_path_render_relight` and `matpbr_path_composite_relight`,
DESIGN.md section 1.4, "Relighting in the photograph"): both radiances of the one walk against `render` under each envmap and against
the two fp64 replays of `path_relight_fp64`, the bits where the two envmaps are one, the ray count, envmaps of two sizes, launch
splits, the composite against its CPU twin, the transfer where the fit is off, and `render_final.py --relight_composite`."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import path_diff_fp64 as pd  # noqa: E402
import path_fp64 as pf  # noqa: E402
import path_relight_fp64 as pr  # noqa: E402
import path_testlib as tl  # noqa: E402
from path_testlib import bits as _bits  # noqa: E402

pytestmark = pytest.mark.gpu

FOV = pf.FOV
_report = tl.reporter("path relight", "test_gpu_path_relight")
_f64 = lambda x: x.cpu().numpy().astype(np.float64)


@pytest.fixture(scope="module")
def pt():
    return tl.load(gpu=True)


@pytest.fixture(scope="module")
def scene(pt):
    """The groove at 24 x 20 with its envmaps (`path_relight_fp64.relight_scene`), its tracer, and the plain renders the cases share,
    each computed once."""
    s = pr.relight_scene(pt)
    s["tracer"] = pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], s["H"], s["W"], FOV)
    s["maps"] = (s["a"], s["r"], s["m"])
    s["plain"] = {}
    return s


def _plain(s, env, spp, max_depth, seed, normal=False, rays=False):
    """`render` under s[env] -> (the image, its ray counts), kept in the scene."""
    key = (env, spp, max_depth, seed, normal)
    if key not in s["plain"]:
        n = torch.zeros(s["H"], s["W"], dtype=torch.int32, device=s["tracer"].device)
        img = s["tracer"].render(*s["maps"], s[env], spp=spp, max_depth=max_depth, seed=seed, rays=n, normal=s["nrm"] if normal else None)
        s["plain"][key] = (img, n)
    return s["plain"][key]


def _relight(s, b, spp, max_depth, seed, normal=False, **kw):
    base, relit = s["tracer"].render_relight(*s["maps"], s["env"], s[b], spp=spp, max_depth=max_depth, seed=seed,
                                             normal=s["nrm"] if normal else None, **kw)
    assert base.shape == (s["H"], s["W"], 3) and relit.shape == base.shape and base.dtype == relit.dtype == torch.float32
    return base, relit


def _against_render(s, b, spp, max_depth, seed, normal=False):
    """Item 1's criterion: base against render(A) and relit against render(B), `path_testlib.parity` share 1.0."""
    base, relit = _relight(s, b, spp, max_depth, seed, normal)
    name = f"{'normal map, ' if normal else ''}{b} max_depth {max_depth} seed {seed} spp {spp}"
    for what, got, env in (("base against render(A)", base, "env"), ("relit against render(B)", relit, b)):
        want = _plain(s, env, spp, max_depth, seed, normal)[0]
        frac, err = tl.parity(_f64(got), _f64(want))
        same = float((_bits(got) == _bits(want)).all(-1).mean())
        _report(f"{name}: {what}, largest error; share of bit-equal pixels", f"{err.max():.3e}; {same:.4f}")
        assert frac == 1.0, (what, max_depth, seed, err.max())
    return base, relit


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_depth", [2, 4, 16])
def test_both_radiances_are_the_renders(pt, scene, max_depth):
    for seed in (0, 1):
        base, relit = _against_render(scene, "env_b", 3, max_depth, seed)
        assert tl.parity(_f64(relit), _f64(base))[0] < 0.5                        # and the two lights are two


def test_both_radiances_are_the_renders_under_the_normal_map(pt, scene):
    base, _ = _against_render(scene, "env_b", 3, 4, 0, normal=True)
    assert tl.parity(_f64(base), _f64(_plain(scene, "env", 3, 4, 0)[0]))[0] < 0.5   # the map reaches the kernel


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_depth", [4, 16])
def test_both_radiances_match_fp64(pt, scene, oracle64, max_depth):
    """spp 1 against the two replays (whose walks `reference` asserts equal): at least 0.99 of the pixels within 1e-3, the project's
    per-walk share."""
    ref = pr.reference(oracle64, scene, max_depth, 0)
    base, relit = _relight(scene, "env_b", 1, max_depth, 0)
    for what, got, want in (("base", base, ref["base"]), ("relit", relit, ref["relit"])):
        frac, err = tl.parity(_f64(got), want)
        _report(f"max_depth {max_depth} seed 0: {what} against its fp64 replay, share of pixels within 1e-3",
                f"{frac:.4f} ({int((err > 1e-3).sum())} pixels beyond, max err {err.max():.3e})")
        assert frac >= 0.99, (what, max_depth, frac)


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_one_envmap_twice_gives_one_radiance_twice(pt, scene):
    """B = A: relit has base's bits everywhere, whether B is A's arrays or copies of them with tables built on their own; the composite
    is then the photograph, bit for bit."""
    s = scene
    tracer = s["tracer"]
    photo = np.random.default_rng(3).gamma(2.0, 0.5, (s["H"], s["W"], 3)).astype(np.float32)
    photo[1, 2] = 0.0
    for max_depth, seed, normal in ((4, 0, False), (16, 3, False), (4, 1, True)):
        kw = dict(spp=3, max_depth=max_depth, seed=seed, normal=s["nrm"] if normal else None)
        base, relit = tracer.render_relight(*s["maps"], s["env"], s["env"], **kw)
        assert np.array_equal(_bits(base), _bits(relit)) and bool(base.any())
        tabs = tracer.tables(s["env"])
        copies = tracer.tables(s["env"].copy())
        assert all(x.data_ptr() != y.data_ptr() for x, y in zip(tabs, copies))
        base2, relit2 = tracer.render_relight(*s["maps"], s["env"], s["env"].copy(), tables=tabs, new_tables=copies, **kw)
        assert np.array_equal(_bits(base2), _bits(base)) and np.array_equal(_bits(relit2), _bits(base))
        for floor in (None, 0.3):
            assert np.array_equal(_bits(pt.composite_relight(base, relit, photo, floor=floor)), photo.view(np.uint32))


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_depth, seed", [(4, 0), (16, 1)])
def test_the_rays_are_the_closest_hits_once_and_each_lights_shadow_rays(pt, scene, max_depth, seed):
    """Per pixel and exactly: rays(relight A, B) = rays(render A) + rays(render B) - rays(render Z), Z the all-zero envmap, which has no
    tables and so traces the closest hits alone.  With B = Z relit is all zero bits and the rays are render(A)'s."""
    s = scene
    dev = s["tracer"].device
    spp = 3
    n_a, n_b, n_z = (_plain(s, env, spp, max_depth, seed)[1] for env in ("env", "env_b", "env_zero"))
    assert bool((n_a > n_z).any()) and int(n_z.min()) >= spp
    n = torch.zeros(s["H"], s["W"], dtype=torch.int32, device=dev)
    _relight(s, "env_b", spp, max_depth, seed, rays=n)
    wrong = int((n != n_a + n_b - n_z).sum())
    _report(f"max_depth {max_depth} seed {seed} spp {spp}: rays of the walk; of render(A) + render(B); saved; pixels off the identity",
            f"{int(n.sum())}; {int(n_a.sum() + n_b.sum())}; {int(n_z.sum())}; {wrong}")
    assert wrong == 0
    n = torch.zeros_like(n)
    base, relit = _relight(s, "env_zero", spp, max_depth, seed, rays=n)
    assert not _bits(relit).any() and bool(base.any())
    assert torch.equal(n, n_a)
    assert tl.parity(_f64(base), _f64(_plain(s, "env", spp, max_depth, seed)[0]))[0] == 1.0


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_envmaps_of_two_sizes(pt, scene):
    assert scene["env"].shape == (8, 16, 3) and scene["env_small"].shape == (4, 8, 3)
    for max_depth, seed in ((4, 0), (16, 1)):
        _against_render(scene, "env_small", 3, max_depth, seed)


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normal", [False, True])
def test_launch_splits_give_the_same_bits(pt, scene, normal):
    whole = _relight(scene, "env_b", 5, 16, 7, normal, spp_per_launch=8)
    assert bool(whole[0].any()) and bool(whole[1].any())
    for split in (1, 2, 5):
        part = _relight(scene, "env_b", 5, 16, 7, normal, spp_per_launch=split)
        for k, (x, y) in enumerate(zip(whole, part)):
            assert np.array_equal(_bits(x), _bits(y)), (split, k)


def test_the_raw_call(pt, scene):
    """`PathTracer.render_relight` is the raw call; the outputs start from whatever they held; `rays` is added to; a tracer with objects
    refuses."""
    s = scene
    tracer, dev = s["tracer"], s["tracer"].device
    whole = _relight(s, "env_small", 5, 4, 2, spp_per_launch=2)
    keep = tracer._inputs(*s["maps"], s["env"], None)
    tabs_b = tracer.tables(s["env_small"])
    base, relit = torch.full((s["H"], s["W"], 3), 7.0, device=dev), torch.full((s["H"], s["W"], 3), -7.0, device=dev)
    rays = torch.zeros(s["H"], s["W"], dtype=torch.int32, device=dev)
    args = (*tracer._frame(*keep, 5, 4, 2, 2), rays.data_ptr(), torch.cuda.current_stream().cuda_stream, *(x.data_ptr() for x in tabs_b), 4, 8, None)
    fn = pt.symbol("matpbr_path_render_relight")
    for _ in range(2):
        assert fn(*args, base.data_ptr(), relit.data_ptr()) == 0
    for k, (x, y) in enumerate(zip(whole, (base, relit))):
        assert np.array_equal(_bits(x), _bits(y)), k
    once = torch.zeros_like(rays)
    _relight(s, "env_small", 5, 4, 2, rays=once)
    assert torch.equal(rays, 2 * once)
    for k in (0, 1):
        ptrs = [base.data_ptr(), relit.data_ptr()]
        ptrs[k] = None
        assert fn(*args, *ptrs) == -1, k
    objects = pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], s["H"], s["W"], FOV, objects=[pd.cube_object(pd.HIDDEN_CUBE)])
    with pytest.raises(ValueError, match="objects"):
        objects.render_relight(*s["maps"], s["env"], s["env_b"], spp=1)


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_composite_has_the_host_twins_bits(pt, scene):
    s = scene
    base, relit = _relight(s, "env_b", 4, 4, 6)
    photo = np.random.default_rng(3).gamma(2.0, 0.5, (s["H"], s["W"], 3)).astype(np.float32)
    b, r = base.cpu().numpy(), relit.cpu().numpy()
    for scale, floor in ((1.0, 0.05), (0.5, 1e-3), (1.0, None)):
        if floor is None:                                                          # the default, formed from the same base on each side
            floor = float(np.float32(0.01 * scale * b.mean(dtype=np.float64)))
            dflt = pt.composite_relight(base, relit, photo, scale)
            assert np.array_equal(_bits(dflt), pt.composite_relight_host(b, r, photo, scale).view(np.uint32))
        got = pt.composite_relight(base, relit, torch.from_numpy(photo).to(base.device), scale, floor)
        host = pt.composite_relight_host(b, r, photo, scale, floor)
        assert np.array_equal(_bits(got), host.view(np.uint32)), (scale, floor)
        assert (_bits(got) != photo.view(np.uint32)).any() and bool(torch.isfinite(got).all()) and bool((got >= 0).all())


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_transfer_helps_where_the_fit_is_off(pt, scene):
    """spp 16, max_depth 4, seed 0.  The true maps T are the groove's; the "fit" F is T with the albedo halved.  Photograph =
    render(T, A), target = render(T, B).  The mean absolute error of composite_relight(render_relight(F, A, B), photograph) is at most
    0.25 x that of render(F, B), the picture the command writes without the composite.  The fp64 restatement gives 2.87e-2 against
    1.83e-1, a quotient of 0.157; the photograph left as it is gives 1.80e-1."""
    s = scene
    tracer = s["tracer"]
    kw = dict(spp=16, max_depth=4, seed=0)
    T, F = s["a"], s["a"] * np.float32(0.5)
    photo = tracer.render(T, s["r"], s["m"], s["env"], **kw)
    target = _f64(tracer.render(T, s["r"], s["m"], s["env_b"], **kw))
    rerender = tracer.render(F, s["r"], s["m"], s["env_b"], **kw)
    base, relit = tracer.render_relight(F, s["r"], s["m"], s["env"], s["env_b"], **kw)
    mae = lambda img: float(np.abs(_f64(img) - target).mean())
    ours, today, nothing = mae(pt.composite_relight(base, relit, photo)), mae(rerender), mae(photo)
    _report("fitted albedo 0.5 x true, A -> A rolled, spp 16: mean |composite - target|; mean |re-render - target|; their quotient; the photograph "
            "left as it is", f"{ours:.3e}; {today:.3e}; {ours / today:.3f}; {nothing:.3e}")
    assert ours <= 0.25 * today


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_render_final_cli_relight_composite(pt, tmp_path):
    """`render_final.py --integrator path --relight_composite --spp 4` in a child process on a synthetic output at 32 x 32 with a
    gt_image.exr written here.  `--mode real --env_path B`: the .exr has the bits of the in-process composite.  `--mode rolling --frames 2
    --rotation_step 90`: frame 0 is the photograph's PNG and frame 1 is not.  `--denoise atrous` runs, and under the fitted envmap
    itself it returns the photograph's bits."""
    from materialist_amd import loss, relight
    from materialist_amd.imageio_exr import read_exr, write_exr
    from materialist_amd.imageio_hdr import write_hdr
    from materialist_amd.pipeline import load_image, write_png

    tmp = str(tmp_path)
    scene_dir = tl.synthetic_output(tmp)
    photo = np.random.default_rng(4).gamma(2.0, 0.3, (32, 32, 3)).astype(np.float32)
    write_exr(os.path.join(scene_dir, "gt_image.exr"), photo)
    fitted = os.path.join(scene_dir, "best_results", "envmap.hdr")
    new = os.path.join(tmp, "turned.hdr")
    write_hdr(new, np.ascontiguousarray(np.roll(load_image(fitted), 5, axis=1)))
    cmd = [sys.executable, os.path.join(ROOT, "render_final.py"), "--save_name", "case", "--input_path", tmp, "--save_path", tmp,
           "--integrator", "path", "--relight_composite", "--spp", "4"]

    def run(*extra):
        res = subprocess.run(cmd + list(extra), capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout + res.stderr

    def exr(name):
        assert os.path.exists(os.path.join(tmp, "case", name + ".png"))
        return np.ascontiguousarray(read_exr(os.path.join(tmp, "case", name + ".exr"))[..., :3], dtype=np.float32)

    run("--mode", "real", "--env_path", new)
    img = exr("mi_rc_case_turned_")
    assert not os.path.exists(os.path.join(tmp, "case", "mi_case_turned_.exr"))
    mat = relight.load_estimated_brdf(os.path.join(scene_dir, "best_results"), "cuda")
    tracer = relight._path_tracer(scene_dir, "case", mat, "cuda")
    base, relit = tracer.render_relight(mat["albedo"], mat["roughness"], mat["metallic"], load_image(fitted), load_image(new), spp=4, max_depth=4, seed=0)
    assert np.array_equal(img.view(np.uint32), _bits(pt.composite_relight(base, relit, photo)))
    assert (img != photo).any(-1).mean() > 0.9 and np.isfinite(img).all() and (img >= 0).all()

    run("--mode", "rolling", "--frames", "2", "--rotation_step", "90")
    from PIL import Image

    frames = [np.asarray(Image.open(os.path.join(tmp, "case", "rolling_rc_animation", f"frame_{k:04d}.png"))) for k in (0, 1)]
    want = os.path.join(tmp, "photo.png")
    write_png(want, loss.linear_to_srgb(torch.from_numpy(photo).cuda().clamp_min(0)).clamp(0, 1).cpu().numpy())
    assert np.array_equal(frames[0], np.asarray(Image.open(want))) and (frames[1] != frames[0]).any()
    for ext in (".mp4", ".gif"):
        assert os.path.exists(os.path.join(tmp, "case", "rolling_rc_case_envmap" + ext))
    assert not os.path.exists(os.path.join(tmp, "case", "rolling_envmap_animation"))

    run("--mode", "real", "--env_path", fitted, "--denoise", "atrous")
    assert np.array_equal(exr("mi_rc_case_envmap_").view(np.uint32), photo.view(np.uint32))
