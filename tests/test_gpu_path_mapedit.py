"""Material edits in the photograph on the GPU (libmatpbr_path.so's `matpbr_path_render_edit_diff`, DESIGN.md section 1.4, "Material
edits in the photograph"): both walks against the two fp64 replays of `path_mapedit_fp64`, exact zeros and the touch rule bracketed
from both sides, the same walk twice, nothing and everything edited against `render`, launch splits, shading normals, the photograph's
bits under both composites, the ratio transfer where the fit is off, and `render_final.py --edit_composite`."""
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
import path_mapedit_fp64 as pm  # noqa: E402
import path_testlib as tl  # noqa: E402
from path_testlib import bits as _bits  # noqa: E402

pytestmark = pytest.mark.gpu

FOV = pf.FOV
_report = tl.reporter("path mapedit", "test_gpu_path_mapedit")


@pytest.fixture(scope="module")
def pt():
    return tl.load(gpu=True)


@pytest.fixture(scope="module")
def scene(pt):
    """The groove at 24 x 20 with the rectangle mask and the edit inside it (`path_mapedit_fp64.edit_scene`), and its tracer."""
    s = pm.edit_scene(pt)
    s["tracer"] = pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], s["H"], s["W"], FOV)
    s["maps"] = (s["a"], s["r"], s["m"], s["env"])
    return s


def _diff(s, spp, max_depth, seed, edited=None, mask="scene", **kw):
    delta, base, rewalked = s["tracer"].render_edit_diff(*s["maps"], s["edited"] if edited is None else edited,
                                                         s["mask"] if isinstance(mask, str) else mask, spp=spp, max_depth=max_depth, seed=seed, **kw)
    assert delta.shape == (s["H"], s["W"], 3) and base.shape == delta.shape and rewalked.shape == (s["H"], s["W"]) and rewalked.dtype == torch.int32
    return delta.cpu().numpy(), base.cpu().numpy(), rewalked.cpu().numpy()


def _parity_case(s, oracle64, max_depth, seed, normal=False):
    """delta against L_e - L_f and base against L_f, the error of the worst channel relative to max(|L_e|, |L_f|, mean |L_e|): at least
    0.98 of the pixels within 1e-3 (the project's 0.99 per walk, and there are two walks).  The reference's own bracket first."""
    ref = pm.reference(oracle64, s, max_depth, seed, normal=normal)
    outside = ref["differ"] & ~s["mask"]
    name = f"{'normal map, ' if normal else ''}max_depth {max_depth} seed {seed}"
    _report(f"{name}: fp64 touched share; differing share; differing outside the mask",
            f"{ref['touched'].mean():.4f}; {ref['differ'].mean():.4f}; {outside.mean():.4f}")
    assert 0.05 <= ref["differ"].mean() <= 0.3
    if max_depth >= 4:
        assert outside.mean() >= 0.03
    assert not (ref["differ"] & ~ref["touched"]).any()
    delta, base, rewalked = _diff(s, 1, max_depth, seed, **({"normal": s["nrm"]} if normal else {}))
    assert np.isfinite(delta).all() and np.isfinite(base).all()
    for what, got, want in (("delta", delta, ref["delta"]), ("base", base, ref["fitted"])):
        frac, err = pd.share_within(got.astype(np.float64), want, ref["scale"], 1e-3)
        _report(f"{name}: {what} against the two fp64 walks, share of pixels within 1e-3",
                f"{frac:.4f} ({int((err > 1e-3).sum())} pixels beyond, max err {err.max():.3e})")
        assert frac >= 0.98, (what, max_depth, seed, frac, np.argwhere(err > 1e-3)[:10])
    return ref, delta, base, rewalked


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_depth", [2, 4, 16])
def test_both_walks_match_fp64(pt, scene, oracle64, max_depth):
    for seed in (0, 1, 2):
        _parity_case(scene, oracle64, max_depth, seed)


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_depth, seed", [(16, 0), (2, 1)])
def test_exact_zeros_and_the_touch_rule(pt, scene, oracle64, max_depth, seed):
    """spp 1: (i) a pixel that was not walked twice has all-zero bits in delta; (ii) a pixel whose fp64 walks differ was walked twice,
    except at most 0.01 of the pixels; (iii) a pixel walked twice lies in fp64's touched set, except at most 0.01 of the pixels.  Both
    caps are the project's 0.99 per-walk parity share; in fp64 the first set is empty and the second included, so the reference
    alone meets them."""
    s = scene
    ref = pm.reference(oracle64, s, max_depth, seed)
    assert not (ref["differ"] & ~ref["touched"]).any()
    delta, base, rewalked = _diff(s, 1, max_depth, seed)
    assert set(np.unique(rewalked)) <= {0, 1}
    assert not delta.view(np.uint32)[rewalked == 0].any()                                                   # (i)
    missed = ref["differ"] & (rewalked == 0)
    beyond = (rewalked >= 1) & ~ref["touched"]
    _report(f"max_depth {max_depth} seed {seed}: pixels walked twice; fp64 touched; differing and not walked twice (bound 0.01); walked twice "
            f"outside fp64's touched set (bound 0.01)", f"{int((rewalked >= 1).sum())}; {int(ref['touched'].sum())}; {missed.mean():.4f}; {beyond.mean():.4f}")
    assert missed.mean() <= 0.01                                                                            # (ii)
    assert beyond.mean() <= 0.01                                                                            # (iii)
    assert (rewalked >= 1).any()


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_same_walk_twice_differs_in_nothing(pt, scene):
    """Mask all ones and the fitted arrays as the edit: every sample whose camera ray reads a texel is walked twice, on the same values,
    and a state of trip 0 that leaked into trip 1 would show in delta.  "Reads a texel": the camera ray's fp64 hit lies at least 1e-4
    (barycentric) inside its triangle for all three samples, which holds for most pixels."""
    s = scene
    spp = 3
    ones = np.ones((s["H"], s["W"]), bool)
    delta, base, rewalked = _diff(s, spp, 16, 5, edited=(s["a"], s["r"], s["m"]), mask=ones)
    assert not delta.view(np.uint32).any()
    brute = pf.TorchBrute(s["V"][s["T"]])
    sure = np.ones(s["H"] * s["W"], bool)
    for k in range(spp):
        t, _, margin = brute.hits(*pd.camera_rays(s["H"], s["W"], 5, k))
        sure &= np.isfinite(t) & (margin > 1e-4)
    sure = sure.reshape(s["H"], s["W"])
    _report("the same walk twice, spp 3: pixels every camera ray of which surely reads a texel; pixels walked twice three times",
            f"{int(sure.sum())}; {int((rewalked == spp).sum())} of {sure.size}")
    assert sure.mean() > 0.8 and (rewalked[sure] == spp).all() and rewalked.max() == spp
    plain = s["tracer"].render(*s["maps"], spp=spp, max_depth=16, seed=5)
    assert tl.parity(base.astype(np.float64), plain.cpu().numpy().astype(np.float64))[0] == 1.0


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_nothing_edited(pt, scene):
    s = scene
    dev = s["tracer"].device
    rays, once = torch.zeros(s["H"], s["W"], dtype=torch.int32, device=dev), torch.zeros(s["H"], s["W"], dtype=torch.int32, device=dev)
    delta, base, rewalked = _diff(s, 4, 4, 2, mask=np.zeros((s["H"], s["W"]), bool), rays=rays)
    assert not rewalked.any() and not delta.view(np.uint32).any()
    plain = s["tracer"].render(*s["maps"], spp=4, max_depth=4, seed=2, rays=once)
    frac, err = tl.parity(base.astype(np.float64), plain.cpu().numpy().astype(np.float64))
    same = np.array_equal(base.view(np.uint32), _bits(plain))
    _report("nothing edited, spp 4: base against render(fitted), largest error; the same bits", f"{err.max():.3e}; {same}")
    assert frac == 1.0
    agree = float((rays == once).float().mean())
    _report("nothing edited, spp 4: share of pixels whose rays equal render's", f"{agree:.4f}")
    assert agree >= 0.99


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_everything_edited(pt, scene):
    s = scene
    ones = np.ones((s["H"], s["W"]), bool)
    edited = pm.edit_inside(s["a"], s["r"], s["m"], ones)
    delta, base, rewalked = _diff(s, 4, 4, 3, edited=edited, mask=ones)
    Le = s["tracer"].render(*edited, s["env"], spp=4, max_depth=4, seed=3).cpu().numpy().astype(np.float64)
    Lf = s["tracer"].render(*s["maps"], spp=4, max_depth=4, seed=3).cpu().numpy().astype(np.float64)
    for what, got, want in (("base + delta against render(edited)", base.astype(np.float64) + delta, Le), ("base against render(fitted)", base, Lf)):
        frac, err = tl.parity(np.asarray(got, np.float64), want)
        _report(f"everything edited, spp 4: {what}, largest error", f"{err.max():.3e}")
        assert frac == 1.0, what
    assert (rewalked == 4).mean() > 0.8 and tl.parity(Le, Lf)[0] < 0.5    # and the edit is one


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normal", [False, True])
def test_launch_splits_give_the_same_bits(pt, scene, normal):
    s = scene
    kw = {"normal": s["nrm"]} if normal else {}
    whole = s["tracer"].render_edit_diff(*s["maps"], s["edited"], s["mask"], spp=5, max_depth=16, seed=7, spp_per_launch=8, **kw)
    assert bool((whole[2] > 0).any()) and bool(whole[0].any())
    for split in (1, 2):
        part = s["tracer"].render_edit_diff(*s["maps"], s["edited"], s["mask"], spp=5, max_depth=16, seed=7, spp_per_launch=split, **kw)
        for k, (x, y) in enumerate(zip(whole, part)):
            assert np.array_equal(_bits(x), _bits(y)), (split, k)
    # the derived mask is the rectangle: the same bits again
    derived = s["tracer"].render_edit_diff(*s["maps"], s["edited"], spp=5, max_depth=16, seed=7, **kw)
    for k, (x, y) in enumerate(zip(whole, derived)):
        assert np.array_equal(_bits(x), _bits(y)), k


def test_the_raw_call(pt, scene):
    """`PathTracer.render_edit_diff` is the raw call; `rewalked` is nullable and added to; the outputs start from whatever they held."""
    s = scene
    tracer, dev = s["tracer"], s["tracer"].device
    whole = tracer.render_edit_diff(*s["maps"], s["edited"], s["mask"], spp=5, max_depth=16, seed=7, spp_per_launch=2)
    keep = tracer._inputs(*s["maps"], None)
    ed = [torch.as_tensor(x).to(dev).contiguous() for x in s["edited"]]
    mk = torch.as_tensor(s["mask"]).to(dev, torch.uint8)
    delta, base = torch.full((s["H"], s["W"], 3), 7.0, device=dev), torch.full((s["H"], s["W"], 3), -7.0, device=dev)
    rewalked = torch.zeros(s["H"], s["W"], dtype=torch.int32, device=dev)
    args = (*tracer._frame(*keep, 5, 16, 7, 2), None, torch.cuda.current_stream().cuda_stream, *(x.data_ptr() for x in ed), mk.data_ptr(), None)
    fn = pt.symbol("matpbr_path_render_edit_diff")
    assert fn(*args, delta.data_ptr(), base.data_ptr(), rewalked.data_ptr()) == 0
    for k, (x, y) in enumerate(zip(whole, (delta, base, rewalked))):
        assert np.array_equal(_bits(x), _bits(y)), k
    assert fn(*args, delta.data_ptr(), base.data_ptr(), None) == 0                        # nullable
    assert fn(*args, delta.data_ptr(), base.data_ptr(), rewalked.data_ptr()) == 0         # added to
    assert np.array_equal(rewalked.cpu().numpy(), 2 * whole[2].cpu().numpy()) and np.array_equal(_bits(delta), _bits(whole[0]))
    for k in (0, 1):
        ptrs = [delta.data_ptr(), base.data_ptr()]
        ptrs[k] = None
        assert fn(*args, *ptrs, None) == -1, k
    objects = pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], s["H"], s["W"], FOV, objects=[pd.cube_object(pd.HIDDEN_CUBE)])
    with pytest.raises(ValueError, match="objects"):
        objects.render_edit_diff(*s["maps"], s["edited"], spp=1)


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_shading_normals(pt, scene, oracle64):
    s = scene
    for seed in (0, 1):
        ref, delta, base, rewalked = _parity_case(s, oracle64, 4, seed, normal=True)
    flat = _diff(s, 1, 4, 1)
    assert tl.parity(flat[1].astype(np.float64), base.astype(np.float64))[0] < 0.5            # the map reaches the kernel
    assert not np.array_equal(flat[0], delta)


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_photograph_survives(pt, scene):
    s = scene
    delta, base, rewalked = s["tracer"].render_edit_diff(*s["maps"], s["edited"], s["mask"], spp=4, max_depth=4, seed=6)
    keep = (rewalked == 0).cpu().numpy()
    assert 0.3 < keep.mean() < 0.9
    photo = np.random.default_rng(3).gamma(2.0, 0.5, (s["H"], s["W"], 3)).astype(np.float32)
    zero3, zero1 = torch.zeros_like(delta), torch.zeros(s["H"], s["W"], device=delta.device)
    d, b = delta.cpu().numpy(), base.cpu().numpy()
    for what, got, host in (("additive", pt.composite(zero3, delta, zero1, photo), pt.composite_host(zero3.cpu().numpy(), d, zero1.cpu().numpy(), photo)),
                            ("ratio", pt.composite_ratio(zero3, delta, base, zero1, photo),
                             pt.composite_ratio_host(zero3.cpu().numpy(), d, b, zero1.cpu().numpy(), photo))):
        assert np.array_equal(_bits(got)[keep], photo.view(np.uint32)[keep]), what
        assert np.array_equal(_bits(got), host.view(np.uint32)), what
        assert (_bits(got)[~keep] != photo.view(np.uint32)[~keep]).any(), what
    assert np.array_equal(_bits(pt.composite_edit(delta, photo)), _bits(pt.composite(zero3, delta, zero1, photo)))
    assert np.array_equal(_bits(pt.composite_edit(delta, photo, base)), _bits(pt.composite_ratio(zero3, delta, base, zero1, photo)))
    assert np.array_equal(pt.composite_edit_host(d, photo, b).view(np.uint32), _bits(pt.composite_edit(delta, photo, base)))


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_the_ratio_transfer_helps_where_the_fit_is_off(pt, scene):
    """spp 16, max_depth 4, seed 0.  The true maps T are the groove's; the "fit" F is T with the albedo halved; the edit multiplies the
    albedo by 0.5 inside the mask.  Photograph = render(T), target = render(T edited).  Over the masked pixels the ratio composite of
    render_edit_diff(F, F edited) is at least four times closer to the target than the additive one.  The fp64 restatement of this
    case gives 6.56e-3 against 1.05e-1 (0.063), and 1.86e-1 for the photograph left as it is."""
    s = scene
    tracer, mask = s["tracer"], s["mask"]
    kw = dict(spp=16, max_depth=4, seed=0)
    half = np.float32(0.5)

    def darker(a):
        out = a.copy()
        out[mask] *= half
        return out

    T, F = s["a"], s["a"] * half
    photo = tracer.render(T, s["r"], s["m"], s["env"], **kw)
    target = tracer.render(darker(T), s["r"], s["m"], s["env"], **kw).cpu().numpy().astype(np.float64)
    delta, base, rewalked = tracer.render_edit_diff(F, s["r"], s["m"], s["env"], (darker(F), s["r"], s["m"]), **kw)
    assert (rewalked.cpu().numpy()[mask] > 0).mean() > 0.9                  # the derived mask is the rectangle
    mae = lambda img: float(np.abs(img.cpu().numpy().astype(np.float64) - target)[mask].mean())
    additive, ratio, nothing = mae(pt.composite_edit(delta, photo)), mae(pt.composite_edit(delta, photo, base)), mae(photo)
    _report("fitted albedo 0.5 x true, albedo edit x 0.5, spp 16: mean |additive - target|; mean |ratio - target|; their quotient; the photograph "
            "left as it is", f"{additive:.3e}; {ratio:.3e}; {ratio / additive:.3f}; {nothing:.3e}")
    assert ratio <= 0.25 * additive


# ---- 10 --------------------------------------------------------------------------------------------------------------------------------
def test_render_final_cli_edit_composite(pt, tmp_path):
    """`render_final.py --mode real --integrator path --edit_roughness 0.2 --edit_composite --spp 4` on a synthetic output at 32 x 32 with a
    gt_image.exr written here: the .exr has the photograph's bits wherever an in-process `render_edit_diff` of the same arguments walked
    no sample twice, and differs from it inside the mask; `--edit_transfer ratio` runs and writes another picture."""
    from materialist_amd import relight
    from materialist_amd.imageio_exr import read_exr, write_exr
    from materialist_amd.pipeline import load_image

    tmp = str(tmp_path)
    scene_dir, mask = tl.synthetic_output(tmp, edit=True)
    photo = np.random.default_rng(4).gamma(2.0, 0.3, (32, 32, 3)).astype(np.float32)
    write_exr(os.path.join(scene_dir, "gt_image.exr"), photo)
    cmd = [sys.executable, os.path.join(ROOT, "render_final.py"), "--save_name", "case", "--input_path", tmp, "--save_path", tmp, "--mode", "real",
           "--integrator", "path", "--edit_roughness", "0.2", "--edit_composite", "--spp", "4"]
    exr, png = (os.path.join(tmp, "case", "mi_ec_case_envmap__r_0.2" + ext) for ext in (".exr", ".png"))

    def run(extra=()):
        res = subprocess.run(cmd + list(extra), capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout + res.stderr
        assert os.path.exists(png) and not os.path.exists(os.path.join(tmp, "case", "mi_case_envmap__r_0.2.exr"))
        return np.ascontiguousarray(read_exr(exr)[..., :3], dtype=np.float32)

    img = run()
    mat = relight.load_estimated_brdf(os.path.join(scene_dir, "best_results"), "cuda")
    fitted = tuple(mat[k].clone() for k in ("albedo", "roughness", "metallic"))
    relight.apply_edit(mat, {"albedo": None, "roughness": 0.2, "metallic": None})
    tracer = relight._path_tracer(scene_dir, "case", mat, "cuda")
    delta, base, rewalked = tracer.render_edit_diff(*fitted, load_image(os.path.join(scene_dir, "best_results", "envmap.hdr")),
                                                    (mat["albedo"], mat["roughness"], mat["metallic"]), spp=4, max_depth=4, seed=0)
    keep = (rewalked == 0).cpu().numpy()
    assert 0.2 < keep.mean() < 0.9 and np.isfinite(img).all() and (img >= 0).all()
    assert np.array_equal(img.view(np.uint32)[keep], photo.view(np.uint32)[keep])
    assert (img != photo).any(-1)[mask].mean() > 0.9
    assert np.array_equal(img.view(np.uint32), _bits(pt.composite_edit(delta, photo)))
    ratio = run(["--edit_transfer", "ratio"])
    assert np.array_equal(ratio.view(np.uint32)[keep], photo.view(np.uint32)[keep])
    assert (ratio != img).any() and np.isfinite(ratio).all()
