"""Vertex-coloured inserted objects on the GPU (libmatpbr_path.so's `matpbr_path_render_objects_colors`, DESIGN.md section 1.4,
"Vertex-coloured inserted objects"): every path of a table with a coloured smooth diffuse sphere and a coloured flat PBR cube against
the fp64 restatement, the closed form of tests/test_path_color_host.py in expectation on the device, bits (launch splits, a table
without colours, uniform colours against the uncoloured table), the colour guide against its CPU twin, the refusals through
`PathTracer`, and `render_final.py --mode oi --oi_scene` with a coloured PLY."""
import json
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

import path_color_fp64 as pc  # noqa: E402
import path_fp64 as pf  # noqa: E402
import path_light_fp64 as pl  # noqa: E402
import path_objects_fp64 as pob  # noqa: E402
import path_oi_fp64 as po  # noqa: E402
import path_oi_pbr_fp64 as pp  # noqa: E402
import path_rough_fp64 as pr  # noqa: E402
import path_testlib as tl  # noqa: E402
from path_testlib import bits as _bits, parity as _parity, raw_args as _raw_args  # noqa: E402
from test_path_color_host import SEEDS, _write_ply, furnace_expected  # noqa: E402

pytestmark = pytest.mark.gpu

FOV = pf.FOV


@pytest.fixture(scope="module")
def pt():
    return tl.load(gpu=True)


_report = tl.reporter("path color", "test_gpu_path_colors")


@pytest.fixture(scope="module")
def scene(pt):
    """The groove at 24 x 20 (a partial tile) with `path_color_fp64.table_scene` in front of it."""
    s = tl.groove_with_objects(pt, pc.table_scene(), pob.merged)
    st = s["tracer"].stats
    assert st["n_objects"] == 4 and st["n_colored_objects"] == 2 and st["n_pbr_objects"] == 1 and st["n_smooth_objects"] == 2
    assert s["tracer"].obj_col is not None and not s["tracer"].rough and s["tracer"].lights is None
    return s


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_on", [True, False])
def test_every_path_matches_the_fp64_restatement(pt, scene, oracle64, env_on):
    """At least 0.99 of the pixels within 1e-3 at spp 1 (`path_testlib.parity`; on the CPU the restatement over the library's fp32
    traversal and over the fp64 brute force disagrees in no pixel of these renders, test_path_color_host.py): max_depth 2, 6, 16 x
    seeds 0-2, with the envmap on and zero (zero: the table holds no light, so both renders must be exactly black)."""
    s = scene
    H, W = s["H"], s["W"]
    env = s["env"] if env_on else np.zeros_like(s["env"])
    tab = pt.env_tables(env)
    for max_depth in (2, 6, 16):
        for seed in (0, 1, 2):
            got = s["tracer"].render(s["a"], s["r"], s["m"], env, spp=1, max_depth=max_depth, seed=seed).cpu().numpy().astype(np.float64)
            assert np.isfinite(got).all()
            ref, rec = pob.replay_objects(oracle64, s["V"], s["T"], s["a"], s["r"], s["m"], env, tab, H, W, max_depth, seed, s["table"])
            assert rec["colored_camera"][:, 0].any() and rec["colored_camera"][:, 1].any() and rec["colored_indirect"].any()
            if not env_on:                                          # this table holds no light: without the envmap there is no emitter and
                assert not ref.any() and not got.any()              # parity's denominator is 0; the render is black, exactly
                continue
            frac, err = _parity(got, ref)
            _report(f"per-path parity with coloured objects, envmap {'on' if env_on else 'zero'}, max_depth {max_depth} seed {seed}: share of pixels within 1e-3",
                    f"{frac:.4f} ({int((err > 1e-3).sum())} flipped paths, max err {err.max():.3e})")
            assert frac >= 0.99, (max_depth, seed, frac, np.argwhere(err > 1e-3)[:10])


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_affine_colours_in_a_furnace(pt):
    """Host test 3 on the device: the same 64 seeds x spp 16 at 12 x 10, max_depth 2, and the same bound, 5 standard errors + 1e-3."""
    H, W = 10, 12
    objects = pc.furnace_scene()
    expected, covered = furnace_expected(objects, H, W)
    assert covered.sum() >= 12
    Vs, Ts = pp.FAR_TRIANGLE
    tracer = pt.PathTracer(Vs, Ts, H, W, FOV, objects=objects)
    assert tracer.stats["n_colored_objects"] == 1 and tracer.stats["n_lights"] == 1
    maps = (np.zeros((H, W, 3), np.float32), np.ones((H, W, 1), np.float32), np.zeros((H, W, 1), np.float32))
    env = np.zeros((4, 8, 3), np.float32)
    tabs = tracer.tables(env)
    vals = np.stack([tracer.render(*maps, env, spp=16, max_depth=2, seed=sd, spp_per_launch=16, tables=tabs).cpu().numpy() for sd in SEEDS])
    assert np.isfinite(vals).all()
    ok, excess = pl.within_five_sigma(vals.astype(np.float64), expected, covered)
    _report(f"affine colours in a furnace, on the device: worst |mean - L p rho| / (5 se + 1e-3) over {int(covered.sum())} pixels", f"{excess:.3f}")
    assert ok


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_bits(pt, scene):
    s = scene
    maps = (s["a"], s["r"], s["m"], s["env"])
    H, W, rm = s["H"], s["W"], s["rm"]
    colors, rough = pt.symbol("matpbr_path_render_objects_colors"), pt.symbol("matpbr_path_render_objects_rough")
    # every split of a frame into launches gives the same bits
    whole = s["tracer"].render(*maps, spp=6, max_depth=16, seed=7, spp_per_launch=6)
    for split in (1, 3, 4):
        assert np.array_equal(_bits(whole), _bits(s["tracer"].render(*maps, spp=6, max_depth=16, seed=7, spp_per_launch=split))), split
    # PathTracer.render with coloured objects is the raw call
    out = torch.empty(H, W, 3, device=s["tracer"].device)
    keep, args = _raw_args(s["tracer"], maps, 6, 16, 5, 4, out)
    assert colors(*args, *tl.object_tail(s["tracer"], "matpbr_path_render_objects_colors")) == 0
    assert np.array_equal(_bits(s["tracer"].render(*maps, spp=6, max_depth=16, seed=5, spp_per_launch=4)), _bits(out))
    # a table without colours renders through the new entry to the bits of matpbr_path_render_objects_rough (obj_col NULL)
    refs = {}
    for name, objects in (("rough", pr.table_scene()), ("pbr", pp.table_scene()), ("unflagged", pc.table_scene(flagged=False))):
        tracer = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV, objects=objects)
        assert tracer.obj_col is None and tracer.stats["n_colored_objects"] == 0
        ref, got = torch.empty(H, W, 3, device=tracer.device), torch.empty(H, W, 3, device=tracer.device)
        keep1, a1 = _raw_args(tracer, maps, 6, 16, 5, 4, ref)
        assert rough(*a1, *tl.object_tail(tracer)) == 0
        keep2, a2 = _raw_args(tracer, maps, 6, 16, 5, 4, got)
        tail = tl.object_tail(tracer, "matpbr_path_render_objects_colors")
        assert len(tail) == 9 and tail[8] is None and colors(*a2, *tail) == 0
        assert np.array_equal(_bits(got), _bits(ref)), name
        assert np.array_equal(_bits(tracer.render(*maps, spp=6, max_depth=16, seed=5, spp_per_launch=4)), _bits(ref)), name
        refs[name] = ref
    # all corner colours (1, 1, 1): the paths of the unflagged table through the parent's kernel; at most 16 vertices contribute, each
    # a few ulp apart between two instantiations of the kernel: 1e-5 relative
    uniform = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV, objects=pc.table_scene(uniform=True))
    assert uniform.stats["n_colored_objects"] == 2
    got = uniform.render(*maps, spp=6, max_depth=16, seed=5, spp_per_launch=4).cpu().numpy().astype(np.float64)
    ref = refs["unflagged"].cpu().numpy().astype(np.float64)
    rel = np.abs(got - ref) / np.maximum(np.abs(ref), np.abs(ref).mean())
    equal = bool(np.array_equal(got, ref))
    _report("uniform colours against the unflagged table through the parent's kernel: worst relative difference (bound 1e-5); bit-equal", f"{rel.max():.3e}; {equal}")
    assert rel.max() <= 1e-5
    # and the coloured table differs from it
    assert np.abs(s["tracer"].render(*maps, spp=6, max_depth=16, seed=5, spp_per_launch=4).cpu().numpy() - ref).max() > 1e-2


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_feature_colors_and_the_guide(pt, scene):
    """`feature_colors` on the device equals its CPU twin bit for bit (the barycentrics are formed without contraction on both); the
    albedo guide multiplies a coloured object's constant by it."""
    from materialist_amd import relight

    s = scene
    H, W = s["H"], s["W"]
    got = s["tracer"].feature_colors()
    Vm, Tm, tb, tint = pt.merge_objects(s["rm"]["vertices"], s["rm"]["triangles"], s["objects"], colors=True)
    n_scene = s["rm"]["triangles"].shape[0]
    host = pt.feature_colors_host(pt.build_bvh(Vm, Tm, n_scene), H, W, FOV, tb, tint, n_scene)
    assert np.array_equal(_bits(got), host.view(np.uint32))
    geom = s["tracer"].features()
    ids = geom[..., 7].cpu().numpy()
    assert set(np.unique(ids)) >= {0.0, 1.0, 2.0, 3.0}
    assert np.all(host[(ids != 1) & (ids != 2)] == 1.0) and host[ids == 1].std() > 0.05 and host[ids == 2].std() > 0.05
    bsdfs = [ob["bsdf"] for ob in s["objects"]]
    alb = torch.as_tensor(s["a"])
    plain = relight.albedo_guide(geom, alb, bsdfs).cpu().numpy()
    guide = relight.albedo_guide(geom, alb, bsdfs, got).cpu().numpy()
    assert np.array_equal(guide[(ids != 1) & (ids != 2)], plain[(ids != 1) & (ids != 2)])
    assert np.allclose(guide[ids == 1], np.float32(pc.DIFFUSE_BASE["reflectance"]) * host[ids == 1], rtol=1e-6, atol=0)
    assert np.allclose(guide[ids == 2], np.float32(pc.PBR_BASE["albedo"]) * host[ids == 2], rtol=1e-6, atol=0)
    # a tracer without a coloured object: (1, 1, 1) everywhere
    plain_tracer = pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], H, W, FOV, objects=pc.table_scene(flagged=False))
    assert bool((plain_tracer.feature_colors() == 1.0).all())


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_through_pathtracer(pt, scene):
    s = scene
    maps = (s["a"], s["r"], s["m"], s["env"])
    H, W, rm = s["H"], s["W"], s["rm"]
    Vc, Tc = po.cube((0.0, 0.0, -1.2), 0.1, (0.0, 0.0, 0.0))
    good = np.full((8, 3), 0.5)
    for bsdf in (po.GLASS, pl.QUAD_LIGHT, pr.FROSTED_02):
        with pytest.raises(ValueError, match="diffuse"):
            pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV, objects=[{"vertices": Vc, "triangles": Tc, "bsdf": bsdf, "colors": good}])
    with pytest.raises(ValueError, match="vertex 2"):
        pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV,
                      objects=[{"vertices": Vc, "triangles": Tc, "bsdf": po.DIFFUSE_08, "colors": np.where(np.arange(8)[:, None] == 2, 1.5, good)}])
    with pytest.raises(ValueError, match="objects"):
        s["tracer"].render(*maps, spp=1, normal=np.zeros((H, W, 3), np.float32))
    with pytest.raises(ValueError, match="objects"):
        s["tracer"].render_bwd(*maps, torch.zeros(H, W, 3))
    # every entry from before the flag refuses the coloured table; the new one refuses it without its colours
    out = torch.empty(H, W, 3, device=s["tracer"].device)
    keep, args = _raw_args(s["tracer"], maps, 1, 2, 0, 1, out)
    for entry in ("matpbr_path_render_objects", "matpbr_path_render_objects_normals", "matpbr_path_render_objects_pbr",
                  "matpbr_path_render_objects_lights", "matpbr_path_render_objects_rough"):
        assert pt.symbol(entry)(*args, *tl.object_tail(s["tracer"], entry)) == -1, entry
    tail = tl.object_tail(s["tracer"], "matpbr_path_render_objects_colors")
    assert pt.symbol("matpbr_path_render_objects_colors")(*args, *tail[:8], None) == -1
    # a library from before the feature: PathError at construction, naming the entry
    real = pt.symbol

    class Old:
        pass

    try:
        pt.symbol = lambda name, lib=None: real(name, Old() if name in pt.COLOR_SYMBOLS else lib)
        with pytest.raises(pt.PathError, match="matpbr_path_render_objects_colors"):
            pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV, objects=pc.table_scene())
        pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV, objects=pc.table_scene(flagged=False))
    finally:
        pt.symbol = real


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_render_final_cli_coloured_ply(pt, tmp_path):
    """`render_final.py --mode oi --oi_scene` with a coloured PLY written here: the bits of the direct PathTracer calls; "vertex" and
    "vertex_linear" give different images; `--denoise atrous` gives a finite image."""
    from materialist_amd import mesh, relight
    from materialist_amd.imageio_exr import read_exr

    tmp = str(tmp_path)
    scene_dir = tl.synthetic_output(tmp)
    Vb, Tb = po.cube((0.02, 0.0, -0.9), 0.12, (0.4, 0.5, 0.3))
    Vb = Vb.astype(np.float32)
    C8 = np.random.default_rng(7).integers(0, 256, (8, 3))
    os.makedirs(os.path.join(tmp, "lists"))
    _write_ply(os.path.join(tmp, "lists", "bowl.ply"), Vb, Tb, C8, "binary_little_endian")
    listing = os.path.join(tmp, "lists", "bowl.json")
    cli = [sys.executable, os.path.join(ROOT, "render_final.py"), "--save_name", "case", "--input_path", tmp, "--save_path", tmp,
           "--mode", "oi", "--spp", "4", "--oi_iters", "2", "--oi_max_depth", "8", "--oi_scene", listing]
    mat = relight.load_estimated_brdf(os.path.join(scene_dir, "best_results"))
    env = relight.load_image(os.path.join(scene_dir, "best_results", "envmap.hdr"))
    maps = (mat["albedo"], mat["roughness"], mat["metallic"])
    exr, png = (os.path.join(tmp, "case", "mi_oi_case_envmap" + ext) for ext in (".exr", ".png"))

    def run(colors, extra=()):
        with open(listing, "w") as f:
            json.dump({"objects": [{"ply": "bowl.ply", "bsdf": po.DIFFUSE_08, "colors": colors}]}, f)
        for path in (exr, png):
            if os.path.exists(path):
                os.remove(path)
        res = subprocess.run(cli + list(extra), capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout + res.stderr
        assert os.path.exists(png)
        img = np.ascontiguousarray(read_exr(exr)[..., :3], dtype=np.float32)
        assert np.isfinite(img).all() and (img >= 0).all() and float(img.std()) > 0
        return img

    def direct(colors):
        V, T, C = mesh.read_ply_any(os.path.join(tmp, "lists", "bowl.ply"), colors=True)
        ob = {"vertices": V, "triangles": T, "bsdf": po.DIFFUSE_08}
        if colors != "none":
            ob["colors"] = C ** 2.2 if colors == "vertex" else C
        tracer = relight._path_tracer(scene_dir, "case", mat, "cuda", [ob])
        assert tracer.stats["n_colored_objects"] == (colors != "none")
        acc = torch.zeros_like(mat["albedo"])
        for seed in (0, 1):
            acc += tracer.render(*maps, env, spp=4, max_depth=8, seed=seed)
        return (acc / 2).cpu().numpy()

    images = {}
    for colors in ("vertex", "vertex_linear"):
        images[colors] = run(colors)
        assert np.array_equal(images[colors].view(np.uint32), direct(colors).view(np.uint32)), colors
    assert np.abs(images["vertex"] - images["vertex_linear"]).max() > 1e-3
    run("vertex", ["--denoise", "atrous"])
