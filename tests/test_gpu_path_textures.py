"""UV-textured inserted objects on the GPU (libmatpbr_path.so's `matpbr_path_render_objects_textures`, DESIGN.md section 1.4, "Textured
inserted objects"): every path of a table with a textured smooth diffuse sphere, a PBR cube with a base and an orm image and a
vertex-coloured and textured cube against the fp64 restatement, the closed form of tests/test_path_texture_host.py in expectation on
the device, bits (launch splits, a table without textures, uniform images against the unflagged table), the tint guide against its CPU
twin, the refusals through `PathTracer`, and `render_final.py --mode oi` with a textured PLY and PNGs."""
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
import path_texture_fp64 as px  # noqa: E402
from path_testlib import bits as _bits, parity as _parity, raw_args as _raw_args  # noqa: E402
from test_path_texture_host import EVENTS, SEEDS, _write_ply, furnace_expected  # noqa: E402

pytestmark = pytest.mark.gpu

FOV = pf.FOV


@pytest.fixture(scope="module")
def pt():
    return tl.load(gpu=True)


_report = tl.reporter("path texture", "test_gpu_path_textures")


@pytest.fixture(scope="module")
def scene(pt):
    """The groove at 24 x 20 (a partial tile) with `path_texture_fp64.table_scene` in front of it."""
    s = tl.groove_with_objects(pt, px.table_scene(), pob.merged)
    st = s["tracer"].stats
    assert st["n_objects"] == 5 and st["n_textured_objects"] == 3 and st["n_colored_objects"] == 1 and st["n_pbr_objects"] == 1 and st["n_smooth_objects"] == 2
    assert s["tracer"].textures is not None and s["tracer"].obj_col is not None and not s["tracer"].rough and s["tracer"].lights is None
    return s


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_on", [True, False])
def test_every_path_matches_the_fp64_restatement(pt, scene, oracle64, env_on):
    """At least 0.99 of the pixels within 1e-3 at spp 1 (`path_testlib.parity`; on the CPU the restatement over the library's fp32
    traversal and over the fp64 brute force disagrees in no pixel of these renders, test_path_texture_host.py): max_depth 2, 6, 16 x
    seeds 0-2, with the envmap on and zero (zero: the table holds no light, so both renders must be exactly black).  Every recorded
    event occurs in each render."""
    s = scene
    H, W = s["H"], s["W"]
    env = s["env"] if env_on else np.zeros_like(s["env"])
    tab = pt.env_tables(env)
    for max_depth in (2, 6, 16):
        for seed in (0, 1, 2):
            got = s["tracer"].render(s["a"], s["r"], s["m"], env, spp=1, max_depth=max_depth, seed=seed).cpu().numpy().astype(np.float64)
            assert np.isfinite(got).all()
            ref, rec = pob.replay_objects(oracle64, s["V"], s["T"], s["a"], s["r"], s["m"], env, tab, H, W, max_depth, seed, s["table"])
            assert rec["textured_camera"][:, :3].any(0).all() and all(rec[e].any() for e in EVENTS), (max_depth, seed)
            if not env_on:                                          # this table holds no light: without the envmap there is no emitter and
                assert not ref.any() and not got.any()              # parity's denominator is 0; the render is black, exactly
                continue
            frac, err = _parity(got, ref)
            _report(f"per-path parity with textured objects, envmap on, max_depth {max_depth} seed {seed}: share of pixels within 1e-3",
                    f"{frac:.4f} ({int((err > 1e-3).sum())} flipped paths, max err {err.max():.3e})")
            assert frac >= 0.99, (max_depth, seed, frac, np.argwhere(err > 1e-3)[:10])


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_affine_texels_in_a_furnace(pt):
    """Host test (c) on the device: the same 64 seeds x spp 16 at 12 x 10, max_depth 2, and the same bound, 5 standard errors + 1e-3."""
    H, W = 10, 12
    objects = px.furnace_scene()
    expected, covered = furnace_expected(objects, H, W)
    assert covered.sum() >= 12
    Vs, Ts = pp.FAR_TRIANGLE
    tracer = pt.PathTracer(Vs, Ts, H, W, FOV, objects=objects)
    assert tracer.stats["n_textured_objects"] == 1 and tracer.stats["n_lights"] == 1
    maps = (np.zeros((H, W, 3), np.float32), np.ones((H, W, 1), np.float32), np.zeros((H, W, 1), np.float32))
    env = np.zeros((4, 8, 3), np.float32)
    tabs = tracer.tables(env)
    vals = np.stack([tracer.render(*maps, env, spp=16, max_depth=2, seed=sd, spp_per_launch=16, tables=tabs).cpu().numpy() for sd in SEEDS])
    assert np.isfinite(vals).all()
    ok, excess = pl.within_five_sigma(vals.astype(np.float64), expected, covered)
    _report(f"affine texels in a furnace, on the device: worst |mean - L p T| / (5 se + 1e-3) over {int(covered.sum())} pixels", f"{excess:.3f}")
    assert ok


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_bits(pt, scene):
    s = scene
    maps = (s["a"], s["r"], s["m"], s["env"])
    H, W, rm = s["H"], s["W"], s["rm"]
    textures, colors = pt.symbol("matpbr_path_render_objects_textures"), pt.symbol("matpbr_path_render_objects_colors")
    # every split of a frame into launches gives the same bits
    whole = s["tracer"].render(*maps, spp=6, max_depth=16, seed=7, spp_per_launch=6)
    for split in (1, 3, 4):
        assert np.array_equal(_bits(whole), _bits(s["tracer"].render(*maps, spp=6, max_depth=16, seed=7, spp_per_launch=split))), split
    # PathTracer.render with textured objects is the raw call
    out = torch.empty(H, W, 3, device=s["tracer"].device)
    keep, args = _raw_args(s["tracer"], maps, 6, 16, 5, 4, out)
    tail = tl.object_tail(s["tracer"], "matpbr_path_render_objects_textures")
    assert len(tail) == 13 and textures(*args, *tail) == 0
    assert np.array_equal(_bits(s["tracer"].render(*maps, spp=6, max_depth=16, seed=5, spp_per_launch=4)), _bits(out))
    # a table without textures renders through the new entry to the bits of matpbr_path_render_objects_colors (the four new arguments NULL / 0)
    refs = {}
    for name, objects in (("colors", pc.table_scene()), ("rough", pr.table_scene()), ("unflagged", px.table_scene(flagged=False))):
        tracer = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV, objects=objects)
        assert tracer.textures is None and tracer.stats["n_textured_objects"] == 0
        ref, got = torch.empty(H, W, 3, device=tracer.device), torch.empty(H, W, 3, device=tracer.device)
        keep1, a1 = _raw_args(tracer, maps, 6, 16, 5, 4, ref)
        nine = tl.object_tail(tracer, "matpbr_path_render_objects_colors")
        assert len(nine) == 9 and colors(*a1, *nine) == 0
        keep2, a2 = _raw_args(tracer, maps, 6, 16, 5, 4, got)
        assert textures(*a2, *nine, None, None, None, 0) == 0
        assert np.array_equal(_bits(got), _bits(ref)), name
        assert np.array_equal(_bits(tracer.render(*maps, spp=6, max_depth=16, seed=5, spp_per_launch=4)), _bits(ref)), name
        refs[name] = ref
    # all images (1, 1, 1): the paths of the unflagged table through the parent's kernel; at most 16 vertices contribute, each a few ulp
    # apart between two instantiations of the kernel: 1e-5 relative
    uniform = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV, objects=px.table_scene(uniform=True))
    assert uniform.stats["n_textured_objects"] == 3
    got = uniform.render(*maps, spp=6, max_depth=16, seed=5, spp_per_launch=4).cpu().numpy().astype(np.float64)
    ref = refs["unflagged"].cpu().numpy().astype(np.float64)
    rel = np.abs(got - ref) / np.maximum(np.abs(ref), np.abs(ref).mean())
    equal = bool(np.array_equal(got, ref))
    _report("uniform images against the unflagged table through the parent's kernel: worst relative difference (bound 1e-5); bit-equal", f"{rel.max():.3e}; {equal}")
    assert rel.max() <= 1e-5
    # and the textured table differs from it
    assert np.abs(s["tracer"].render(*maps, spp=6, max_depth=16, seed=5, spp_per_launch=4).cpu().numpy() - ref).max() > 1e-2


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_feature_tints_and_the_guide(pt, scene):
    """`feature_tints` on the device equals its CPU twin bit for bit (the barycentrics are formed without contraction on both, the
    coordinate and the fetch with explicit fmaf alone); the albedo guide multiplies a textured object's constant by it."""
    from materialist_amd import relight

    s = scene
    H, W = s["H"], s["W"]
    got = s["tracer"].feature_tints()
    Vm, Tm, tb, tint, tex = pt.merge_objects(s["rm"]["vertices"], s["rm"]["triangles"], s["objects"], colors=True, textures=True)
    n_scene = s["rm"]["triangles"].shape[0]
    host = pt.feature_tints_host(pt.build_bvh(Vm, Tm, n_scene), H, W, FOV, tb, tint, tex, n_scene)
    assert np.array_equal(_bits(got), host.view(np.uint32))
    geom = s["tracer"].features()
    ids = geom[..., 7].cpu().numpy()
    assert set(np.unique(ids)) >= {0.0, 1.0, 2.0, 3.0, 4.0}
    flagged = (ids == 1) | (ids == 2) | (ids == 3)
    assert np.all(host[~flagged] == 1.0) and all(host[ids == k].std() > 0.05 for k in (1, 2, 3))
    # the older guide still works on this tracer (the flag is hidden from it): the vertex colours alone
    only = s["tracer"].feature_colors().cpu().numpy()
    assert np.all(only[ids != 3] == 1.0) and only[ids == 3].std() > 0.05
    bsdfs = [ob["bsdf"] for ob in s["objects"]]
    alb = torch.as_tensor(s["a"])
    plain = relight.albedo_guide(geom, alb, bsdfs).cpu().numpy()
    guide = relight.albedo_guide(geom, alb, bsdfs, got).cpu().numpy()
    assert np.array_equal(guide[~flagged], plain[~flagged])
    assert np.allclose(guide[ids == 1], np.float32(px.DIFFUSE_BASE["reflectance"]) * host[ids == 1], rtol=1e-6, atol=0)
    assert np.allclose(guide[ids == 2], np.float32(px.PBR_BASE["albedo"]) * host[ids == 2], rtol=1e-6, atol=0)
    # a tracer without a flagged object: (1, 1, 1) everywhere
    plain_tracer = pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], H, W, FOV, objects=pp.table_scene())
    assert bool((plain_tracer.feature_tints() == 1.0).all())


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals_through_pathtracer(pt, scene):
    s = scene
    maps = (s["a"], s["r"], s["m"], s["env"])
    H, W, rm = s["H"], s["W"], s["rm"]
    Vc, Tc = po.cube((0.0, 0.0, -1.2), 0.1, (0.0, 0.0, 0.0))
    uv, img = np.full((8, 2), 0.5), np.full((2, 2, 3), 0.5)
    build = lambda **ob: pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV, objects=[{"vertices": Vc, "triangles": Tc, **ob}])
    for bsdf in (po.GLASS, pl.QUAD_LIGHT, pr.FROSTED_02):
        with pytest.raises(ValueError, match="diffuse"):
            build(bsdf=bsdf, uv=uv, texture=img)
    with pytest.raises(ValueError, match="'uv' without an image"):
        build(bsdf=po.DIFFUSE_08, uv=uv)
    with pytest.raises(ValueError, match="without 'uv'"):
        build(bsdf=po.DIFFUSE_08, texture=img)
    with pytest.raises(ValueError, match="'orm_texture'"):
        build(bsdf=po.DIFFUSE_08, uv=uv, texture=img, orm_texture=img)
    with pytest.raises(ValueError, match="vertex 2"):
        build(bsdf=po.DIFFUSE_08, uv=np.where(np.arange(8)[:, None] == 2, 65.0, uv), texture=img)
    with pytest.raises(ValueError, match="row 1, column 0"):
        build(bsdf=po.DIFFUSE_08, uv=uv, texture=np.where((np.arange(4) == 2).reshape(2, 2, 1), 1.5, img))
    with pytest.raises(ValueError, match="objects"):
        s["tracer"].render(*maps, spp=1, normal=np.zeros((H, W, 3), np.float32))
    with pytest.raises(ValueError, match="objects"):
        s["tracer"].render_bwd(*maps, torch.zeros(H, W, 3))
    # every entry from before the flag refuses the textured table; the new one refuses it without its coordinates, records or texels
    out = torch.empty(H, W, 3, device=s["tracer"].device)
    keep, args = _raw_args(s["tracer"], maps, 1, 2, 0, 1, out)
    for entry in ("matpbr_path_render_objects", "matpbr_path_render_objects_normals", "matpbr_path_render_objects_pbr",
                  "matpbr_path_render_objects_lights", "matpbr_path_render_objects_rough", "matpbr_path_render_objects_colors"):
        assert pt.symbol(entry)(*args, *tl.object_tail(s["tracer"], entry)) == -1, entry
    tail = tl.object_tail(s["tracer"], "matpbr_path_render_objects_textures")
    new = pt.symbol("matpbr_path_render_objects_textures")
    for k in (9, 10, 11):
        assert new(*args, *(None if j == k else x for j, x in enumerate(tail))) == -1, k
    assert new(*args, *tail[:12], tail[12] - 1) == -1 and new(*args, *tail[:11], tail[11] + 4, tail[12]) == -1
    # a library from before the feature: PathError at construction, naming the entry
    real = pt.symbol

    class Old:
        pass

    try:
        pt.symbol = lambda name, lib=None: real(name, Old() if name in pt.TEXTURE_SYMBOLS else lib)
        with pytest.raises(pt.PathError, match="matpbr_path_render_objects_textures"):
            pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV, objects=px.table_scene())
        pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV, objects=px.table_scene(flagged=False))
    finally:
        pt.symbol = real


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_render_final_cli_textured_ply(pt, tmp_path):
    """`render_final.py --mode oi --oi_scene` with a textured PLY and PNGs written here: the bits of the direct PathTracer calls;
    `--denoise atrous` gives a finite image; `--oi_texture` textures oi2.ply on the default route, to the bits of the direct calls."""
    from PIL import Image

    from materialist_amd import mesh, relight
    from materialist_amd.imageio_exr import read_exr

    tmp = str(tmp_path)
    scene_dir = tl.synthetic_output(tmp)
    Vb, Tb = po.cube((0.02, 0.0, -0.9), 0.12, (0.4, 0.5, 0.3))
    Vb = Vb.astype(np.float32)
    UV = np.random.default_rng(7).uniform(-1.5, 2.5, (8, 2))
    os.makedirs(os.path.join(tmp, "lists"))
    ply = os.path.join(tmp, "lists", "crate.ply")
    _write_ply(ply, Vb, Tb, UV, "binary_little_endian", "float", ("u", "v"))
    rng = np.random.default_rng(8)
    wood, orm = os.path.join(tmp, "lists", "wood.png"), os.path.join(tmp, "lists", "wood_orm.png")
    Image.fromarray(rng.integers(0, 256, (4, 5, 3), dtype=np.uint8), "RGB").save(wood)
    Image.fromarray(rng.integers(0, 256, (2, 3, 3), dtype=np.uint8), "RGB").save(orm)
    listing = os.path.join(tmp, "lists", "crate.json")
    base = [sys.executable, os.path.join(ROOT, "render_final.py"), "--save_name", "case", "--input_path", tmp, "--save_path", tmp,
            "--mode", "oi", "--spp", "4", "--oi_iters", "2", "--oi_max_depth", "8"]
    mat = relight.load_estimated_brdf(os.path.join(scene_dir, "best_results"))
    env = relight.load_image(os.path.join(scene_dir, "best_results", "envmap.hdr"))
    maps = (mat["albedo"], mat["roughness"], mat["metallic"])
    exr, png = (os.path.join(tmp, "case", "mi_oi_case_envmap" + ext) for ext in (".exr", ".png"))

    def run(extra):
        for path in (exr, png):
            if os.path.exists(path):
                os.remove(path)
        res = subprocess.run(base + list(extra), capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout + res.stderr
        assert os.path.exists(png)
        img = np.ascontiguousarray(read_exr(exr)[..., :3], dtype=np.float32)
        assert np.isfinite(img).all() and (img >= 0).all() and float(img.std()) > 0
        return img

    def direct(bsdf, with_orm, path=ply):
        V, T, U = mesh.read_ply_any(path, uv=True)
        ob = {"vertices": V, "triangles": T, "bsdf": bsdf, "uv": U, "texture": (np.asarray(Image.open(wood)) / 255.0) ** 2.2}
        if with_orm:
            ob["orm_texture"] = np.asarray(Image.open(orm)) / 255.0
        tracer = relight._path_tracer(scene_dir, "case", mat, "cuda", [ob])
        assert tracer.stats["n_textured_objects"] == 1
        acc = torch.zeros_like(mat["albedo"])
        for seed in (0, 1):
            acc += tracer.render(*maps, env, spp=4, max_depth=8, seed=seed)
        return (acc / 2).cpu().numpy()

    with open(listing, "w") as f:
        json.dump({"objects": [{"ply": "crate.ply", "bsdf": px.PBR_BASE, "texture": "wood.png", "orm_texture": "wood_orm.png"}]}, f)
    img = run(["--oi_scene", listing])
    assert np.array_equal(img.view(np.uint32), direct(px.PBR_BASE, True).view(np.uint32))
    run(["--oi_scene", listing, "--denoise", "atrous"])
    # the default route: oi2.ply, the diffuse object of reflectance 0.8, textured by --oi_texture
    _write_ply(os.path.join(scene_dir, "oi2.ply"), Vb, Tb, UV, "ascii", "float", ("s", "t"))
    img2 = run(["--oi_texture", wood])
    assert np.array_equal(img2.view(np.uint32), direct({"type": "diffuse", "reflectance": (0.8, 0.8, 0.8)}, False, os.path.join(scene_dir, "oi2.ply")).view(np.uint32))
    assert np.abs(img2 - img).max() > 1e-3
