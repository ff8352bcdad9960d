"""Moving inserted objects on the GPU ("Moving inserted objects"): `matpbr_path_objects_move` against its CPU
twin byte for byte, the render after a move against the fp64 restatement over the fp64-transformed mesh, the same bits by either road,
everything downstream of a move, the features' normals of a spun smooth object, and `render_oi(frames=3)` with its command line."""
import ctypes
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

import path_fp64 as pf  # noqa: E402
import path_light_fp64 as pl  # noqa: E402
import path_move_testlib as ml  # noqa: E402
import path_oi_fp64 as po  # noqa: E402
import path_testlib as tl  # noqa: E402
from path_testlib import bits as _bits  # noqa: E402

pytestmark = pytest.mark.gpu

FOV = pf.FOV
_report = tl.reporter("path move", "test_gpu_path_move")


@pytest.fixture(scope="module")
def pt():
    return tl.load(gpu=True)


@pytest.fixture(scope="module")
def scene(pt):
    """The groove at 24 x 20 with the glass and the diffuse cube, and a movable tracer over it."""
    from materialist_amd import mesh

    H, W = 20, 24
    rm = mesh.reference_mesh(pf.groove_scene(H, W), FOV)
    rng = np.random.default_rng(11)
    a, r, m = pf.groove_maps(H, W, rng)
    objects = po.two_cubes()
    tracer = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV, objects=objects, movable=True, reach=ml.REACH)
    return {"rm": rm, "a": a, "r": r, "m": m, "env": pf.groove_env(rng), "H": H, "W": W, "objects": objects, "tracer": tracer}


def _device_move(pt, g, table, ns, rec, nrm=None, lights=None):
    """`matpbr_path_objects_move` over fresh device copies of a grafted BVH -> what `objects_move_host` returns, read back."""
    dev = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    ptr = lambda x: None if x is None else x.data_ptr()
    nodes, tris, rest, level = dev(g["nodes"]), dev(g["tris"]), dev(g["rest_tris"]), dev(g["node_level"])
    rest_nrm = dev(None if nrm is None else np.asarray(nrm, np.float32))
    out_nrm = None if nrm is None else torch.zeros_like(rest_nrm)
    rest_l = None if lights is None else dev(np.asarray(lights["tris"], np.float32))
    out_l = None if lights is None else torch.zeros_like(rest_l)
    tab, _ = pt._table_ptrs(table)
    pt.check(pt.symbol("matpbr_path_objects_move")(
        nodes.data_ptr(), tris.data_ptr(), rest.data_ptr(), ns, g["rest_tris"].size // 48, g["first_object_node"], g["n_object_nodes"], level.data_ptr(),
        g["object_depth"], tab, len(table), ctypes.cast(rec, ctypes.c_void_p), float(g["pad"]), ptr(rest_nrm), ptr(out_nrm), ptr(rest_l), ptr(out_l),
        0 if lights is None else int(rest_l.shape[0]), None if lights is None else pt._ref(lights["header"]), torch.cuda.current_stream().cuda_stream),
        "matpbr_path_objects_move")
    torch.cuda.synchronize()
    back = lambda x: None if x is None else x.cpu().numpy()
    return {"nodes": back(nodes), "tris": back(tris), "obj_nrm": back(out_nrm), "light_tris": back(out_l)}


def _same_bytes(pt, g, table, ns, rec, nrm=None, lights=None, what=""):
    host = pt.objects_move_host(g, table, ns, rec, nrm, lights)
    got = _device_move(pt, g, table, ns, rec, nrm, lights)
    for key in ("nodes", "tris", "obj_nrm", "light_tris"):
        if host[key] is None:
            assert got[key] is None
            continue
        assert np.array_equal(np.asarray(got[key]).view(np.uint8).reshape(-1), np.asarray(host[key]).view(np.uint8).reshape(-1)), (what, key)
    first = g["first_object_node"]                                    # the scene part is the build's
    assert np.array_equal(got["nodes"][64:64 * first], g["nodes"][64:64 * first]) and np.array_equal(got["nodes"][:24], g["nodes"][:24])
    assert np.array_equal(got["tris"][:48 * ns], g["tris"][:48 * ns])
    return host


@pytest.mark.parametrize("pose", list(ml.POSES))
def test_the_device_move_is_the_host_move_byte_for_byte(pt, scene, pose):
    rm, objects = scene["rm"], scene["objects"]
    V, T, table = pt.merge_objects(rm["vertices"], rm["triangles"], objects)
    ns = rm["triangles"].shape[0]
    g = pt.build_bvh_grafted(V, T, ns, ml.REACH)
    host = _same_bytes(pt, g, table, ns, ml.records(pt, ml.POSES[pose], objects), what=pose)
    assert not np.array_equal(host["tris"], g["tris"])


@pytest.mark.parametrize("case", ["1 triangle", "4 triangles", "5 triangles", "8 objects", "scene of 2", "sliver scene", "sliver object", "smooth and light"])
def test_the_device_move_on_every_layout(pt, scene, case):
    rm = scene["rm"]
    Vs, Ts = rm["vertices"], rm["triangles"]
    Vc, Tc = po.cube((0.10, -0.04, -1.40), 0.20, (-0.3, 0.7, 0.2))
    turn = {"rotate": {"axis": (1, 2, 3), "deg": 37}, "scale": 1.25, "translate": (0.02, 0.01, -0.03)}
    kw, reach = {}, ml.REACH
    if case in ("1 triangle", "4 triangles", "5 triangles"):
        objects = [{"vertices": Vc, "triangles": Tc[:int(case[0])], "bsdf": po.DIFFUSE_08}]
    elif case == "8 objects":
        objects = [{"vertices": Vc + (0.05 * k, 0, 0), "triangles": Tc, "bsdf": po.DIFFUSE_08} for k in range(8)]
    elif case == "scene of 2":
        Vs, Ts = np.array([[-1, -1, -2], [1, -1, -2], [1, 1, -2], [-1, 1, -2]], np.float64), np.array([[0, 1, 2], [0, 2, 3]], np.int32)
        objects = po.two_cubes()
    elif case == "sliver scene":                                      # the scene side at the cap, slot 1 a leaf of one triangle
        Vs, Ts = ml.sliver_mesh()
        objects = [{"vertices": ml.one_triangle()[0], "triangles": ml.one_triangle()[1], "bsdf": po.DIFFUSE_08}]
        reach = None
    elif case == "sliver object":                                     # 39 object nodes, one per level down to the cap
        objects = [{"vertices": ml.sliver_mesh()[0], "triangles": ml.sliver_mesh()[1], "bsdf": po.DIFFUSE_08}]
        turn, reach = {"rotate": {"axis": (0, 0, 1), "deg": 37}, "pivot": (0, 0, -1)}, None
    else:
        Vi, Ti, Ni = ml.icosahedron()
        quad = {"vertices": np.array([[-0.2, 0.5, -1.3], [0.2, 0.5, -1.3], [0.2, 0.5, -1.0], [-0.2, 0.5, -1.0]], np.float64),
                "triangles": np.array([[0, 1, 2], [0, 2, 3]], np.int32), "bsdf": pl.QUAD_LIGHT}
        objects = [{"vertices": Vi, "triangles": Ti, "bsdf": po.DIFFUSE_08, "normals": Ni}, quad, po.two_cubes()[0]]
    if case == "smooth and light":
        V, T, table, nrm, lights = pt.merge_objects(Vs, Ts, objects, normals=True, lights=True)
        kw = {"nrm": nrm, "lights": lights}
    else:
        V, T, table = pt.merge_objects(Vs, Ts, objects)
    ns = Ts.shape[0]
    if reach is None:                                                 # a rotation about z of a mesh that lies along x: within sqrt(2) of its extent
        reach = 1.5 * float(np.abs(V).max())
    g = pt.build_bvh_grafted(V, T, ns, reach)
    transforms = [turn if k % 2 == 0 else None for k in range(len(objects))]
    host = _same_bytes(pt, g, table, ns, ml.records(pt, transforms, objects), what=case, **kw)
    assert not np.array_equal(host["tris"], g["tris"])
    if case == "smooth and light":
        assert not np.array_equal(host["obj_nrm"], nrm) and np.array_equal(host["obj_nrm"][20:], nrm[20:])
        assert np.array_equal(host["light_tris"], np.asarray(lights["tris"], np.float32))     # the light was left at rest
        _same_bytes(pt, g, table, ns, ml.records(pt, [None, turn, turn], objects), what=case + ", the light turned", **kw)
    _same_bytes(pt, g, table, ns, ml.records(pt, [None] * len(objects), objects), what=case + ", identity", **kw)


def test_move_objects_with_a_light(pt, scene):
    """`PathTracer.move_objects` on a tracer with an area light, scaled by 2 and turned: the header's area is (float)((double) area_rest 4),
    the light records on the device are the CPU twin's, and the render is that of a static tracer over the fp64-baked pose by the
    renders' criterion (the two walk other trees over vertices rounded differently, and the baked light's area is rebuilt: 1e-7)."""
    s = scene
    rm, H, W = s["rm"], s["H"], s["W"]
    quad = {"vertices": np.array([[-0.2, 0.5, -1.3], [0.2, 0.5, -1.3], [0.2, 0.5, -1.0], [-0.2, 0.5, -1.0]], np.float64),
            "triangles": np.array([[0, 1, 2], [0, 2, 3]], np.int32), "bsdf": pl.QUAD_LIGHT}
    objects = [po.two_cubes()[1], quad]
    pose = [{"translate": (0.03, 0.0, 0.0)}, {"scale": 2.0, "rotate": {"axis": (0, 0, 1), "deg": 20}, "translate": (0.0, 0.05, 0.0)}]
    tracer = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV, objects=objects, movable=True, reach=ml.REACH)
    rest_area = float(tracer.lights[0].area[0])
    tracer.move_objects(pose)
    assert float(tracer.lights[0].area[0]) == float(np.float32(rest_area * 4.0)) and tracer.stats["n_lights"] == 1
    V, T, table, lights = pt.merge_objects(rm["vertices"], rm["triangles"], objects, lights=True)
    ns = rm["triangles"].shape[0]
    host = pt.objects_move_host(pt.build_bvh_grafted(V, T, ns, ml.REACH, rm["vertices"].shape[0]), table, ns, tracer.poses(pose), None, lights)
    assert np.array_equal(_bits(tracer.lights[1]), host["light_tris"].view(np.uint32))
    assert np.array_equal(tracer.tris.cpu().numpy(), host["tris"]) and np.array_equal(tracer.nodes.cpu().numpy(), host["nodes"])
    baked = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV, objects=ml.moved_objects(pt, objects, tracer.poses(pose)))
    maps = (s["a"], s["r"], s["m"], s["env"])
    for seed in (0, 1):
        got = tracer.render(*maps, spp=16, max_depth=6, seed=seed).cpu().numpy().astype(np.float64)
        ref = baked.render(*maps, spp=16, max_depth=6, seed=seed).cpu().numpy().astype(np.float64)
        frac, err = tl.parity(got, ref)
        _report(f"moved light against the baked pose's static tracer, seed {seed}: share of pixels within 1e-3", f"{frac:.4f} (max err {err.max():.3e})")
        assert frac >= 0.99
    tracer.move_objects([None, None])                                 # and back: the rest area, the rest records
    assert float(tracer.lights[0].area[0]) == rest_area
    assert np.array_equal(_bits(tracer.lights[1]), np.asarray(lights["tris"], np.float32).view(np.uint32))


@pytest.mark.parametrize("pose", ["quarter", "oblique", "double"])
def test_render_after_a_move_matches_an_fp64_restatement(pt, scene, oracle64, pose):
    """tests/test_gpu_path_oi.py's criterion over the fp64-transformed merged mesh: error relative to max(|ref|, mean |ref|), at least
    0.99 of the pixels within 1e-3.  On the CPU twin the restatement over the library's fp32 traversal of the moved BVH and over the
    fp64 brute force disagree in no pixel of these eighteen renders (nor for POSES["away"])."""
    s = scene
    H, W = s["H"], s["W"]
    tab = pt.env_tables(s["env"])
    s["tracer"].move_objects(ml.POSES[pose])
    moved = ml.moved_objects(pt, s["objects"], s["tracer"].poses(ml.POSES[pose]))
    Vm, Tm, table = po.merged(s["rm"]["vertices"], s["rm"]["triangles"], moved)
    for max_depth in (6, 16):
        for seed in (0, 1, 2):
            got = s["tracer"].render(s["a"], s["r"], s["m"], s["env"], spp=1, max_depth=max_depth, seed=seed).cpu().numpy().astype(np.float64)
            assert np.isfinite(got).all()
            ref, rec = po.replay_oi(oracle64, Vm, Tm, s["a"], s["r"], s["m"], s["env"], tab, H, W, max_depth, seed, table)
            frac, err = tl.parity(got, ref)
            _report(f"pose {pose}: per-path parity after the move, max_depth {max_depth} seed {seed}: share of pixels within 1e-3",
                    f"{frac:.4f} ({int((err > 1e-3).sum())} flipped paths, max err {err.max():.3e})")
            assert frac >= 0.99, (pose, max_depth, seed, frac, np.argwhere(err > 1e-3)[:10])
            assert rec["transmitted"].any() and rec["blocked_by_object"].any(), (pose, max_depth, seed)
    s["tracer"].move_objects([None, None])


def test_the_same_bits_by_either_road(pt, scene):
    s = scene
    tr = s["tracer"]
    maps = (s["a"], s["r"], s["m"], s["env"])
    M, N = ml.POSES["oblique"], ml.POSES["double"]
    tr.move_objects(M)
    first = tr.render(*maps, spp=16, max_depth=8, seed=3, spp_per_launch=8)
    for split in (1, 3):                                              # every split into launches gives the same bits after a move
        assert np.array_equal(_bits(first), _bits(tr.render(*maps, spp=16, max_depth=8, seed=3, spp_per_launch=split))), split
    tr.move_objects(N)
    other = tr.render(*maps, spp=16, max_depth=8, seed=3)
    assert not np.array_equal(_bits(first), _bits(other))
    tr.move_objects(M)                                                # M -> N -> M: the bits of the first M, a move starts from the rest pose
    assert np.array_equal(_bits(first), _bits(tr.render(*maps, spp=16, max_depth=8, seed=3)))
    # a tracer whose rest pose is the fp64-baked M, moved by the identity, rounds differently: it need not agree bit for bit, and is held
    # to the renders' parity criterion alone
    baked = pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], s["H"], s["W"], FOV, movable=True, reach=ml.REACH,
                          objects=ml.moved_objects(pt, s["objects"], tr.poses(M)))
    baked.move_objects([None, None])
    frac, err = tl.parity(baked.render(*maps, spp=16, max_depth=8, seed=3).cpu().numpy().astype(np.float64), first.cpu().numpy().astype(np.float64))
    _report("moved to M against a rest pose baked at M: share of pixels within 1e-3 / pixels with other bits",
            f"{frac:.4f} / {int((_bits(first) != _bits(baked.render(*maps, spp=16, max_depth=8, seed=3))).any(-1).sum())}")
    assert frac >= 0.95
    # the rest pose again: the bits of a tracer that never moved, and the merged BVH's picture to the parity criterion
    tr.move_objects([None, None])
    fresh = pt.PathTracer(s["rm"]["vertices"], s["rm"]["triangles"], s["H"], s["W"], FOV, objects=s["objects"], movable=True, reach=ml.REACH)
    assert np.array_equal(_bits(tr.render(*maps, spp=16, max_depth=8, seed=3)), _bits(fresh.render(*maps, spp=16, max_depth=8, seed=3)))
    assert np.array_equal(_bits(tr.nodes), _bits(fresh.nodes)) and np.array_equal(_bits(tr.tris), _bits(fresh.tris))


def test_everything_downstream_sees_the_move(pt, scene):
    s = scene
    tr, H, W = s["tracer"], s["H"], s["W"]
    maps = (s["a"], s["r"], s["m"], s["env"])
    photo = torch.from_numpy(np.random.default_rng(3).random((H, W, 3)).astype(np.float32)).cuda()
    # the diffuse cube slid sideways by 8 pixels' worth at its centre's depth (a pixel is 2 tan(fov / 2) |z| / W wide there), the glass
    # cube out of the picture
    dx = 8 * 2 * np.tan(np.radians(FOV) / 2) * 1.40 / W
    slid = [{"translate": (6.0, 0.0, 0.0)}, {"translate": (-dx, 0.0, 0.0)}]
    rest_in, _ = tl.footprints(s["objects"][1:], H, W)
    tr.move_objects(slid)
    moved = ml.moved_objects(pt, s["objects"], tr.poses(slid))
    inside, outside = tl.footprints(moved[1:], H, W)
    left = rest_in & outside
    assert inside.sum() >= 4 and left.sum() >= 4 and not np.array_equal(inside, rest_in)
    fg, delta, alpha, rewalked = tr.render_diff(*maps, spp=2, max_depth=2, seed=1)
    al = alpha.cpu().numpy()
    assert np.all(al[inside] == 1.0) and np.all(al[outside] == 0.0)                      # alpha's footprint moved with the cube
    img = pt.composite(fg, delta, alpha, photo, 1.0)
    untouched = (rewalked.cpu().numpy() == 0) & (al == 0.0)
    _report("slid cube: pixels it covered at rest and left / of them untouched by any sample", f"{int(left.sum())} / {int((left & untouched).sum())}")
    assert (left & untouched).sum() >= 1
    assert np.array_equal(_bits(img)[untouched], _bits(photo)[untouched])                # the pixels it left keep the photograph's bits
    assert not np.array_equal(_bits(img)[inside], _bits(photo)[inside])
    # every other method runs on the moved scene
    out = tr.render_diff_through(*maps, photo, spp=2, max_depth=4, seed=1)
    assert len(out) == 5 and all(torch.isfinite(x.float()).all() for x in out)
    fg2, delta2, base, alpha2, rw2 = tr.render_diff_ratio(*maps, spp=2, max_depth=2, seed=1)
    assert np.array_equal(_bits(alpha2), _bits(alpha)) and np.array_equal(_bits(fg2), _bits(fg))
    ratio = pt.composite_ratio(fg2, delta2, base, alpha2, photo, 1.0)
    assert torch.isfinite(ratio).all() and np.array_equal(_bits(ratio)[untouched], _bits(photo)[untouched])
    geom = tr.features()
    ids = geom[..., 7].cpu().numpy()
    assert np.all(ids[inside] == 2) and np.all(ids[outside] <= 0)                         # the features' ids follow the cube
    A, B = tr.render_diff(*maps, spp=2, max_depth=2, seed=4)[:3], tr.render_diff(*maps, spp=2, max_depth=2, seed=5)[:3]
    guide = torch.from_numpy(s["a"]).cuda()
    dn = tr.denoise_diff(A, B, guide, geom, 1.0)
    assert all(torch.isfinite(x).all() for x in dn) and np.all(dn[2].cpu().numpy()[inside] == 1.0)
    # both cubes behind the depth mesh (z <= -2.8): no ray finds them, the composite is the photograph bit for bit
    tr.move_objects([{"translate": (0.0, 0.0, -2.0)}, {"translate": (0.0, 0.0, -2.0)}])
    fg, delta, alpha, rewalked = tr.render_diff(*maps, spp=4, max_depth=6, seed=2)
    assert int(rewalked.sum()) == 0 and float(alpha.abs().sum()) == 0.0
    assert np.array_equal(_bits(pt.composite(fg, delta, alpha, photo, 1.0)), _bits(photo))
    tr.move_objects([None, None])


def test_features_of_a_spun_smooth_object(pt, scene):
    """A smooth icosahedron spun 37 degrees about (1, 2, 3) through its centre: where the camera ray through a pixel centre first hits
    it, the features' normal is R times the normal the same routine gives the rest pose at the corresponding ray, R^T (o - c) + c and
    R^T d, to 1e-5 (fp32 rounding of a unit vector's interpolation, a few 1e-7, on either side of the rotation)."""
    s = scene
    rm, H, W = s["rm"], s["H"], s["W"]
    Vi, Ti, Ni = ml.icosahedron()
    objects = [{"vertices": Vi, "triangles": Ti, "bsdf": po.DIFFUSE_08, "normals": Ni}]
    tracer = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV, objects=objects, movable=True)
    spin = [{"rotate": {"axis": (1, 2, 3), "deg": 37}}]
    rest_geom = tracer.features().cpu().numpy()
    tracer.move_objects(spin)
    geom = tracer.features().cpu().numpy()
    on = geom[..., 7] == 1
    assert on.sum() >= 12 and (rest_geom[..., 7] == 1).sum() >= 12
    R, _, _, c = ml.sims64(tracer.poses(spin))[0]
    f = (W / 2.0) / np.tan(np.radians(FOV) / 2.0)
    ii, jj = np.nonzero(on)
    d = np.stack([(jj - (W - 1) / 2) / f, -(ii - (H - 1) / 2) / f, -np.ones(ii.size)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o_rest, d_rest = np.tile(c - R.T @ c, (ii.size, 1)), d @ R                           # R^T (0 - c) + c, R^T d
    V, T, table, nrm = pt.merge_objects(rm["vertices"], rm["triangles"], objects, normals=True)
    ns = rm["triangles"].shape[0]
    rest = pt.build_bvh(V, T, ns)
    t, k = pt.trace_host(rest, o_rest, d_rest)
    hit = k >= ns                                                     # a grazing ray may miss the rest pose by rounding: left out, and counted
    assert hit.mean() >= 0.9
    P = V[T[k[hit]]].astype(np.float32)
    tri = np.stack([P[:, 0], P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]], 1)
    _, _, n_rest = pt.object_normal_host(tri, nrm[k[hit] - ns], o_rest[hit], d_rest[hit])
    # the third fallback, which the features apply as the render does: the face normal where the two normals disagree about the viewer's side
    ng = np.cross(tri[:, 1].astype(np.float64), tri[:, 2].astype(np.float64))
    ng /= np.linalg.norm(ng, axis=-1, keepdims=True)
    sides = (n_rest * -d_rest[hit]).sum(-1) * (ng * -d_rest[hit]).sum(-1)
    assert np.abs(sides).min() > 1e-4                                 # no pixel sits on the rule's threshold
    n_rest = np.where((sides > 0)[:, None], n_rest, ng)
    want = n_rest.astype(np.float64) @ R.T
    got = geom[ii[hit], jj[hit], 4:7].astype(np.float64)
    err = np.abs(got - want).max()
    _report("spun icosahedron: pixels on it / compared / largest difference of a normal's component from R x the rest normal",
            f"{int(on.sum())} / {int(hit.sum())} / {err:.3e}")
    assert err <= 1e-5
    assert np.abs(got - n_rest).max() > 0.1                           # and the spin is seen: the normals are not the rest pose's


def _oi_files(tmp, name="case"):
    """A synthetic output directory with its photograph, two cube files and an object list: one cube spins, one slides."""
    from materialist_amd import mesh
    from materialist_amd.imageio_exr import write_exr

    scene = tl.synthetic_output(tmp, name)
    write_exr(os.path.join(scene, "gt_image.exr"), np.random.default_rng(8).random((32, 32, 3)).astype(np.float32))
    cubes = [po.cube((-0.12, 0.02, -1.2), 0.16, (0.4, 0.5, 0.3)), po.cube((0.12, -0.04, -1.1), 0.14, (-0.3, 0.7, 0.2))]
    for k, (V, T) in enumerate(cubes):
        mesh.write_ply(os.path.join(tmp, f"cube{k}.ply"), V, T)
    entries = [{"ply": "cube0.ply", "bsdf": po.GLASS, "transform": {"rotate": {"axis": [0, 1, 0], "deg": 20}},
                "motion": {"spin": {"axis": [1, 2, 3], "deg_per_frame": 25}}},
               {"ply": "cube1.ply", "bsdf": po.DIFFUSE_08, "transform": {"scale": 1.2, "translate": [0.0, 0.01, 0.0]}, "motion": {"slide": [-0.03, 0.0, 0.01]}}]
    path = os.path.join(tmp, "list.json")
    with open(path, "w") as f:
        json.dump({"objects": entries}, f)
    return scene, path, cubes, entries


def _png(path):
    from PIL import Image

    return np.asarray(Image.open(path))


@pytest.mark.parametrize("route", ["plain", "composite ratio"])
def test_render_oi_frames(pt, tmp_path, route):
    from materialist_amd import loss, mesh, relight
    from materialist_amd.pipeline import write_png

    tmp = str(tmp_path)
    scene, path, cubes, entries = _oi_files(tmp)
    opts = {"composite": True, "shadows": "ratio"} if route != "plain" else {}
    kw = dict(input_path=tmp, spp=4, n_iter=1, max_depth=6, seed=2, objects_file=path, **opts)
    res = relight.render_oi("case", save_path=os.path.join(tmp, "video"), frames=3, **kw)
    assert len(res["frames"]) == 3 and all(os.path.isfile(p) for p in res["frames"]) and res["animation_dir"].endswith("oi_animation")
    tag = "mi_oic_" if opts else "mi_oi_"
    assert os.path.basename(res["mp4"]).startswith(tag) and os.path.getsize(res["mp4"]) > 0 and os.path.getsize(res["gif"]) > 0
    frames = [_png(p) for p in res["frames"]]
    assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[1], frames[2])
    # frame k is a movable tracer moved to pose k and the same render calls
    mat = relight.load_estimated_brdf(os.path.join(scene, "best_results"), "cuda")
    objects = [{"vertices": V, "triangles": T, "bsdf": e["bsdf"]} for (V, T), e in zip(cubes, entries)]
    sims = [[relight.oi_pose(e["transform"], e["motion"], f, pivot=0.5 * (V.min(0) + V.max(0))) for (V, _), e in zip(cubes, entries)] for f in range(3)]
    Vs, Ts = mesh.read_ply(os.path.join(scene, "case.ply"))
    boxes = [(V.min(0), V.max(0)) for V, _ in cubes]                  # `render_oi`'s reach, so that the boxes are padded alike
    reach = max(pt.pose_extent(sim, lo, hi) for per_frame in sims for sim, (lo, hi) in zip(per_frame, boxes)) * (1 + 1e-6)
    tracer = pt.PathTracer(Vs, Ts, 32, 32, FOV, objects=objects, movable=True, reach=reach)
    env = relight.load_image(relight.find_envmap_oi("case", None, tmp))
    tabs = tracer.tables(env)
    photo = relight._oi_photo(scene, None, False, 1.0) if opts else None
    maps = (mat["albedo"], mat["roughness"], mat["metallic"], env)
    for f in range(3):
        tracer.move_objects([{"rotate": R, "scale": s, "translate": t, "pivot": c} for R, s, t, c in sims[f]])
        if opts:
            fg, delta, base, alpha, _ = tracer.render_diff_ratio(*maps, 4, 6, 2, tables=tabs)
            img = pt.composite_ratio(fg, delta, base, alpha, torch.from_numpy(photo).cuda(), 1.0)
        else:
            img = tracer.render(*maps, 4, 6, 2, tables=tabs)
        direct = os.path.join(tmp, f"direct_{f}.png")
        write_png(direct, loss.linear_to_srgb(img.clamp_min(0)).clamp(0, 1).cpu().numpy())
        assert np.array_equal(_png(direct), frames[f]), (route, f)
    # frames=1 with the same list writes the bytes the pre-baked files write
    still = relight.render_oi("case", save_path=os.path.join(tmp, "still"), **kw)
    baked = []
    for k, ((V, T), e) in enumerate(zip(cubes, entries)):
        sim = relight.oi_pose(e["transform"], None, 0, pivot=0.5 * (V.min(0) + V.max(0)))
        mesh.write_ply(os.path.join(tmp, f"baked{k}.ply"), pt.apply_similarity(sim, V), T)
        baked.append({"ply": f"baked{k}.ply", "bsdf": e["bsdf"]})
    with open(os.path.join(tmp, "baked.json"), "w") as f:
        json.dump({"objects": baked}, f)
    ref = relight.render_oi("case", save_path=os.path.join(tmp, "baked"), **dict(kw, objects_file=os.path.join(tmp, "baked.json")))
    for ext in (".png", ".exr"):
        with open(still[:-4] + ext, "rb") as fa, open(ref[:-4] + ext, "rb") as fb:
            assert fa.read() == fb.read(), (route, ext)


def test_render_final_oi_frames_command_line(pt, tmp_path):
    """`render_final.py --mode oi --oi_scene ... --oi_frames 3` in a child process writes what `render_oi(frames=3)` writes."""
    from materialist_amd import relight

    tmp = str(tmp_path)
    scene, path, _, _ = _oi_files(tmp)
    res = relight.render_oi("case", input_path=tmp, save_path=os.path.join(tmp, "lib"), spp=4, n_iter=1, max_depth=6, seed=2, objects_file=path, frames=3)
    cmd = [sys.executable, os.path.join(ROOT, "render_final.py"), "--save_name", "case", "--mode", "oi", "--input_path", tmp, "--save_path", os.path.join(tmp, "cli"),
           "--spp", "4", "--oi_iters", "1", "--oi_max_depth", "6", "--seed", "2", "--oi_scene", path, "--oi_frames", "3"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "Animation saved to" in out.stdout
    for p in res["frames"]:
        q = p.replace(os.path.join(tmp, "lib"), os.path.join(tmp, "cli"))
        assert np.array_equal(_png(p), _png(q)), q
    assert os.path.isfile(res["mp4"].replace(os.path.join(tmp, "lib"), os.path.join(tmp, "cli")))
    bad = subprocess.run(cmd[:-4] + ["--oi_frames", "3"], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "--oi_frames" in bad.stderr
