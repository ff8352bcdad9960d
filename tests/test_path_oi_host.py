"""Host side of object insertion ("Inserted objects"): the fp64 restatement against the one without objects,
the builder that keeps an inserted mesh's winding, the object BSDF sampler the kernel runs (on the CPU) against fp64, the general
PLY reader, and the command line's new flags.  No GPU needed."""
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
import path_oi_fp64 as po  # noqa: E402
import path_testlib as tl  # noqa: E402

ETA = 1.49 / 1.000277


@pytest.fixture(scope="module")
def path_lib():
    return tl.load()


_report = tl.reporter("path oi", "test_path_oi_host")


@pytest.fixture(scope="module")
def groove(path_lib):
    from materialist_amd import mesh

    H, W = 20, 24
    rm = mesh.reference_mesh(pf.groove_scene(H, W), pf.FOV)
    rng = np.random.default_rng(11)
    a, r, m = pf.groove_maps(H, W, rng)
    env = pf.groove_env(rng)
    return {"V": rm["vertices"], "T": rm["triangles"], "a": a, "r": r, "m": m, "env": env, "tab": path_lib.env_tables(env), "H": H, "W": W}


def test_restatement_without_objects_is_the_restatement(groove, oracle64):
    g = groove
    V = g["V"].astype(np.float32).astype(np.float64)
    for seed, depth in ((0, 4), (5, 6)):
        args = (oracle64, V, g["T"], g["a"], g["r"], g["m"], g["env"], g["tab"], g["H"], g["W"], depth, seed)
        ref, rec0 = pf.replay(*args)
        got, rec1 = po.replay_oi(*args)
        assert np.array_equal(ref, got)
        assert len(rec0["vertices"]) == len(rec1["vertices"]) and not rec1["object_vertices"]
        assert not rec1["transmitted"].any() and not rec1["diffuse_object"].any() and not rec1["blocked_by_object"].any()


# ---- the builder --------------------------------------------------------------------------------------------------------------------
def _records(bvh):
    """triangle id -> its 48 bytes"""
    raw = bvh["tris"].reshape(-1, 48)
    ids = raw.view(np.int32).reshape(-1, 12)[:, 3]
    return {int(i): raw[k].tobytes() for k, i in enumerate(ids)}


def test_builder_keeps_the_winding_of_inserted_meshes(groove, path_lib):
    g = groove
    V, T = g["V"], g["T"]
    n_scene = T.shape[0]
    old = path_lib.build_bvh(V, T)
    same = path_lib.build_bvh(V, T, n_scene)
    assert old["nodes"].tobytes() == same["nodes"].tobytes() and old["tris"].tobytes() == same["tris"].tobytes()
    assert (old["n_nodes"], old["depth"], old["n_leaves"]) == (same["n_nodes"], same["depth"], same["n_leaves"])
    # a cube appended: its far faces' e1 x e2 points away from the camera, which the depth mesh's builder would turn round
    centre = np.array([0.03, -0.02, -1.2])
    Vc, Tc = po.cube(centre, 0.25, (0.4, 0.5, 0.3))
    Vm, Tm, table = path_lib.merge_objects(V, T, [{"vertices": Vc, "triangles": Tc, "bsdf": po.GLASS}])
    assert (table[0].first_tri, table[0].n_tri, table[0].kind) == (n_scene, 12, path_lib.BSDF_DIELECTRIC)
    bvh = path_lib.build_bvh(Vm, Tm, n_scene)
    rng = np.random.default_rng(3)
    d = rng.normal(size=(200, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = centre - 0.6 * d                                             # outside the cube (half diagonal 0.22), in front of the mesh
    o = o[o[:, 2] > -1.55]
    t, k = path_lib.trace_host(bvh, o, (centre - o) / np.linalg.norm(centre - o, axis=-1, keepdims=True))
    assert o.shape[0] > 100 and np.all((k >= n_scene) & (k < n_scene + 12)) and np.all(t < 0.6)
    assert len(set(k.tolist())) >= 8                                # rays from all round reach most of its faces
    tf = bvh["tris"].view(np.float32).reshape(-1, 3, 4)
    ids = bvh["tris"].view(np.int32).reshape(-1, 12)[:, 3]
    ob = ids >= n_scene
    assert ob.sum() == 12
    nrm = np.cross(tf[ob, 1, :3].astype(np.float64), tf[ob, 2, :3].astype(np.float64))
    mid = tf[ob, 0, :3] + (tf[ob, 1, :3] + tf[ob, 2, :3]) / 3.0
    assert np.all((nrm * (mid - centre)).sum(-1) > 0), "e1 x e2 of an inserted triangle is its outward normal"
    assert np.any((nrm * mid).sum(-1) > 0), "the far faces point away from the camera: the winding was kept"
    # the depth mesh's triangles are what they were, wherever the leaves put them
    r0, r1 = _records(old), _records(bvh)
    assert all(r0[i] == r1[i] for i in range(n_scene)) and len(r1) == n_scene + 12
    # an object triangle with an index outside the vertex array
    bad = Tm.copy()
    bad[-1, 2] = Vm.shape[0]
    lib = path_lib.load()
    nodes, tris = np.zeros(bad.shape[0] * 64, np.uint8), np.zeros(bad.shape[0] * 48, np.uint8)
    outs = [ctypes.c_long(0), ctypes.c_int(0), ctypes.c_long(0)]
    P = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    code = lib.matpbr_path_bvh_build_objects(P(Vm), Vm.shape[0], P(bad), bad.shape[0], n_scene, P(nodes), bad.shape[0], P(tris),
                                             *(ctypes.cast(ctypes.byref(x), ctypes.c_void_p) for x in outs))
    assert code == -1
    with pytest.raises(path_lib.PathError):
        path_lib.build_bvh(Vm, Tm, Tm.shape[0] + 1)                  # more scene triangles than triangles


# ---- the object BSDFs ---------------------------------------------------------------------------------------------------------------
def _directions(n, cos_o, rng):
    """unit wo with n . wo = cos_o, at random azimuths"""
    tng = np.cross(n, [0.3, -0.5, 0.8])
    tng /= np.linalg.norm(tng)
    bit = np.cross(n, tng)
    ph = rng.uniform(0, 2 * np.pi, cos_o.shape[0])
    s = np.sqrt(1 - cos_o ** 2)
    return cos_o[:, None] * n + (s * np.cos(ph))[:, None] * tng + (s * np.sin(ph))[:, None] * bit


def test_object_sampler_matches_fp64(path_lib):
    """Tolerance 1e-5 absolute on O(1) quantities: fp32 rounding over a few dozen operations.  The grid of cosines stays 1e-3 in
    sin^2 theta_t away from the critical angle, where cos_t = sqrt(1 - sin^2 theta_t) is ill-conditioned in any precision."""
    rng = np.random.default_rng(5)
    n = np.array([0.36, -0.48, 0.8])
    tol = 1e-5
    worst = 0.0
    # outside (entering): every angle; inside (leaving): both sides of the critical angle, 1e-3 in sin^2 theta_t clear of it
    c_out = np.r_[1.0, np.linspace(0.02, 0.999, 60)]
    s2_in = np.r_[0.0, np.linspace(0.0, 1.0 / ETA ** 2 - 1e-3 / ETA ** 2, 40), np.linspace(1.0 / ETA ** 2 + 1e-3 / ETA ** 2, 0.9996, 40)]
    cos_o = np.r_[c_out, -np.sqrt(1 - s2_in)]
    tir = np.r_[np.zeros(c_out.size, bool), s2_in * ETA ** 2 > 1]
    assert tir.sum() == 40 and np.all(np.abs((1 - cos_o ** 2) * np.where(cos_o > 0, 1 / ETA ** 2, ETA ** 2) - 1) >= 1e-3 - 1e-12)
    wo = _directions(n, cos_o, rng).astype(np.float32)
    wo64, n32 = wo.astype(np.float64), n.astype(np.float32)
    for u6 in (0.0, 0.99999994):                                    # reflect; refract wherever something is transmitted
        u = np.stack([np.full(cos_o.size, u6), rng.random(cos_o.size), rng.random(cos_o.size)], -1).astype(np.float32)
        wi, w, pdf, flags = path_lib.object_sample_host(po.GLASS, n32, wo, u)
        ewi, ew, eprob, etrans = po.sample_dielectric(1.49, 1.000277, np.broadcast_to(n32.astype(np.float64), wo.shape), wo64, u[:, 0].astype(np.float64))
        assert np.array_equal(flags, 1 + 2 * etrans.astype(np.int32))
        assert np.all(etrans == ((u6 > 0) & ~tir))
        for got, ref in ((wi, ewi), (w, ew[:, None].repeat(3, 1)), (pdf, eprob)):
            worst = max(worst, float(np.abs(got - ref).max()))
        assert worst <= tol, worst
        cin = (wo64 * n32).sum(-1)
        if u6 == 0.0:
            R = pdf.astype(np.float64)
            assert np.all(w == 1.0)
            assert abs(R[0] - ((ETA - 1) / (ETA + 1)) ** 2) <= tol      # normal incidence
            assert np.all(np.abs(R[tir] - 1.0) <= tol)                 # total internal reflection beyond asin(1/eta) from inside
            np.testing.assert_allclose((wi * n32).sum(-1), cin, atol=tol)      # mirrored about n
        else:
            tr = etrans
            assert np.all(w[tir] == 1.0) and np.all(pdf[tir] == 1.0)
            ent, lea = tr & (cin > 0), tr & (cin < 0)
            np.testing.assert_allclose(w[ent], 1 / ETA ** 2, atol=tol)
            np.testing.assert_allclose(w[lea], ETA ** 2, atol=tol)
            np.testing.assert_allclose(np.linalg.norm(wi[tr], axis=-1), 1.0, atol=tol)
            cout = (wi.astype(np.float64) * n32).sum(-1)
            assert np.all(cout[tr] * cin[tr] < 0)                     # on the far side
            nn = n32.astype(np.float64) / np.linalg.norm(n32.astype(np.float64))
            sin = lambda v: np.linalg.norm(v - (v * nn).sum(-1, keepdims=True) * nn, axis=-1)    # (sqrt(1 - cos^2) loses the small angles)
            sin_i, sin_t = sin(wo64), sin(wi.astype(np.float64))
            np.testing.assert_allclose(sin_t[ent], sin_i[ent] / ETA, atol=tol)           # Snell
            np.testing.assert_allclose(sin_t[lea], sin_i[lea] * ETA, atol=tol)
            # R(entering, theta_i) = R(leaving, theta_t): the refracted direction as the view direction on the far side
            back = path_lib.object_sample_host(po.GLASS, n32, wi[tr], u[tr] * np.float32([0, 1, 1]))
            np.testing.assert_allclose(back[2], 1.0 - pdf[tr], atol=2 * tol)
    # diffuse: cosine-weighted about n, weight rho, nothing from inside
    rho = (0.8, 0.55, 0.3)
    N = 400
    u = rng.random((N, 3)).astype(np.float32)
    wo = _directions(n, rng.uniform(0.05, 1.0, N), rng).astype(np.float32)
    wi, w, pdf, flags = path_lib.object_sample_host({"type": "diffuse", "reflectance": rho}, n32, wo, u)
    ewi, epdf = po.sample_diffuse(np.broadcast_to(n32.astype(np.float64), wo.shape), u[:, 1].astype(np.float64), u[:, 2].astype(np.float64))
    worst = max(worst, float(np.abs(wi - ewi).max()), float(np.abs(pdf - epdf).max()))
    assert worst <= tol, worst
    np.testing.assert_allclose(pdf, np.maximum((wi * n32).sum(-1), 0) / np.pi, atol=tol)
    assert np.all(flags == 0) and np.array_equal(w, np.broadcast_to(np.float32(rho), w.shape))
    inside = path_lib.object_sample_host({"type": "diffuse", "reflectance": rho}, n32, -wo, u)
    assert np.all(inside[1] == 0.0) and np.all(inside[2] == 0.0)
    _report("object sampler vs fp64: max abs error (bound 1e-5)", f"{worst:.3e}")
    for bad in ({"type": "dielectric", "int_ior": 0.0}, {"type": "dielectric", "ext_ior": -1.0}, {"type": "diffuse", "reflectance": 1.5},
                {"type": "plastic"}):
        with pytest.raises(ValueError):
            path_lib.object_sample_host(bad, n32, wo, u)


# ---- mesh.read_ply_any ---------------------------------------------------------------------------------------------------------------
def test_read_ply_any(tmp_path):
    from materialist_amd import mesh

    V, T = po.cube((0.1, -0.2, -1.3), 0.4, (0.2, 0.3, 0.4))
    V = V.astype(np.float32).astype(np.float64)                        # exact in every file below
    ours = str(tmp_path / "ours.ply")
    mesh.write_ply(ours, V, T)
    V0, T0 = mesh.read_ply(ours)
    same = lambda p: (lambda v, t: np.array_equal(v, V0) and np.array_equal(t, T0) and v.dtype == np.float64 and t.dtype == np.int32)(*mesh.read_ply_any(p))
    assert same(ours)
    head = lambda fmt, props, nf, nv=8: (f"ply\nformat {fmt} 1.0\ncomment made by a test\nelement vertex {nv}\n" + "".join(f"property {p}\n" for p in props) +
                                          f"element face {nf}\nproperty list uchar int vertex_indices\nend_header\n")
    xyz = ["float x", "float y", "float z"]
    p = str(tmp_path / "ascii.ply")
    with open(p, "w") as f:
        f.write(head("ascii", xyz, 12) + "".join(f"{v[0]!r} {v[1]!r} {v[2]!r}\n" for v in V.tolist()) + "".join(f"3 {t[0]} {t[1]} {t[2]}\n" for t in T.tolist()))
    assert same(p)
    faces = np.empty(12, dtype=[("n", "u1"), ("v", "<i4", (3,))])
    faces["n"], faces["v"] = 3, T
    p = str(tmp_path / "f32.ply")
    with open(p, "wb") as f:
        f.write(head("binary_little_endian", xyz, 12).encode() + V.astype("<f4").tobytes() + faces.tobytes())
    assert same(p)
    p = str(tmp_path / "extras.ply")                                   # normals before, colours after the position
    rec = np.zeros(8, dtype=[("nx", "<f4"), ("x", "<f8"), ("y", "<f8"), ("ny", "<f4"), ("z", "<f8"), ("nz", "<f4"), ("red", "u1"), ("s", "<i2")])
    rec["x"], rec["y"], rec["z"], rec["nx"], rec["red"], rec["s"] = V[:, 0], V[:, 1], V[:, 2], 0.5, 200, -3
    props = ["float nx", "double x", "double y", "float32 ny", "float64 z", "float nz", "uchar red", "short s"]
    with open(p, "wb") as f:
        f.write(head("binary_little_endian", props, 12).replace("list uchar int", "list uint8 uint").encode() + rec.tobytes() + faces.tobytes())
    assert same(p)
    p = str(tmp_path / "quad.ply")                                     # the first two triangles as the quad they came from
    q = [int(T[0, 0]), int(T[0, 1]), int(T[0, 2]), int(T[1, 2])]
    assert T[1, 0] == q[0] and T[1, 1] == q[2]
    with open(p, "w") as f:
        f.write(head("ascii", xyz + ["uchar red"], 11) + "".join(f"{v[0]!r} {v[1]!r} {v[2]!r} 7\n" for v in V.tolist()) + f"4 {q[0]} {q[1]} {q[2]} {q[3]}\n" +
                "".join(f"3 {t[0]} {t[1]} {t[2]}\n" for t in T[2:].tolist()))
    assert same(p)
    p = str(tmp_path / "big.ply")
    with open(p, "wb") as f:
        f.write(head("binary_big_endian", xyz, 12).encode() + V.astype(">f4").tobytes())
    with pytest.raises(ValueError, match="big.ply"):
        mesh.read_ply_any(p)
    p = str(tmp_path / "noz.ply")
    with open(p, "w") as f:
        f.write(head("ascii", xyz[:2], 0) + "".join(f"{v[0]!r} {v[1]!r}\n" for v in V.tolist()))
    with pytest.raises(ValueError, match="noz.ply"):
        mesh.read_ply_any(p)


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def test_command_line_takes_the_oi_mode_and_render_oi_wants_a_mesh(tmp_path):
    import render_final
    from materialist_amd import relight

    a = render_final.parse_args(["--save_name", "case", "--mode", "oi", "--oi_iters", "2", "--oi_max_depth", "6"])
    assert (a.mode, a.oi_iters, a.oi_max_depth, a.max_depth) == ("oi", 2, 6, 4)
    d = render_final.parse_args(["--save_name", "case", "--mode", "oi"])
    assert (d.oi_iters, d.oi_max_depth) == (10, 16)
    os.makedirs(tmp_path / "case" / "best_results")
    with pytest.raises(FileNotFoundError, match="oi.ply.*oi2.ply"):
        relight.render_oi("case", input_path=str(tmp_path), save_path=str(tmp_path))
    with pytest.raises(ValueError):
        relight.find_envmap_oi("case", None, str(tmp_path))
    for name in ("envmap.hdr", "envmap_opt.hdr"):
        open(tmp_path / "case" / "best_results" / name, "wb").close()
        assert os.path.basename(relight.find_envmap_oi("case", None, str(tmp_path))) == name
    assert relight.find_envmap_oi("case", "x/y.hdr", str(tmp_path)) == "x/y.hdr"
