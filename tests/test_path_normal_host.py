"""Host side of the path render's shading normals ("Shading normals"): the restatement
tests/path_normal_fp64.py against central differences of its own held paths, the library's normal-gradient composition (on the CPU)
against the restatement's analytic d f / d n, the restatement's sensitivity to fp32 hit decisions on every render the GPU test
checks, its identity with path_fp64.replay where the map is the face normal, the C ABI, and the refusals.  No GPU needed."""
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

import path_fp64 as pf  # noqa: E402
import path_normal_fp64 as pnf  # noqa: E402
import path_testlib as tl  # noqa: E402


@pytest.fixture(scope="module")
def path_lib():
    return tl.load()


_report = tl.reporter("path normal", "test_path_normal_host")


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


# ---- 1. the restatement's gradient against central differences of the same paths ------------------------------------------------------
@pytest.fixture(scope="module")
def held(path_lib, oracle64):
    s = pnf.normal_scene(path_lib)
    L, rec = pnf.replay_normal(oracle64, s["V"], s["T"], s["a"], s["r"], s["m"], s["env"], s["tab"], s["nrm"], s["H"], s["W"], 4, 1)
    x = {"a": s["a"].astype(np.float64), "r": s["r"].astype(np.float64), "m": s["m"].astype(np.float64), "env": s["env"].astype(np.float64),
         "n": s["nrm"].astype(np.float64)}
    d_out = np.random.default_rng(3).normal(size=(s["H"], s["W"], 3))
    grad = pnf.held_grad_normal(oracle64, rec, x["a"], x["r"], x["m"], x["env"], x["n"], d_out)
    return {"s": s, "L": L, "rec": rec, "x": x, "d_out": d_out, "grad": grad}


def test_held_radiance_is_the_replay_and_the_scene_does_what_it_is_for(oracle64, held):
    h, x = held, held["x"]
    got = pnf.held_radiance_normal(oracle64, h["rec"], x["a"], x["r"], x["m"], x["env"], x["n"])
    assert np.allclose(got, h["L"], rtol=1e-10, atol=1e-12)
    rec, s = h["rec"], h["s"]
    assert len(rec["vertices"]) == 3 and rec["vertices"][2]["pix"].size > 0
    assert rec["below"].sum() >= 5 and rec["nov0"].sum() >= s["planted"].sum() >= 10, (rec["below"].sum(), rec["nov0"].sum())
    assert np.abs(np.linalg.norm(s["nrm"].astype(np.float64), axis=-1) - 1).max() < 1e-6
    # the planted texels look away from their own camera ray; the tilt alone turns no normal that far
    v0 = rec["vertices"][0]
    own = v0["tp"] == rec["pixels"][v0["pix"]]
    nov = (v0["n"] * v0["wo"]).sum(-1)
    assert (nov[own & s["planted"].ravel()[v0["tp"]]] < 0).all()
    # a sample below the sheet ends its path: no later vertex, no escape, of that row
    for k, v in enumerate(rec["vertices"]):
        gone = set(v["pix"][v["below"]].tolist())
        later = set(np.concatenate([w["pix"] for w in rec["vertices"][k + 1:]] + [e["pix"] for e in rec["escapes"] if e["depth"] > k]
                                   + [np.zeros(0, np.int64)]).tolist())
        assert not (gone & later)


@pytest.mark.parametrize("key", ["n", "a", "r", "m", "env"])
def test_detached_derivative_matches_central_differences(oracle64, held, key):
    """test_path_grad_host.py's check and tolerance (1e-6 of the directional derivative; 1e-6 texel by texel), under the normal map,
    for the normal map itself and for the other four."""
    h, x = held, held["x"]
    grad = h["grad"][key]
    rng = np.random.default_rng({"a": 1, "r": 2, "m": 3, "env": 4, "n": 5}[key])
    x0 = x[key]
    delta = rng.normal(size=x0.shape)
    step = 1e-6 * max(1.0, float(np.abs(x0).max()))
    order = ("a", "r", "m", "env", "n")
    F = lambda v: float((h["d_out"] * pnf.held_radiance_normal(oracle64, h["rec"], *[v if k == key else x[k] for k in order])).sum())
    fd = (F(x0 + step * delta) - F(x0 - step * delta)) / (2 * step)
    an = float((grad * delta).sum())
    _report(f"d_{key}: directional derivative, analytic and central difference", f"{an:.9e}, {fd:.9e}")
    assert abs(an) > 1e-3
    assert abs(fd - an) <= 1e-6 * abs(an), (key, fd, an)
    rec = h["rec"]
    hits = np.unique(np.concatenate([v["tp"] for v in rec["vertices"][1:]])) if key != "env" else \
        np.unique(np.concatenate([v["te"][v["em"]] for v in rec["vertices"]]))
    flat = grad.reshape(grad.shape[0] * grad.shape[1], -1) if key != "env" else grad.reshape(-1, 3)
    for t in hits[:: max(1, hits.size // 4)][:4]:
        e = np.zeros_like(x0).reshape(flat.shape)
        e[t, 0] = 1.0
        e = e.reshape(x0.shape)
        fd1 = (F(x0 + step * e) - F(x0 - step * e)) / (2 * step)
        assert abs(fd1 - flat[t, 0]) <= 1e-6 * max(abs(flat[t, 0]), 1e-3 * np.abs(flat).max()), (key, t, fd1, flat[t, 0])


# ---- 2. the library's composition of the normal gradient ---------------------------------------------------------------------------------
def _grad_lanes():
    rng = np.random.default_rng(7)
    N = 8192
    n = _unit(rng.normal(size=(N, 3)))
    wo = _unit(rng.normal(size=(N, 3)))          # n . wo, n . wi and n . h on both sides of zero
    wi = _unit(rng.normal(size=(N, 3)))
    a = rng.uniform(0.05, 0.95, (N, 3))
    r = rng.uniform(0.07, 1.0, N)
    r[::4] = 0.07                                # the pipeline's floor
    m = rng.choice([0.0, 0.3, 1.0], N)
    g = rng.normal(size=(N, 3))
    # lanes near the GGX peak at the floor: h within a few alpha of n
    k = N // 8
    wo[:k] = _unit(n[:k] + 0.6 * rng.normal(size=(k, 3)))
    wi[:k] = _unit(2 * (wo[:k] * n[:k]).sum(-1, keepdims=True) * n[:k] - wo[:k] + 0.01 * rng.normal(size=(k, 3)))
    r[:k] = 0.07
    n = _f32(_unit(_f32(n)))
    return tuple(_f32(v) for v in (n, wo, wi, a, r, m, g))


def test_eval_normal_grad_host_against_the_restatement(path_lib, oracle64):
    """The project's criterion for eval_brdf: error relative to max(|ref|, mean |ref|) <= 1e-3.  The restatement's analytic d f / d n is
    the oracle's (a second derivation of the same formula), to rounding."""
    n, wo, wi, a, r, m, g = _grad_lanes()
    nl, nv, nh = (n * wi).sum(-1), (n * wo).sum(-1), (n * _unit(wi + wo)).sum(-1)
    for c in (nl, nv, nh):
        assert 0.2 < (c > 0).mean() < 0.8
    assert (r == _f32(0.07)).mean() > 0.3
    # the library takes the fp32 normal as the unit vector it stands for (its GGX denominator is the stable form, 1 - NoH^2 from
    # n x h); the literal denominator of the fp64 formula sees |n|^2 = 1 +- 6e-8 against alpha^2 = 2.4e-5 at the floor, so the
    # reference is evaluated at that unit vector
    n_hat = _unit(n)
    ref, (gl, gv, gh) = pnf.dfdn(wi, wo, n_hat, a, r, m, g)
    assert (gl != 0).any() and (gv != 0).any() and (gh != 0).any()
    assert (gl[nl <= 0] == 0).all() and (gv[nv <= 0] == 0).all() and (gh[nh <= 0] == 0).all()
    orc = oracle64.eval_brdf_grad(wi, wo, n_hat, a, r, m, g)[3]
    assert np.abs(orc - ref).max() <= 1e-9 * np.abs(ref).max()
    got = path_lib.eval_normal_grad_host(n, wo, wi, a, r, m, g).astype(np.float64)
    assert np.isfinite(got).all()
    err = (np.abs(got - ref) / np.maximum(np.abs(ref), np.abs(ref).mean())).max(-1)
    floor = r == _f32(0.07)
    _report("eval_normal_grad_host vs fp64: max error relative to max(|ref|, mean |ref|), all lanes / roughness 0.07",
            f"{err.max():.3e} / {err[floor].max():.3e} (lane {err.argmax()})")
    assert err.max() <= 1e-3
    # a gated cosine sends nothing: a lane with all three raw cosines <= 0 gets exactly 0
    dead = (nl <= 0) & (nv <= 0) & (nh <= 0)
    assert dead.sum() > 50 and not got[dead].any()
    assert path_lib.load().matpbr_path_eval_normal_grad_host(*[None] * 7, 0, None) == -1
    with pytest.raises(ValueError, match="same rows"):
        path_lib.eval_normal_grad_host(n, wo[:-1], wi, a, r, m, g)


# ---- 3. the GPU parity test's cap, for the restatement alone ----------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", pnf.SIZES)
def test_restatement_over_fp32_and_fp64_traversal(path_lib, oracle64, H, W):
    """The GPU parity test lets 1 % of the pixels differ by more than 1e-3: paths whose hit decisions differ between fp32 and fp64.
    The restatement over the library's fp32 traversal and over the fp64 brute force may differ by more than 1e-3 in at most 0.5 % of
    the pixels of each render the GPU test checks, which leaves the kernel the other half of the cap."""
    s = pnf.normal_scene(path_lib, H, W)
    bvh = path_lib.build_bvh(s["rm"]["vertices"], s["rm"]["triangles"])

    def closest(o, d):
        t, k = path_lib.trace_host(bvh, o, d)
        return np.where(k >= 0, t.astype(np.float64), np.inf), k.astype(np.int64)

    occluded = lambda o, d: path_lib.trace_host(bvh, o, d)[1] >= 0
    worst = 0.0
    for max_depth, seed in pnf.CASES:
        args = (oracle64, s["V"], s["T"], s["a"], s["r"], s["m"], s["env"], s["tab"], s["nrm"], H, W, max_depth, seed)
        ref, rec = pnf.replay_normal(*args)
        got, _ = pnf.replay_normal(*args, closest=closest, occluded=occluded)
        assert np.isfinite(ref).all() and np.isfinite(got).all()
        err = (np.abs(got - ref) / np.maximum(np.abs(ref), np.abs(ref).mean())).max(-1)
        frac = float((err > 1e-3).mean())
        worst = max(worst, frac)
        print(f"[path normal] {W}x{H} max_depth {max_depth} seed {seed}: {int((err > 1e-3).sum())} pixels differ; below {int(rec['below'].sum())}, "
              f"nov0 {int(rec['nov0'].sum())}")
        assert frac <= 0.005, (H, W, max_depth, seed, frac)
        assert rec["below"].any() and rec["nov0"].any(), (H, W, max_depth, seed)
    _report(f"restatement over fp32 traversal vs fp64 brute force at {W}x{H}: largest share of pixels that differ by more than 1e-3 (6 renders)",
            f"{worst:.4f}")


def test_face_normals_as_the_map_on_a_plane_is_the_plain_replay(path_lib, oracle64):
    """One face normal: a fronto-parallel plane.  With the map equal to it at every texel the two normals coincide at every vertex and
    the walk is path_fp64.replay's, to the bit."""
    from materialist_amd import mesh

    H, W = 12, 16
    rm = mesh.reference_mesh(np.full((H, W), 2.0, np.float32), pf.FOV)
    V = rm["vertices"].astype(np.float32).astype(np.float64)
    ng = pnf.face_normals(V, rm["triangles"])
    assert np.array_equal(ng, np.tile([0.0, 0.0, 1.0], (ng.shape[0], 1)))
    rng = np.random.default_rng(11)
    a, r, m = pf.groove_maps(H, W, rng)
    env = pf.groove_env(rng)
    tab = path_lib.env_tables(env)
    nrm = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (H, W, 1))
    for seed in (0, 1):
        x, rec = pnf.replay_normal(oracle64, V, rm["triangles"], a, r, m, env, tab, nrm, H, W, 4, seed)
        y, _ = pf.replay(oracle64, V, rm["triangles"], a, r, m, env, tab, H, W, 4, seed)
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64)) and x.mean() > 0
        assert not rec["nov0"].any()


# ---- 4. the C ABI and the refusals ---------------------------------------------------------------------------------------------------------
def test_signatures_match_the_header(path_lib):
    import ctypes

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "matpbr_path.h")).read(), flags=re.S)
    decl = {name: (ret, [x.strip() for x in args.split(",")])
            for ret, name, args in re.findall(r"^\s*((?:const\s+)?\w+\*?)\s+(matpbr_path_\w+)\(([^)]*)\);", text, flags=re.M)}
    new = ("matpbr_path_render_normals", "matpbr_path_eval_normal_grad_host", "matpbr_path_render_bwd_normals_workspace_bytes",
           "matpbr_path_render_bwd_normals")
    ctype = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t}
    lib = path_lib.load()
    for name in new:
        assert name in decl and name in path_lib.SIGNATURES, name
        assert hasattr(lib, name)
        ret, args = decl[name]
        res, argtypes = path_lib.SIGNATURES[name]
        assert res is ctype[ret] and len(args) == len(argtypes), name
        for arg, t in zip(args, argtypes):
            assert t is (ctypes.c_void_p if "*" in arg else ctype[arg.rsplit(None, 1)[0].replace("const ", "")]), (name, arg)
    # the two *_normals entry points take their plain siblings' arguments first
    for name, plain, extra in (("matpbr_path_render_normals", "matpbr_path_render", 1), ("matpbr_path_render_bwd_normals", "matpbr_path_render_bwd", 2)):
        assert decl[name][1][:-extra] == decl[plain][1] and all("float*" in x for x in decl[name][1][-extra:])
    assert lib.matpbr_path_version() == path_lib.VERSION == 3
    assert lib.matpbr_path_render_bwd_normals_workspace_bytes(24, 20, 8, 16) == lib.matpbr_path_render_bwd_workspace_bytes(24, 20, 8, 16) + 24 * 20 * 3 * 8
    assert lib.matpbr_path_render_bwd_normals_workspace_bytes(0, 20, 8, 16) == 0


def test_refusals(path_lib, tmp_path):
    from materialist_amd import mesh, pipeline, relight, render

    H, W = 8, 8
    rm = mesh.reference_mesh(pf.groove_scene(H, W), pf.FOV)
    rng = np.random.default_rng(0)
    a, r, m = pf.groove_maps(H, W, rng)
    env = pf.groove_env(rng)
    nrm = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (H, W, 1))
    tracer = path_lib.PathTracer(rm["vertices"], rm["triangles"], H, W, pf.FOV, device="cpu")
    with pytest.raises(ValueError, match="normal"):
        tracer.render_bwd(a, r, m, env, np.ones((H, W, 3), np.float32), want=("a", "n"))
    with pytest.raises(ValueError, match=r"\[8,8,3\]"):
        tracer.render(a, r, m, env, normal=nrm[:-1])
    with pytest.raises(ValueError, match="shading normals"):
        tracer.render_trans(a, r, m, env, np.zeros((H, W), bool), np.zeros((H, W, 3), np.float32), normal=nrm)
    cube = {"vertices": np.array([[x, y, z] for z in (-1.3, -1.2) for y in (-0.05, 0.05) for x in (-0.05, 0.05)], np.float64),
            "triangles": np.array([[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2],
                                   [1, 3, 7], [1, 7, 5]], np.int32), "bsdf": {"type": "diffuse", "reflectance": (0.8, 0.8, 0.8)}}
    with_objects = path_lib.PathTracer(rm["vertices"], rm["triangles"], H, W, pf.FOV, device="cpu", objects=[cube])
    with pytest.raises(ValueError, match="objects"):
        with_objects.render(a, r, m, env, normal=nrm)
    # the switch: its values, and "map" is the path integrator's
    scene = render.Scene(H, W, "cpu")
    with pytest.raises(ValueError, match="shading_normals"):
        scene.set_integrator("path", rm["vertices"], rm["triangles"], shading_normals="vertex")
    with pytest.raises(ValueError, match="shading_normals"):
        render.load_estimated_mesh(None, True, height=H, width=W, device="cpu", shading_normals="map")
    for fn in (relight.render_real, lambda *x, **k: relight.render_rolling_envmap(*x, None, **k)):
        with pytest.raises(ValueError, match="shading_normals"):
            fn("case", input_path=str(tmp_path), save_path=str(tmp_path), shading_normals="map")
    with pytest.raises(ValueError, match="--shading_normals"):
        pipeline.inverse_image(str(tmp_path / "missing.png"), "z", opt_order=["an"], save_path=str(tmp_path), shading_normals="map", device="cpu")
    # with the default "face" the path integrator still refuses normals, with the messages it had
    with pytest.raises(ValueError, match="--opt_order"):
        pipeline.inverse_image(str(tmp_path / "missing.png"), "y", opt_order=["an"], save_path=str(tmp_path), integrator="path", device="cpu")
    with pytest.raises(ValueError, match="use_mesh_normal=True"):
        render.Scene(H, W, "cpu", use_mesh_normal=False).set_integrator("path", rm["vertices"], rm["triangles"])
    assert not (tmp_path / "y").exists() and not (tmp_path / "z").exists()


def test_command_lines_refuse_map_without_path(tmp_path):
    import inverse_img_w_mi
    import render_final

    a = inverse_img_w_mi.parse_args(["--img_inverse_path", "x.png", "--save_name", "x", "--opt_src", "arm"])
    assert a.shading_normals == "face"
    a = inverse_img_w_mi.parse_args(["--img_inverse_path", "x.png", "--save_name", "x", "--opt_src", "arm", "--integrator", "path",
                                     "--shading_normals", "map", "--opt_order", "arm", "n"])
    assert a.shading_normals == "map" and a.opt_order == ["arm", "n"]
    assert render_final.parse_args(["--save_name", "x", "--mode", "real"]).shading_normals == "face"
    assert render_final.parse_args(["--save_name", "x", "--mode", "rolling", "--integrator", "path", "--shading_normals", "map"]).shading_normals == "map"
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    inv = [sys.executable, os.path.join(ROOT, "inverse_img_w_mi.py"), "--img_inverse_path", str(tmp_path / "missing.png"), "--save_name", "x",
           "--opt_src", "arm", "--save_path", str(tmp_path), "--shading_normals", "map"]
    fin = [sys.executable, os.path.join(ROOT, "render_final.py"), "--save_name", "x", "--input_path", str(tmp_path), "--save_path", str(tmp_path),
           "--shading_normals", "map"]
    for cli in (inv, inv + ["--integrator", "sh", "--opt_order", "arm", "n"], fin + ["--mode", "real"], fin + ["--mode", "real", "--integrator", "sh"],
                fin + ["--mode", "oi", "--integrator", "path"], inv + ["--integrator", "path", "--shading_normals", "vertex"]):
        res = subprocess.run(cli, capture_output=True, text=True, timeout=120, env=env)
        assert res.returncode == 2 and "--shading_normals" in res.stderr, res.stdout + res.stderr
    assert not (tmp_path / "x").exists()
