"""The path render's gradient on the CPU ("Gradients"): the detached derivative of the fp64 restatement
against central differences of the same paths with their sampling held, the C ABI of the backward pass as the binding declares it,
and the inversion command line's refusal of what the path render cannot do."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import path_fp64 as pf  # noqa: E402


def _groove(oracle64, edge=False, H=24, W=24):
    from materialist_amd import mesh, pathtrace

    rm = mesh.reference_mesh(pf.groove_scene(H, W), pf.FOV)
    rng = np.random.default_rng(11)
    a, r, m = pf.groove_maps(H, W, rng)
    env = pf.groove_env(rng)
    if edge:   # the clamps the pipeline feeds: roughness at its floor, black-metal texels, a sun of 1000
        r[:] = 0.07
        black = (np.add.outer(np.arange(H), np.arange(W)) % 3 == 0)
        a[black], m[black] = 0.0, 1.0
        env[1, 3] = [1000.0, 950.0, 900.0]
    tab = pathtrace.env_tables(env)
    V = rm["vertices"].astype(np.float32).astype(np.float64)
    L, rec = pf.replay(oracle64, V, rm["triangles"], a, r, m, env, tab, H, W, 4, 1)
    d_out = np.random.default_rng(3).normal(size=(H, W, 3))
    return {"a": a.astype(np.float64), "r": r.astype(np.float64), "m": m.astype(np.float64), "env": env.astype(np.float64), "L": L,
            "rec": rec, "d_out": d_out, "V": V, "T": rm["triangles"], "tab": tab, "H": H, "W": W, "maps32": (a, r, m, env)}


@pytest.fixture(scope="module")
def groove_rec(oracle64):
    return _groove(oracle64)


@pytest.fixture(scope="module")
def edge_rec(oracle64):
    return _groove(oracle64, edge=True)


def test_held_radiance_is_the_replay(oracle64, groove_rec):
    g = groove_rec
    held = pf.held_radiance(oracle64, g["rec"], g["a"], g["r"], g["m"], g["env"])
    assert np.allclose(held, g["L"], rtol=1e-10, atol=1e-12)
    assert len(g["rec"]["vertices"]) == 3 and g["rec"]["vertices"][2]["pix"].size > 0      # three surface vertices reached


def test_a_subset_replay_is_the_full_replays_rows(oracle64, groove_rec):
    g = groove_rec
    a, r, m, env = g["maps32"]
    sel = np.random.default_rng(2).permutation(g["H"] * g["W"])[:97]
    for sample in (0, 2):
        full, rec_full = pf.replay(oracle64, g["V"], g["T"], a, r, m, env, g["tab"], g["H"], g["W"], 4, 1, sample=sample)
        part, rec = pf.replay(oracle64, g["V"], g["T"], a, r, m, env, g["tab"], g["H"], g["W"], 4, 1, pixels=sel, sample=sample)
        assert part.shape == (sel.size, 3)
        assert np.array_equal(part.view(np.uint64), full.reshape(-1, 3)[sel].view(np.uint64)), sample
        # the records replay those rows too, and their gradient is the full one's for a d_out that only those pixels carry
        held = pf.held_radiance(oracle64, rec, g["a"], g["r"], g["m"], g["env"])
        assert np.array_equal(held, pf.held_radiance(oracle64, rec_full, g["a"], g["r"], g["m"], g["env"]).reshape(-1, 3)[sel])
        d_out = np.zeros_like(g["d_out"]).reshape(-1, 3)
        d_out[sel] = g["d_out"].reshape(-1, 3)[sel]
        d_out = d_out.reshape(g["d_out"].shape)
        gp = pf.held_grad(oracle64, rec, g["a"], g["r"], g["m"], g["env"], d_out)
        gf = pf.held_grad(oracle64, rec_full, g["a"], g["r"], g["m"], g["env"], d_out)
        for k in gp:
            np.testing.assert_allclose(gp[k], gf[k], rtol=1e-12, atol=1e-12 * np.abs(gf[k]).max())
    # another sample index draws other paths
    other, _ = pf.replay(oracle64, g["V"], g["T"], a, r, m, env, g["tab"], g["H"], g["W"], 4, 1, pixels=sel, sample=1)
    assert not np.array_equal(other, part)


def test_held_radiance_is_the_replay_for_later_samples(oracle64, groove_rec):
    g = groove_rec
    a, r, m, env = g["maps32"]
    for sample in (1, 5):
        L, rec = pf.replay(oracle64, g["V"], g["T"], a, r, m, env, g["tab"], g["H"], g["W"], 4, 1, sample=sample)
        assert np.allclose(pf.held_radiance(oracle64, rec, g["a"], g["r"], g["m"], g["env"]), L, rtol=1e-10, atol=1e-12)
    # spp 3: the mean of samples 0..2, and held_radiance / held_grad of the record list are the mean of theirs
    L3, recs = pf.replay_spp(oracle64, g["V"], g["T"], a, r, m, env, g["tab"], g["H"], g["W"], 4, 1, 3)
    assert len(recs) == 3
    assert np.allclose(pf.held_radiance(oracle64, recs, g["a"], g["r"], g["m"], g["env"]), L3, rtol=1e-10, atol=1e-12)
    g3 = pf.held_grad(oracle64, recs, g["a"], g["r"], g["m"], g["env"], g["d_out"])
    g1 = [pf.held_grad(oracle64, x, g["a"], g["r"], g["m"], g["env"], g["d_out"]) for x in recs]
    for k in g3:
        np.testing.assert_allclose(g3[k], sum(x[k] for x in g1) / 3, rtol=1e-12, atol=1e-15)
    c = pf.contributions(recs)
    assert c["maps"].sum() == sum(v["pix"].size for x in recs for v in x["vertices"])


def test_camera_consistent_texel_lookup(oracle64):
    """The texel a hit reads is the inverse of the render's camera: the surface point under a pixel's centre reads that pixel's own
    texel at every H, W (the deterministic render's identity, DESIGN a6), which a6 world_to_screen with fov_x gives only at H = W."""
    for H, W in ((24, 24), (20, 36), (36, 20), (21, 35)):
        i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        depth = 1.5 + 0.3 * np.random.default_rng(H).random((H, W))
        p = np.stack([oracle64.pixel_to_world(int(a), int(b), float(z), H, W, pf.FOV) for a, b, z in zip(i.ravel(), j.ravel(), depth.ravel())])
        assert np.array_equal(pf.texel(oracle64, p, H, W), np.arange(H * W)), (H, W)
        if H != W:
            x6 = np.array([oracle64.world_to_screen(q, np.deg2rad(pf.FOV), W / H, 0.01, 10000.0, W, H) for q in p])
            own = (np.clip(np.floor(x6[:, 1]), 0, H - 1) * W + np.clip(np.floor(x6[:, 0]), 0, W - 1)).astype(np.int64) == np.arange(H * W)
            assert own.mean() < 0.1, (H, W, own.mean())


def _central_differences(oracle64, g, key):
    grad = pf.held_grad(oracle64, g["rec"], g["a"], g["r"], g["m"], g["env"], g["d_out"])[key]
    rng = np.random.default_rng({"a": 1, "r": 2, "m": 3, "env": 4}[key])
    x0 = g[key]
    delta = rng.normal(size=x0.shape)
    h = 1e-6 * max(1.0, float(np.abs(x0).max()))
    F = lambda x: float((g["d_out"] * pf.held_radiance(oracle64, g["rec"], *[x if k == key else g[k] for k in ("a", "r", "m", "env")])).sum())
    fd = (F(x0 + h * delta) - F(x0 - h * delta)) / (2 * h)
    an = float((grad * delta).sum())
    assert abs(an) > 1e-3
    assert abs(fd - an) <= 1e-6 * abs(an), (key, fd, an)
    # and texel by texel on a few texels that receive gradient from a bounce, not only from their own camera vertex
    hits = np.unique(np.concatenate([v["tp"] for v in g["rec"]["vertices"][1:]])) if key != "env" else \
        np.unique(np.concatenate([v["te"][v["em"]] for v in g["rec"]["vertices"]]))
    flat = grad.reshape(grad.shape[0] * grad.shape[1], -1) if key != "env" else grad.reshape(-1, 3)
    for t in hits[:: max(1, hits.size // 4)][:4]:
        e = np.zeros_like(x0).reshape(flat.shape)
        e[t, 0] = 1.0
        e = e.reshape(x0.shape)
        fd1 = (F(x0 + h * e) - F(x0 - h * e)) / (2 * h)
        assert abs(fd1 - flat[t, 0]) <= 1e-6 * max(abs(flat[t, 0]), 1e-3 * np.abs(flat).max()), (key, t, fd1, flat[t, 0])


@pytest.mark.parametrize("key", ["a", "r", "m", "env"])
def test_detached_derivative_matches_central_differences(oracle64, groove_rec, key):
    _central_differences(oracle64, groove_rec, key)


@pytest.mark.parametrize("key", ["a", "r", "m", "env"])
def test_detached_derivative_at_the_clamps(oracle64, edge_rec, key):
    """Roughness 0.07 everywhere, a third of the texels black metal (a = 0, m = 1: f_s is Schlick's (1 - VoH)^5 term alone), a sun
    of 1000: the same central-difference check."""
    g = edge_rec
    black = (g["a"].max(-1) == 0).ravel()
    assert black.mean() > 0.3 and np.all(g["m"].ravel()[black] == 1.0)
    # black-metal texels are read by bounce vertices, and their gradient is finite there
    tps = np.concatenate([v["tp"] for v in g["rec"]["vertices"][1:]])
    assert black[tps].sum() > 10
    _central_differences(oracle64, g, key)


def _declarations(header: str):
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"^\s*((?:const\s+)?\w+\*?)\s+(matpbr_path_\w+)\(([^)]*)\);", text, flags=re.M):
        out[name] = (ret, [a.strip() for a in args.split(",") if a.strip() and a.strip() != "void"])
    return out


def test_signatures_and_version_match_the_header():
    import ctypes

    from materialist_amd import pathtrace

    decl = _declarations(os.path.join(ROOT, "include", "matpbr_path.h"))
    assert set(decl) == set(pathtrace.SIGNATURES), set(decl) ^ set(pathtrace.SIGNATURES)
    ctype = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t,
             "const char*": ctypes.c_char_p, "double": ctypes.c_double}
    for name, (ret, args) in decl.items():
        res, argtypes = pathtrace.SIGNATURES[name]
        assert res is ctype[ret], (name, ret, res)
        assert len(args) == len(argtypes), (name, args)
        for a, t in zip(args, argtypes):
            base = a.rsplit(None, 1)[0] if not a.endswith("*") else a
            if "*" in a:
                assert t is ctypes.c_void_p, (name, a, t)
            else:
                assert t is ctype[base.replace("const ", "")], (name, a, t)
    assert "matpbr_path_render_bwd" in decl
    # the library, the binding and the header name one version: 3 since the texel lookup at H != W and the backward pass's fp64
    # remainder, so a library built before them is refused
    header_version = int(re.search(r"^#define MATPBR_PATH_VERSION (\d+)", open(os.path.join(ROOT, "include", "matpbr_path.h")).read(), re.M).group(1))
    lib = pathtrace.load()
    assert lib.matpbr_path_version() == pathtrace.VERSION == header_version == 3


def test_cli_rejects_path_with_normals_before_any_gpu_work(tmp_path):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    cli = [sys.executable, os.path.join(ROOT, "inverse_img_w_mi.py"), "--img_inverse_path", str(tmp_path / "missing.png"), "--save_name", "x",
           "--opt_src", "arm", "--save_path", str(tmp_path), "--integrator", "path"]
    for order in (["arm", "n"], ["armn"]):
        res = subprocess.run(cli + ["--opt_order", *order], capture_output=True, text=True, timeout=120, env=env)
        assert res.returncode == 2, res.stdout + res.stderr
        assert "--opt_order" in res.stderr and "--integrator path" in res.stderr, res.stderr
    assert not (tmp_path / "x").exists()
    from materialist_amd import pipeline

    with pytest.raises(ValueError, match="--opt_order"):
        pipeline.inverse_image(str(tmp_path / "missing.png"), "y", opt_order=["an"], save_path=str(tmp_path), integrator="path", device="cpu")
    assert not (tmp_path / "y").exists()
