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


@pytest.fixture(scope="module")
def groove_rec(oracle64):
    from materialist_amd import mesh, pathtrace

    H = W = 24
    rm = mesh.reference_mesh(pf.groove_scene(H, W), pf.FOV)
    rng = np.random.default_rng(11)
    a, r, m = pf.groove_maps(H, W, rng)
    env = pf.groove_env(rng)
    tab = pathtrace.env_tables(env)
    V = rm["vertices"].astype(np.float32).astype(np.float64)
    L, rec = pf.replay(oracle64, V, rm["triangles"], a, r, m, env, tab, H, W, 4, 1)
    d_out = np.random.default_rng(3).normal(size=(H, W, 3))
    return {"a": a.astype(np.float64), "r": r.astype(np.float64), "m": m.astype(np.float64), "env": env.astype(np.float64), "L": L,
            "rec": rec, "d_out": d_out}


def test_held_radiance_is_the_replay(oracle64, groove_rec):
    g = groove_rec
    held = pf.held_radiance(oracle64, g["rec"], g["a"], g["r"], g["m"], g["env"])
    assert np.allclose(held, g["L"], rtol=1e-10, atol=1e-12)
    assert len(g["rec"]["vertices"]) == 3 and g["rec"]["vertices"][2]["pix"].size > 0      # three surface vertices reached


@pytest.mark.parametrize("key", ["a", "r", "m", "env"])
def test_detached_derivative_matches_central_differences(oracle64, groove_rec, key):
    g = groove_rec
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


def _declarations(header: str):
    text = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"^\s*((?:const\s+)?\w+\*?)\s+(matpbr_path_\w+)\(([^)]*)\);", text, flags=re.M):
        out[name] = (ret, [a.strip() for a in args.split(",") if a.strip() and a.strip() != "void"])
    return out


def test_signatures_match_the_header():
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
    lib = pathtrace.load()
    assert lib.matpbr_path_version() == pathtrace.VERSION == 2


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
