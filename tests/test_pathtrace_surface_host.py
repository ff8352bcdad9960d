"""The surface of `materialist_amd.pathtrace` after its split into path_abi, path_scene, path_host and path_filters: every name the
one-file module had still resolves there, the symbol groups partition what the header declares, and the two calls of each folded
filter step (NAME_host on numpy arrays, NAME on the device) refuse the same inputs with the same words before a device is touched.
CPU only.  Bit equality of the two calls is the GPU tests' (test_gpu_denoise.py, test_gpu_diff_denoise.py, test_gpu_path_diff.py)."""
import os
import re

import numpy as np
import pytest

import path_testlib as tl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the top-level names of pathtrace.py before the split (its functions, classes and assignments: 120), without the private ones that no
# other module uses: every public name, `_FEATURE`, and the helpers the new modules take from each other
NAMES = """_P NODE_BYTES TRI_BYTES MAX_BVH_DEPTH MAX_OBJECTS BSDF_DIELECTRIC BSDF_DIFFUSE BSDF_PBR PBR_MIN_ROUGHNESS PBR_DEFAULTS BSDF_AREA
BSDF_ROUGH_DIELECTRIC ROUGH_MIN_ALPHA ROUGH_MIN_CONTRAST OBJECT_SMOOTH OBJECT_COLORED OBJECT_TEXTURED OBJECT_FLAGS TEXTURE_MAX_SIDE
TEXTURE_MAX_UV PathObject PathObjectPbr PathObjectTex PathLights PathTransEdit PathDenoise SIGNATURES VERSION MAX_BWD_ENV_TEXELS
SMOOTH_SYMBOLS DENOISE_SYMBOLS PBR_SYMBOLS LIGHT_SYMBOLS ROUGH_SYMBOLS COLOR_SYMBOLS TEXTURE_SYMBOLS DIFF_SYMBOLS DIFF_DENOISE_SYMBOLS
THROUGH_SYMBOLS LATE_SYMBOLS _FEATURE OBJECT_ENTRIES DENOISE_DEFAULTS PathError load symbol check _ptr _rows _same_rows _table_ptrs
_uncolored _tex_ptrs build_bvh trace_host trace_scene_host through_chain_host env_tables env_sample_host object_bsdf light_tables
light_sample_host light_pdf_host merge_objects object_lookup_host object_sample_host object_normal_host object_color_host
object_texture_host _aligned_texels object_sample_shading_host rough_sample_host rough_eval_host trans_edit trans_eval_host
trans_lookup_host eval_normal_grad_host denoise_params _host_image features_host feature_colors_host feature_tints_host denoise_prepare_host
denoise_level_host denoise_prepare denoise_level denoise composite_host composite denoise_diff_prepare_host denoise_diff_level_host
denoise_diff_finish_host denoise_diff_host denoise_diff_prepare denoise_diff_level denoise_diff_finish denoise_diff PathTracer PathRenderFn
PathTables""".split()

# group -> the feature `symbol` names when a library lacks one of its symbols, in the order of LATE_SYMBOLS
GROUPS = {"SMOOTH_SYMBOLS": "smooth inserted objects", "DENOISE_SYMBOLS": "the denoiser", "PBR_SYMBOLS": "PBR inserted objects",
          "LIGHT_SYMBOLS": "emissive inserted objects", "ROUGH_SYMBOLS": "rough dielectric inserted objects",
          "COLOR_SYMBOLS": "vertex-coloured inserted objects", "TEXTURE_SYMBOLS": "textured inserted objects",
          "DIFF_SYMBOLS": "the differential render", "DIFF_DENOISE_SYMBOLS": "the differential render's denoiser",
          "THROUGH_SYMBOLS": "the photograph seen through inserted glass"}


@pytest.fixture(scope="module")
def path_lib():
    return tl.load()


def test_every_name_of_the_one_file_module_resolves(path_lib):
    assert len(NAMES) == len(set(NAMES)) == 100
    assert [name for name in NAMES if not hasattr(path_lib, name)] == []


def test_the_groups_partition_the_late_symbols_of_the_header(path_lib):
    with open(os.path.join(ROOT, "include", "matpbr_path.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(matpbr_path_\w+)\s*\(", text))
    assert set(path_lib.SIGNATURES) == declared, set(path_lib.SIGNATURES) ^ declared
    groups = [getattr(path_lib, name) for name in GROUPS]
    assert all(isinstance(g, tuple) and g and set(g) <= declared for g in groups)
    assert sum(len(g) for g in groups) == len(set().union(*groups)) == 43                      # pairwise disjoint
    assert path_lib.LATE_SYMBOLS == sum(groups, ())                                             # the same contents in the same order
    assert path_lib._FEATURE == {name: what for g, what in zip(groups, GROUPS.values()) for name in g}


H, W = 5, 7


def _good():
    rng = np.random.default_rng(0)
    f = lambda *shape: rng.random(shape).astype(np.float32)
    triple = lambda: (f(H, W, 3), f(H, W, 3), f(H, W))
    A, B = triple(), triple()
    return {"A": A, "B": B, "fg": A[0], "delta": A[1], "alpha": A[2], "half_b": B[0], "geom": f(H, W, 8), "alb": f(H, W, 3), "cv": f(H, W, 4),
            "cov": f(H, W), "photo": f(H, W, 3), "scale": 1.0, "level": 0}


def _with(i, x, t):
    return tuple(x if k == i else y for k, y in enumerate(t))


# (the step, its arguments in order, [(what is wrong, argument, its bad value as a function of the good one, the words of the refusal)])
STEPS = [
    ("composite", ("fg", "delta", "alpha", "photo", "scale"),
     [("photo", "photo", lambda x: x[..., :2], "photo must be [H,W,3], got [5, 7, 2]"), ("image", "alpha", lambda x: x[:-1], "alpha must be [5, 7], got [4, 7]"),
      ("image", "delta", lambda x: x[:, :-1], "delta must be [5, 7, 3], got [5, 6, 3]"), ("scale", "scale", lambda x: 0.0, "scale must be finite and positive"),
      ("scale", "scale", lambda x: float("nan"), "scale must be finite and positive")]),
    ("denoise_prepare", ("fg", "half_b", "geom"),
     [("geom", "geom", lambda x: x[..., :7], "geom must be [H,W,8], got [5, 7, 7]"), ("image", "half_b", lambda x: x[1:], "B must be [5, 7, 3], got [4, 7, 3]")]),
    ("denoise_level", ("cv", "geom", "alb", "level"),
     [("geom", "geom", lambda x: x[0], "geom must be [H,W,8], got [7, 8]"), ("image", "alb", lambda x: x[..., :1], "alb must be [5, 7, 3], got [5, 7, 1]"),
      ("level", "level", lambda x: 8, "level must lie in 0..7, got 8")]),
    ("denoise_diff_prepare", ("A", "B", "geom", "scale"),
     [("geom", "geom", lambda x: x[..., :7], "geom must be [H,W,8]"), ("triple", "A", lambda t: t[:2], "A and B must be (fg, delta, alpha) triples"),
      ("triple", "B", lambda t: _with(2, t[0], t), "B[2] (alpha) must be [5, 7], got [5, 7, 3]"), ("scale", "scale", lambda x: -1.0, "scale must be finite and positive")]),
    ("denoise_diff_level", ("cv", "cov", "geom", "alb", "level"),
     [("geom", "geom", lambda x: x[..., :7], "geom must be [H,W,8]"), ("image", "cov", lambda x: x[..., None], "cov must be [5, 7], got [5, 7, 1]"),
      ("image", "alb", lambda x: x[:-1], "alb must be [5, 7, 3], got [4, 7, 3]"), ("level", "level", lambda x: -1, "level must lie in 0..7, got -1")]),
    ("denoise_diff_finish", ("cv", "cov", "A", "B", "geom", "scale"),
     [("geom", "geom", lambda x: x[..., :7], "geom must be [H,W,8]"), ("image", "cov", lambda x: x[:-1], "cov must be [5, 7], got [4, 7]"),
      ("triple", "B", lambda t: t + t[:1], "A and B must be (fg, delta, alpha) triples"),
      ("triple", "B", lambda t: _with(1, t[1][:-1], t), "B[1] (delta) must be [5, 7, 3], got [4, 7, 3]"), ("scale", "scale", lambda x: 0.0, "scale must be finite and positive")]),
    ("denoise_diff", ("A", "B", "alb", "geom", "scale"),
     [("geom", "geom", lambda x: x[..., :7], "geom must be [H,W,8]"), ("triple", "A", lambda t: t[:2], "A and B must be (fg, delta, alpha) triples"),
      ("triple", "A", lambda t: _with(1, t[1][:-1], t), "A[1] (delta) must be [5, 7, 3], got [4, 7, 3]"),
      ("image", "alb", lambda x: x[:, 1:], "alb must be [5, 7, 3], got [5, 6, 3]"), ("scale", "scale", lambda x: float("inf"), "scale must be finite and positive")]),
]


@pytest.mark.parametrize("step", STEPS, ids=[s[0] for s in STEPS])
def test_the_two_calls_of_a_step_refuse_alike_before_the_device(path_lib, monkeypatch, step):
    """NAME_host and NAME over CPU arrays: the same ValueError text for a wrong geom (the frame), image, triple, scale or level.  Every
    way to the device or into the library raises AssertionError here, so a ValueError came before them."""
    import torch

    from materialist_amd import path_filters

    def touched(*_a, **_k):
        raise AssertionError("the refusal comes before the device and the library")

    monkeypatch.setattr(torch.Tensor, "to", touched)
    monkeypatch.setattr(torch, "empty", touched)
    monkeypatch.setattr(torch.cuda, "current_stream", touched)
    monkeypatch.setattr(path_filters, "symbol", touched)
    name, order, cases = step
    kinds = {c[0] for c in cases}
    assert kinds & {"geom", "photo"} and kinds & {"image", "triple"}        # the frame and an image inside it, for every step
    for _, arg, spoil, words in cases:
        good = _good()
        good[arg] = spoil(good[arg])
        args = [good[k] for k in order]
        said = []
        for fn in (getattr(path_lib, name + "_host"), getattr(path_lib, name)):
            with pytest.raises(ValueError) as e:
                fn(*args)
            said.append(str(e.value))
        assert said[0] == said[1] and words in said[0], (name, arg, said)
    with pytest.raises(AssertionError, match="before the device"):          # and a good call does go on to them
        good = _good()
        getattr(path_lib, name)(*[good[k] for k in order])
