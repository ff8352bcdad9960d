"""The forward entry points of libmatpbr_path.so as levels of one rule ("The object entries"): a scene renders
to the bits of `PathTracer.render` through every entry at or above its level, called directly with the matching prefix of
`PathTracer.object_args()`, and every entry below its level refuses the table."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import path_color_fp64 as pc  # noqa: E402
import path_light_fp64 as pl  # noqa: E402
import path_medium_fp64 as pm  # noqa: E402
import path_oi_fp64 as po  # noqa: E402
import path_oi_pbr_fp64 as pp  # noqa: E402
import path_oi_smooth_fp64 as ps  # noqa: E402
import path_rough_fp64 as pr  # noqa: E402
import path_testlib as tl  # noqa: E402
import path_texture_fp64 as px  # noqa: E402

pytestmark = pytest.mark.gpu

# level -> the entry (level 0 takes no table)
ENTRIES = ("matpbr_path_render", "matpbr_path_render_objects", "matpbr_path_render_objects_normals", "matpbr_path_render_objects_pbr",
           "matpbr_path_render_objects_lights", "matpbr_path_render_objects_rough", "matpbr_path_render_objects_colors",
           "matpbr_path_render_objects_textures", "matpbr_path_render_objects_media")
# level -> the scene each feature's own tests render
SCENES = (lambda: None, po.two_cubes, ps.table_scene, pp.table_scene, pl.table_scene, pr.table_scene, pc.table_scene, px.table_scene,
          pm.table_scene)
SPP, SPP_PER_LAUNCH, MAX_DEPTH, SEED = 3, 2, 4, 9   # two launches: the first and the last flag are set in different ones


@pytest.fixture(scope="module")
def pt():
    return tl.load(gpu=True)


@pytest.mark.parametrize("level", range(len(SCENES)))
def test_a_scene_renders_alike_through_every_entry_that_admits_it(pt, level):
    s = tl.groove_with_objects(pt, SCENES[level](), lambda V, T, objects: (V, T, None))
    tracer, maps = s["tracer"], (s["a"], s["r"], s["m"], s["env"])
    st = tracer.stats
    assert (st["n_medium_objects"] > 0, st["n_textured_objects"] > 0, st["n_colored_objects"] > 0, st["n_rough_objects"] > 0, st["n_lights"] > 0,
            st["n_pbr_objects"] > 0, st["n_smooth_objects"] > 0, st["n_objects"] > 0, True).index(True) == 8 - level, st
    ref = tl.bits(tracer.render(*maps, spp=SPP, max_depth=MAX_DEPTH, seed=SEED, spp_per_launch=SPP_PER_LAUNCH))
    for at, entry in enumerate(ENTRIES):
        out = torch.full((s["H"], s["W"], 3), float("nan"), device=tracer.device)
        keep, args = tl.raw_args(tracer, maps, SPP, MAX_DEPTH, SEED, SPP_PER_LAUNCH, out)
        code = pt.symbol(entry)(*args, *(tl.object_tail(tracer, entry) if at else ()))
        if at >= level:
            assert code == 0, (entry, code)
            assert np.array_equal(tl.bits(out), ref), entry
        elif at >= 1:   # the table holds a kind the entry does not admit (matpbr_path_render takes no table)
            assert code == -1, (entry, code)
