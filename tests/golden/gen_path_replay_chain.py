#!/usr/bin/env python3
"""The recorded predecessors of `path_objects_fp64.replay_objects` (tests/golden/path_replay_chain.npz).

Before the six per-feature copies of the object walk were folded into one, three "chain" tests compared a copy with its predecessor
on one scene.  With one walk left they would compare a function with itself, so the predecessors' output is recorded here instead:
the L and the record arrays each test compares, with exactly each test's arguments (the groove at 12 x 10, max_depth 6, seed 1), plus
`replay_texture` itself on its own table, the walk that was kept.

    entry     function                             table                               compared in
    smooth    path_oi_smooth_fp64.replay_oi        path_oi_smooth_fp64.table_scene()   test_path_oi_pbr_host.py
    pbr       path_oi_pbr_fp64.replay_oi           path_oi_pbr_fp64.table_scene()      test_path_light_host.py
    lights    path_light_fp64.replay_lights        path_light_fp64.table_scene()       test_path_rough_host.py
    texture   path_texture_fp64.replay_texture     path_texture_fp64.table_scene()     test_path_texture_host.py

THIS SCRIPT RUNS ONLY AT THE RECORDED PARENT COMMIT (the fixture's `parent_commit`, the last one that has these four functions): check
it out, then

    python tests/golden/gen_path_replay_chain.py        # writes tests/golden/path_replay_chain.npz

Every array of a record is stored as `<entry>.<key>`, the render as `<entry>.L`."""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

H, W, MAX_DEPTH, SEED = 10, 12, 6, 1


def main():
    import path_fp64 as pf
    import path_light_fp64 as pl
    import path_oi_pbr_fp64 as pp
    import path_oi_smooth_fp64 as ps
    import path_testlib as tl
    import path_texture_fp64 as px
    from materialist_amd import mesh
    from oracle import oracle

    oracle.build()
    o64 = oracle.Oracle(np.float64)
    path_lib = tl.load()
    rm = mesh.reference_mesh(pf.groove_scene(H, W), pf.FOV)
    rng = np.random.default_rng(11)
    a, r, m = pf.groove_maps(H, W, rng)
    env = pf.groove_env(rng)
    tab = path_lib.env_tables(env)
    out = {"parent_commit": subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()}
    for entry, mod, walk in (("smooth", ps, ps.replay_oi), ("pbr", pp, pp.replay_oi), ("lights", pl, pl.replay_lights),
                             ("texture", px, px.replay_texture)):
        V, T, table = mod.merged(rm["vertices"], rm["triangles"], mod.table_scene())
        L, rec = walk(o64, V, T, a, r, m, env, tab, H, W, MAX_DEPTH, SEED, table)
        out[f"{entry}.L"] = L
        out.update({f"{entry}.{k}": v for k, v in rec.items() if isinstance(v, np.ndarray)})
        print(entry, "mean L", L.mean(), "arrays", sum(k.startswith(entry + ".") for k in out))
    np.savez_compressed(os.path.join(HERE, "path_replay_chain.npz"), **out)


if __name__ == "__main__":
    main()
