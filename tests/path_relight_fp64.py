"""The reference of the walk under two environments in fp64 ("Relighting in the photograph"), for
tests/test_gpu_path_relight.py and tests/test_path_relight_host.py.  No library code: two `path_fp64.replay` calls (or two
`path_normal_fp64.replay_normal` calls under a shading-normal map), one per environment, and the property the kernel rests on, asserted
on their records: no decision of the walk reads the envmap, so both replays record the same vertices.  A plain module: nothing pytest
collects."""
import numpy as np

import path_fp64 as pf
import path_mapedit_fp64 as pm
import path_normal_fp64 as pnf

ROLL = 8                                                   # B = A rolled by 8 of its 16 columns
# what a vertex record holds of the walk; "em", "wl", "te", "we" are the emitter sample's, which is each environment's own
WALK = ("depth", "pix", "tp", "wo", "n", "wi", "ip")


def relight_scene(pathtrace):
    """`path_mapedit_fp64.edit_scene` (the groove at 24 x 20, its 8 x 16 envmap A with the sun, the tilted normal map) with B = A rolled
    by 8 columns, a 4 x 8 envmap with a sun of its own and the all-zero envmap Z of A's size, each with its tables."""
    s = pm.edit_scene(pathtrace)
    s["env_b"] = np.ascontiguousarray(np.roll(s["env"], ROLL, axis=1))
    s["env_small"] = pf.groove_env(np.random.default_rng(23), 4, 8)
    s["env_zero"] = np.zeros_like(s["env"])
    for k in ("env_b", "env_small", "env_zero"):
        s["tab" + k[3:]] = pathtrace.env_tables(s[k])
    return s


def same_walk(rec_a, rec_b):
    """AssertionError unless two replays' records hold the same walk: the same vertices (every array of WALK, bit for bit) and the same
    pixel list at every escape."""
    assert len(rec_a["vertices"]) == len(rec_b["vertices"]) and len(rec_a["escapes"]) == len(rec_b["escapes"])
    for va, vb in zip(rec_a["vertices"], rec_b["vertices"]):
        for k in WALK:
            assert np.array_equal(va[k], vb[k]), (va["depth"], k)
    for ea, eb in zip(rec_a["escapes"], rec_b["escapes"]):
        assert ea["depth"] == eb["depth"] and np.array_equal(ea["pix"], eb["pix"]), ea["depth"]


def reference(o64, s, max_depth, seed, sample=0, normal=False, b="env_b", maps=None):
    """-> {"base": the radiance under s["env"], "relit": under s[b], "rec": (the two records)}, the two replays' walks asserted equal.
    `normal`: both under s["nrm"].  `maps`: (a, r, m) in the scene's place.  The scene's own cases are computed once and kept in it."""
    key = ("relight", max_depth, seed, sample, normal, b) if maps is None else None
    if key is not None and key in s:
        return s[key]
    a, r, m = (s["a"], s["r"], s["m"]) if maps is None else maps
    H, W = s["H"], s["W"]

    def walk(env, tab):
        if normal:
            return pnf.replay_normal(o64, s["V"], s["T"], a, r, m, env, tab, s["nrm"], H, W, max_depth, seed, sample=sample)
        return pf.replay(o64, s["V"], s["T"], a, r, m, env, tab, H, W, max_depth, seed, sample=sample)

    La, rec_a = walk(s["env"], s["tab"])
    Lb, rec_b = walk(s[b], s["tab" + b[3:]])
    same_walk(rec_a, rec_b)
    out = {"base": La, "relit": Lb, "rec": (rec_a, rec_b)}
    if key is not None:
        s[key] = out
    return out


def composite(base, relit, photo, scale=1.0, floor=None):
    """The quotient composite in fp64: max(0, photo (relit scale + floor) / (base scale + floor)); floor None: 0.01 x mean(base scale)."""
    B0, B1 = np.asarray(base, np.float64) * scale, np.asarray(relit, np.float64) * scale
    fl = 0.01 * B0.mean() if floor is None else float(floor)
    return np.maximum(0.0, np.asarray(photo, np.float64) * ((B1 + fl) / (B0 + fl)))
