"""The differential render's references in fp64 ("Differential render"), for tests/test_gpu_path_diff.py and
tests/test_path_diff_host.py.  No library code: two walks of `path_objects_fp64.replay_objects`, over the merged mesh with its table
and over `merged(V, T, [])` without one (that call rounds the vertices to fp32 as the merged one does; over the unrounded mesh two
thirds of the pixels would differ spuriously), and the camera ray's coverage by `path_fp64.brute`.  A plain module: nothing pytest
collects."""
import math

import numpy as np

import path_fp64 as pf
import path_objects_fp64 as pob
import path_oi_fp64 as po

HIDDEN_CUBE = ((0.0, 0.0, -6.0), 0.2, (0.0, 0.0, 0.0))              # behind the depth mesh: no path meets it
VISIBLE_CUBE = ((0.02, 0.0, -0.9), 0.12, (0.4, 0.5, 0.3))            # in front of `path_testlib.synthetic_output`'s mesh


def cube_object(place, bsdf=po.DIFFUSE_08):
    V, T = po.cube(*place)
    return {"vertices": V, "triangles": T, "bsdf": bsdf}


def camera_rays(H, W, seed, sample=0, pixels=None):
    """The render's camera ray of sample `sample` of every pixel (or of the flat indices `pixels`) -> (o [N,3], d [N,3])."""
    pix = np.arange(H * W, dtype=np.uint32) if pixels is None else np.asarray(pixels, dtype=np.uint32)
    base = pf.pcg(pf.pcg(pf.pcg(np.uint32(seed)) + pix) + np.uint32(sample))
    f = (W / 2.0) / math.tan(math.radians(pf.FOV) / 2.0)
    x = (pix % W) - 0.5 + pf.rng_u(base, 0, 0)
    y = (pix // W) - 0.5 + pf.rng_u(base, 0, 1)
    d = np.stack([(x - (W - 1) / 2) / f, -(y - (H - 1) / 2) / f, -np.ones(pix.size)], -1)
    return np.zeros((pix.size, 3)), d / np.linalg.norm(d, axis=-1, keepdims=True)


def covered(s, seed, sample=0):
    """c_ref [H,W] bool: the camera ray's closest hit on the merged mesh is an inserted triangle."""
    o, d = camera_rays(s["H"], s["W"], seed, sample)
    return (pf.brute(s["V"][s["T"]], o, d)[1] >= s["n_scene"]).reshape(s["H"], s["W"])


def scene_only(s):
    """The depth mesh of scene `s` alone, rounded as the merged one is -> (V, T)."""
    if "scene_only" not in s:
        s["scene_only"] = pob.merged(s["rm"]["vertices"], s["rm"]["triangles"], [])[:2]
    return s["scene_only"]


def reference(o64, s, tab, max_depth, seed, sample=0):
    """-> {"with": L_with [H,W,3], "without": L_without, "c": c_ref [H,W] bool, "fg", "delta", "alpha": the three outputs of one sample,
    "scale" [H,W,1]: what an error is taken relative to, max(|L_with|, |L_without|, mean |L_with|) of the worst channel's own}.  Computed
    once per (max_depth, seed, sample) of a scene and kept in it."""
    key = ("reference", max_depth, seed, sample)
    if key not in s:
        args = (s["a"], s["r"], s["m"], s["env"], tab, s["H"], s["W"], max_depth, seed)
        Lw, _ = pob.replay_objects(o64, s["V"], s["T"], *args, s["table"], sample=sample)
        V0, T0 = scene_only(s)
        L0, _ = pob.replay_objects(o64, V0, T0, *args, (), sample=sample)
        c = covered(s, seed, sample)
        s[key] = {"with": Lw, "without": L0, "c": c, "fg": np.where(c[..., None], Lw, 0.0), "delta": np.where(c[..., None], 0.0, Lw - L0),
                  "alpha": c.astype(np.float64), "scale": np.maximum(np.maximum(np.abs(Lw), np.abs(L0)), np.abs(Lw).mean())}
    return s[key]


def share_within(got, ref, scale, bound):
    """The error of the worst channel relative to `scale` -> (share of pixels within `bound`, the errors [H,W])."""
    err = (np.abs(got - ref) / scale).max(-1)
    return float((err <= bound).mean()), err


def meets_object_anywhere(o64, s, tab, max_depth, seed):
    """The loosest possible touch rule, [H,W] bool: some ray of the pixel's sample 0, camera, bounce or shadow, meets an inserted triangle
    at any distance, in front of the depth mesh or behind it.  One-lane replays over the merged mesh with a recording `closest=`."""
    key = ("anywhere", max_depth, seed)
    if key not in s:
        P = s["V"][s["T"]]
        P_obj = P[s["n_scene"]:]
        out = np.zeros(s["H"] * s["W"], bool)
        for p in range(out.size):
            met = [False]

            def closest(o, d):
                met[0] = met[0] or bool(np.isfinite(pf.brute(P_obj, o, d)[0]).any())
                return pf.brute(P, o, d)

            pob.replay_objects(o64, s["V"], s["T"], s["a"], s["r"], s["m"], s["env"], tab, s["H"], s["W"], max_depth, 0, s["table"],
                               closest=closest, lanes=([p], [seed], [0]))
            out[p] = met[0]
        s[key] = out.reshape(s["H"], s["W"])
    return s[key]


def any_path_returns_object(o64, s, tab, max_depth, seeds, spp):
    """True where a traversal of some path of `seeds` x samples 0..spp-1 of some pixel returns an inserted triangle (a closest hit, or a
    shadow ray's occluder): one walk over every lane with a recording `closest=`."""
    P = s["V"][s["T"]]
    met = [False]

    def closest(o, d):
        t, k = pf.brute(P, o, d)
        met[0] = met[0] or bool((k >= s["n_scene"]).any())
        return t, k

    n = s["H"] * s["W"]
    pix, sd, smp = np.meshgrid(np.arange(n), np.asarray(seeds), np.arange(spp), indexing="ij")
    pob.replay_objects(o64, s["V"], s["T"], s["a"], s["r"], s["m"], s["env"], tab, s["H"], s["W"], max_depth, 0, s["table"], closest=closest,
                       lanes=(pix.reshape(-1), sd.reshape(-1), smp.reshape(-1)))
    return met[0]
