"""Ratio shadow transfer's references ("Ratio shadow transfer"), for tests/test_path_ratio_host.py and
tests/test_gpu_path_ratio.py.  No library code: the composite's expression in numpy float32, one operation per rounding, and the
experiment that shows what the ratio is for, two pairs of fp64 walks of `path_diff_fp64.reference` over true and over "fitted" maps.
A plain module: nothing pytest collects."""
import numpy as np

import path_diff_fp64 as pd
import path_fp64 as pf
import path_objects_fp64 as pob

H, W = 20, 24                      # the groove's size in every test of the differential render: a partial tile
FITTED_ALBEDO = 0.5                # the "fitted" albedo of the experiment: the true one times this


def composite_additive_f32(fg, delta, alpha, photo, scale):
    """`matpbr_path_composite`'s expression in numpy float32."""
    sc, one, zero = np.float32(scale), np.float32(1), np.float32(0)
    return np.maximum(zero, (fg + delta) * sc + (one - alpha[..., None] * sc) * photo)


def composite_ratio_f32(fg, delta, base, alpha, photo, scale):
    """`matpbr_path_composite_ratio`'s expression in numpy float32 -> (out [H,W,3], the ratio channels [H,W,3] bool).  fmax, not
    maximum: C's fmaxf returns the other operand for a NaN (a base whose product with scale underflows to 0)."""
    sc, one, zero = np.float32(scale), np.float32(1), np.float32(0)
    bg = (one - alpha[..., None] * sc) * photo
    with np.errstate(divide="ignore", invalid="ignore"):
        B, D = base * sc, delta * sc
        g = np.fmax(zero, B + D) / B
        dark = np.fmax(zero, fg * sc + bg * g)
    ratio = (delta < 0) & (base > 0)
    out = np.where(ratio, dark, composite_additive_f32(fg, delta, alpha, photo, scale))
    assert out.dtype == np.float32
    return out, ratio


def composite_ratio_f64(fg, delta, base, alpha, photo):
    """The same composite of fp64 means (scale 1), for the experiment."""
    bg = (1.0 - alpha[..., None]) * photo
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.maximum(0.0, base + delta) / base
    ratio = (delta < 0) & (base > 0)
    return np.where(ratio, np.maximum(0.0, fg + bg * np.where(ratio, g, 0.0)), np.maximum(0.0, fg + delta + bg))


def groove_scene(objects, env_tables):
    """`path_testlib.groove_with_objects` without a tracer (no GPU), with what `path_diff_fp64.reference` reads besides."""
    from materialist_amd import mesh

    rm = mesh.reference_mesh(pf.groove_scene(H, W), pf.FOV)
    rng = np.random.default_rng(11)
    a, r, m = pf.groove_maps(H, W, rng)
    env = pf.groove_env(rng)
    V, T, table = pob.merged(rm["vertices"], rm["triangles"], objects)
    return {"rm": rm, "a": a, "r": r, "m": m, "env": env, "H": H, "W": W, "objects": objects, "V": V, "T": T, "table": table,
            "n_scene": rm["triangles"].shape[0], "tab": env_tables(env)}


def experiment(o64, s, max_depth, seeds, spp):
    """The true maps are scene `s`'s, the fitted ones the same with the albedo times FITTED_ALBEDO.  Over samples 0..spp-1 of `seeds`, in
    fp64 -> {"shadow": the flat indices of the shadow pixels, the uncovered pixels (c = 0 in every sample) whose true delta is negative
    in every channel, and over them, [N,3] each: "photo": the true-map mean of L_without, "truth": the true-map mean of L_with, "delta",
    "base": the fitted maps' sums (fg and alpha are 0 there), "additive", "ratio": the two composites of the photograph from them}.  The
    true maps' walks run over every pixel (they say where the shadow is), the fitted maps' over the shadow pixels' lanes alone."""
    n = len(seeds) * spp
    photo, truth, alpha = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W))
    for seed in seeds:
        for sample in range(spp):
            t = pd.reference(o64, s, s["tab"], max_depth, seed, sample)
            photo += t["without"] / n
            truth += t["with"] / n
            alpha += t["alpha"] / n
    shadow = np.flatnonzero(((alpha == 0) & (truth - photo < 0).all(-1)).reshape(-1))
    sd, smp, pix = (x.reshape(-1) for x in np.meshgrid(np.asarray(seeds), np.arange(spp), shadow, indexing="ij"))
    fitted = ((np.asarray(s["a"], np.float64) * FITTED_ALBEDO).astype(s["a"].dtype), s["r"], s["m"], s["env"], s["tab"], H, W, max_depth, 0)
    with_f = pob.replay_objects(o64, s["V"], s["T"], *fitted, s["table"], lanes=(pix, sd, smp))[0].reshape(n, shadow.size, 3).mean(0)
    base = pob.replay_objects(o64, *pd.scene_only(s), *fitted, (), lanes=(pix, sd, smp))[0].reshape(n, shadow.size, 3).mean(0)
    zero3, zero1 = np.zeros((1, shadow.size, 3)), np.zeros((1, shadow.size))
    m = {"shadow": shadow, "photo": photo.reshape(-1, 3)[shadow], "truth": truth.reshape(-1, 3)[shadow], "delta": with_f - base, "base": base}
    m["additive"] = np.maximum(0.0, m["delta"] + m["photo"])
    m["ratio"] = composite_ratio_f64(zero3, m["delta"][None], base[None], zero1, m["photo"][None])[0]
    return m


def shadow_errors(m):
    """-> (the mean absolute error against the truth over the shadow pixels of the additive composite, of the ratio composite)."""
    return float(np.abs(m["additive"] - m["truth"]).mean()), float(np.abs(m["ratio"] - m["truth"]).mean())
