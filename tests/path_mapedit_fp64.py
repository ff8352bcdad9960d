"""The references of the differential render of edited maps in fp64 ("Material edits in the photograph"), for
tests/test_gpu_path_mapedit.py and tests/test_path_mapedit_host.py.  No library code: two `path_fp64.replay` calls (or two
`path_normal_fp64.replay_normal` calls under a shading-normal map), one over the edited maps and one over the fitted ones, and the
touch rule read off the edited replay's record: a sample is touched where some vertex of its walk read a masked texel.  A plain
module: nothing pytest collects."""
import numpy as np

import path_fp64 as pf
import path_normal_fp64 as pnf

FOV = pf.FOV
MASK_ROWS, MASK_COLS = slice(4, 13), slice(3, 10)          # 9 rows x 7 columns of the 20 x 24 frame


def edit_inside(a, r, m, mask, roughness=0.3, metallic=1.0, reverse_albedo=True):
    """The maps with the edit applied where `mask` is set: constant roughness and metallic, the albedo's channels reversed -> (a_e, r_e,
    m_e), copies."""
    a_e, r_e, m_e = a.copy(), r.copy(), m.copy()
    if reverse_albedo:
        a_e[mask] = a[mask][:, ::-1]
    if roughness is not None:
        r_e[mask] = np.float32(roughness)
    if metallic is not None:
        m_e[mask] = np.float32(metallic)
    return a_e, r_e, m_e


def edit_scene(pathtrace):
    """The groove at 24 x 20 (partial 16 x 8 tiles on both axes), built as `path_testlib.groove_with_objects` builds it, without objects
    and without a tracer; the rectangle mask and the edit inside it; the tilted normal map of the same frame."""
    from materialist_amd import mesh

    H, W = 20, 24
    rm = mesh.reference_mesh(pf.groove_scene(H, W), FOV)
    rng = np.random.default_rng(11)
    a, r, m = pf.groove_maps(H, W, rng)
    env = pf.groove_env(rng)
    mask = np.zeros((H, W), bool)
    mask[MASK_ROWS, MASK_COLS] = True
    nrm, _ = pnf.tilted_normals(rm, H, W)
    return {"rm": rm, "a": a, "r": r, "m": m, "env": env, "H": H, "W": W, "mask": mask, "edited": edit_inside(a, r, m, mask), "nrm": nrm,
            "tab": pathtrace.env_tables(env), "V": rm["vertices"].astype(np.float32).astype(np.float64), "T": rm["triangles"]}


def reference(o64, s, max_depth, seed, sample=0, normal=False, edited=None, mask=None):
    """-> {"edited": L_e [H,W,3], "fitted": L_f, "delta": L_e - L_f, "touched" [H,W] bool: the edited walk read a masked texel, "differ"
    [H,W] bool: the two walks' radiances differ, "scale" [H,W,3]: what an error is taken relative to, max(|L_e|, |L_f|, mean |L_e|)}.
    `normal`: both walks under s["nrm"].  The default edit and mask are the scene's; computed once per case and kept in it."""
    key = ("reference", max_depth, seed, sample, normal) if edited is None and mask is None else None
    if key is not None and key in s:
        return s[key]
    edited = s["edited"] if edited is None else edited
    mask = s["mask"] if mask is None else mask
    H, W = s["H"], s["W"]

    def walk(a, r, m):
        if normal:
            return pnf.replay_normal(o64, s["V"], s["T"], a, r, m, s["env"], s["tab"], s["nrm"], H, W, max_depth, seed, sample=sample)
        return pf.replay(o64, s["V"], s["T"], a, r, m, s["env"], s["tab"], H, W, max_depth, seed, sample=sample)

    Le, rec = walk(*edited)
    Lf, _ = walk(s["a"], s["r"], s["m"])
    masked = set(np.flatnonzero(mask.reshape(-1)).tolist())
    touched = np.array([bool(t & masked) for t in pf.touched(rec)[0]]).reshape(H, W)
    out = {"edited": Le, "fitted": Lf, "delta": Le - Lf, "touched": touched, "differ": (Le != Lf).any(-1),
           "scale": np.maximum(np.maximum(np.abs(Le), np.abs(Lf)), np.abs(Le).mean())}
    if key is not None:
        s[key] = out
    return out
