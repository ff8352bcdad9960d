"""The photograph seen through inserted glass in fp64 ("Seen through glass"), for tests/test_gpu_path_through.py
and tests/test_path_through_host.py.  No library code.  `chain` states the camera chain alone: dielectric vertices from the camera ray
to a landing on the depth mesh's front.  `reference` puts the estimator together from walks that exist: L_with is
`path_objects_fp64.replay_objects` over the merged mesh, and L_tail of a see-through lane is a one-lane replay of the same sample whose
`closest=` answers over every triangle until the first call that returns a depth-mesh triangle (delta vertices trace no shadow rays, so
those calls are exactly the chain) and over the depth mesh's triangles alone from the next call on.  Where nothing of the objects is met
after the landing both tails are the same fp64 arithmetic and their difference is exactly 0, with no touch rule in the reference.  A
plain module: nothing pytest collects."""
import numpy as np

import path_diff_fp64 as pd
import path_fp64 as pf
import path_light_fp64 as pl
import path_objects_fp64 as pob
import path_oi_fp64 as po
import path_oi_smooth_fp64 as ps

FAR_GLASS_CUBE = ((0.42, 0.25, -1.6), 0.22, (0.5, 0.2, 0.6))


def scene_objects(light=False):
    """Scene S: a smooth glass icosphere, a flat glass cube sunk into the depth mesh (the mesh is met inside it: thr_k != 1), a diffuse
    cube behind the sphere and a flat glass cube; `light`: plus `path_light_fp64`'s small area light (S_light)."""
    Vs, Ts, Ns = ps.icosphere((0.02, -0.01, -1.2), 0.2, 1)
    out = [{"vertices": Vs, "triangles": Ts, "bsdf": po.GLASS, "normals": Ns},
           pd.cube_object(((-0.45, 0.2, -2.1), 0.4, (0.2, 0.3, 0.1)), po.GLASS),
           pd.cube_object(((0.12, -0.12, -1.7), 0.15, (0.4, 0.5, 0.3)), po.DIFFUSE_08),
           pd.cube_object(FAR_GLASS_CUBE, po.GLASS)]
    if light:
        Vl, Tl = pl.quad(pl.LIGHT_QUAD)
        out.append({"vertices": Vl, "triangles": Tl, "bsdf": pl.QUAD_LIGHT})
    return out


def photograph(H, W):
    return np.random.default_rng(3).gamma(2.0, 0.5, (H, W, 3)).astype(np.float32)


def chain(o64, s, max_depth, seed, sample=0, pixels=None):
    """The camera chain of sample `sample` of every pixel (or of `pixels`) of scene `s` -> {"k" [N]: the landing depth, -1 where the
    sample is not see-through; "p" [N,3]: the landing point; "thr" [N]: the chain's throughput; "q" [N]: the texel p projects to
    (`path_fp64.texel`); "o", "d" [N,3]: the ray that lands; "covered" [N]: the camera ray's closest hit is an inserted triangle;
    "back" [N]: the chain landed on the sheet's back; "cut" [N]: a chain that was still a chain when max_depth ended it}."""
    H, W, n_scene = s["H"], s["W"], s["n_scene"]
    P = s["V"][s["T"]]
    o, d = pd.camera_rays(H, W, seed, sample, pixels)
    N = o.shape[0]
    pix = np.arange(H * W, dtype=np.uint32) if pixels is None else np.asarray(pixels, dtype=np.uint32)
    base = pf.pcg(pf.pcg(pf.pcg(np.uint32(seed)) + pix) + np.uint32(sample))
    ng_all = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    ng_all *= np.where(((ng_all * P[:, 0]).sum(-1, keepdims=True) > 0) & (np.arange(P.shape[0]) < n_scene)[:, None], -1.0, 1.0)
    ng_all /= np.linalg.norm(ng_all, axis=-1, keepdims=True)
    glass = np.zeros(P.shape[0], bool)
    ior = np.ones((P.shape[0], 2))
    corner = [None] * P.shape[0]
    for ob in s["table"]:
        sl = slice(ob["first_tri"], ob["first_tri"] + ob["n_tri"])
        if ob["bsdf"]["type"] == "dielectric":
            glass[sl], ior[sl] = True, [ob["bsdf"]["int_ior"], ob["bsdf"]["ext_ior"]]
            if ob.get("corner_normals") is not None:
                for j, cn in enumerate(np.asarray(ob["corner_normals"], np.float64)):
                    corner[ob["first_tri"] + j] = cn
    out = {"k": np.full(N, -1), "p": np.zeros((N, 3)), "thr": np.ones(N), "q": np.full(N, -1), "o": np.zeros((N, 3)), "d": np.zeros((N, 3)),
           "covered": np.zeros(N, bool), "back": np.zeros(N, bool), "cut": np.zeros(N, bool)}
    thr = np.ones(N)
    alive = np.ones(N, bool)
    for depth in range(max_depth):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        t, k = pf.brute(P, o[idx], d[idx])
        alive[idx] = False
        if depth == 0:
            out["covered"][idx] = k >= n_scene
        hit = k >= 0
        idx, t, k = idx[hit], t[hit], k[hit]
        p = o[idx] + t[:, None] * d[idx]
        wo = -d[idx]
        ng = ng_all[k]
        if depth >= 1:                                             # a landing on the depth mesh: front or back
            sc = k < n_scene
            front = sc & ((ng * wo).sum(-1) > 0)
            out["back"][idx[sc & ~front]] = True
            ids = idx[front]
            out["k"][ids], out["p"][ids], out["thr"][ids], out["o"][ids], out["d"][ids] = depth, p[front], thr[ids], o[ids], d[ids]
            if ids.size:
                out["q"][ids] = pf.texel(o64, p[front], H, W)
        go = glass[k]                                              # every other kind ends the chain
        if depth + 1 >= max_depth:
            out["cut"][idx[go]] = True
            break
        idx, k, p, wo, ng = idx[go], k[go], p[go], wo[go], ng[go]
        if idx.size == 0:
            break
        ns = ng.copy()
        sm = np.array([corner[j] is not None for j in k], bool)
        if sm.any():
            bu, bv = ps.barycentrics(P[k[sm]], o[idx[sm]], d[idx[sm]])
            ns[sm] = ps.shading_normal(np.stack([corner[j] for j in k[sm]]), bu, bv, ng[sm], wo[sm])[0]
        wi, wgt, _, _, _ = ps.sample_dielectric_shading(ior[k, 0], ior[k, 1], ng, ns, wo, pf.rng_u(base[idx], depth, 6))
        side = np.where((ng * wi).sum(-1) > 0, 1.0, -1.0)
        eps = 1e-5 * (1 + np.abs(p).max(-1))
        thr[idx] *= wgt
        o[idx], d[idx] = p + (side * eps)[:, None] * ng, wi
        alive[idx] = True
    return out


def chains(o64, s, max_depth, seed, sample=0):
    key = ("chain", max_depth, seed, sample)
    if key not in s:
        s[key] = chain(o64, s, max_depth, seed, sample)
    return s[key]


def tail_table(table):
    """The table of the tail's replay: the `area` entries turned into `diffuse`, so that the envmap is the only emitter (n_e = have_tab).
    The chain of a see-through lane never shades them."""
    return [dict(ob, bsdf=po.DIFFUSE_08) if ob["bsdf"]["type"] == "area" else ob for ob in table]


def reference(o64, s, tab, photo, max_depth, seed, sample=0):
    """One sample of every pixel -> {"chain": `chain`'s record, "see" [H,W] bool, "with": L_with, "tail": L_tail (0 off the see-through
    lanes), "fg", "through", "delta", "alpha": the outputs, "scale": `path_diff_fp64.reference`'s}.  Computed once per
    (max_depth, seed, sample) of a scene and kept in it; delta, alpha and the scale are `path_diff_fp64.reference`'s."""
    key = ("through", max_depth, seed, sample)
    if key not in s:
        H, W, n_scene = s["H"], s["W"], s["n_scene"]
        base = pd.reference(o64, s, tab, max_depth, seed, sample)
        ch = chains(o64, s, max_depth, seed, sample)
        see = ch["k"] >= 0
        P = s["V"][s["T"]]
        P_scene = P[:n_scene]
        tail = np.zeros((H * W, 3))
        table = tail_table(s["table"])
        for lane in np.nonzero(see)[0]:
            landed = [False]

            def closest(o, d):
                if landed[0]:
                    return pf.brute(P_scene, o, d)
                t, k = pf.brute(P, o, d)
                landed[0] = bool(((k >= 0) & (k < n_scene)).any())
                return t, k

            L, _ = pob.replay_objects(o64, s["V"], s["T"], s["a"], s["r"], s["m"], s["env"], tab, H, W, max_depth, 0, table, closest=closest,
                                      lanes=([lane], [seed], [sample]))
            tail[lane] = L[0]
        tail = tail.reshape(H, W, 3)
        see = see.reshape(H, W)
        c = base["c"]
        through = np.where(see[..., None], ch["thr"].reshape(H, W, 1) * photo.astype(np.float64).reshape(-1, 3)[np.maximum(ch["q"], 0)].reshape(H, W, 3), 0.0)
        s[key] = {"chain": ch, "see": see, "with": base["with"], "tail": tail, "fg": np.where(c[..., None], base["with"] - tail, 0.0),
                  "through": through, "delta": base["delta"], "alpha": base["alpha"], "scale": base["scale"]}
    return s[key]


def preconditions(s, o64, seeds=(0, 1, 2)):
    """The reference's own preconditions on scene S, asserted first in each test: at sample 0 of `seeds`, at max_depth 6 a see-through
    share of at least 0.2, at least 20 landings with thr_k != 1 and at least 20 at depth 1; at max_depth 3 at least 50 landings whose
    tail max_depth cuts (k + 1 >= max_depth: no second walk can run there)."""
    for seed in seeds:
        c6, c3 = chains(o64, s, 6, seed), chains(o64, s, 3, seed)
        see = c6["k"] >= 0
        assert see.mean() >= 0.2, (seed, see.mean())
        assert (see & (c6["thr"] != 1.0)).sum() >= 20, seed
        assert (c6["k"] == 1).sum() >= 20, seed
        assert (c3["k"] + 1 >= 3).sum() >= 50, seed
