"""The photograph reflected in inserted objects in fp64 ("Reflected in inserted objects"), for
tests/test_gpu_path_reflect.py and tests/test_path_reflect_host.py.  No library code.  `chain` generalises `path_through_fp64.chain` to
the vertices of objects that carry "photo": a dielectric vertex or a flagged one keeps the camera chain, a flagged one with
`path_objects_fp64.replay_objects`' samplers (the depth mesh's BSDF on a pbr object's constants, the cosine sampler, the rough
dielectric's), and thr_k is a colour.  `reference` puts the estimator together from walks that exist:

  * L_with is `replay_objects` over the merged mesh;
  * L_chain of a see-through lane is the same walk cut at max_depth = k + 1: the landing ray is traced, nothing is added at or after it;
  * the tail without the objects is a one-lane replay whose `closest=` (it answers the shadow rays too) is over every triangle up to and
    including the landing ray and over the depth mesh alone after it, with the lights turned off (`path_through_fp64.tail_table`), minus
    the same replay cut at k + 1, so that the chain's own emitter samples cancel;
  * fg = c (L_with - [see-through] tail), which is L_chain + (L_with - L_chain) - tail.

Where nothing of the objects is met after the landing the two tails are the same fp64 arithmetic.  A plain module: nothing pytest
collects."""
import numpy as np

import path_diff_fp64 as pd
import path_fp64 as pf
import path_light_fp64 as pl
import path_objects_fp64 as pob
import path_oi_fp64 as po
import path_oi_pbr_fp64 as pp
import path_oi_smooth_fp64 as ps
import path_through_fp64 as tf
from path_rough_fp64 import rough_params, rough_sample

CHROME = {"type": "pbr", "albedo": (0.95, 0.93, 0.88), "roughness": 0.1, "metallic": 1.0}
FROSTED = {"type": "roughdielectric", "int_ior": 1.49, "ext_ior": 1.000277, "alpha": 0.15}
GREY = {"type": "pbr", "albedo": (0.5, 0.5, 0.5), "roughness": 0.5, "metallic": 0.0}
SPHERE = ((0.2, 0.0, -2.1), 0.33)                                 # inside the groove: what its rim reflects lands on the walls
SUNK_CUBE = ((-0.45, 0.1, -2.15), 0.6, (0.1, 0.15, 0.05))
DIFFUSE_CUBE = ((0.5, 0.3, -2.0), 0.3, (0.5, 0.9, 0.6))
GLASS_CUBE = ((-0.25, 0.08, -1.0), 0.18, (0.1, 0.1, 0.05))           # in front of the sunk cube
FAR_GLASS_CUBE = ((-0.28, -0.3, -1.3), 0.16, (0.4, 0.5, 0.3))         # in front of the bare sheet: chains of glass alone, tails that meet nothing
PBR_CUBE = ((0.3, -0.3, -1.5), 0.12, (0.3, 0.2, 0.5))


def chrome_sphere(photo=True):
    Vs, Ts, Ns = ps.icosphere(*SPHERE, 1)
    return {"vertices": Vs, "triangles": Ts, "bsdf": CHROME, "normals": Ns, "photo": photo}


def scene_objects(light=False, photo=True):
    """Scene R: a flagged smooth chrome icosphere, a flagged rough-glass cube sunk into the depth mesh (thr_k picks up a transmission),
    a flagged diffuse cube turned so that the camera sees its sides, an unflagged clear-glass cube in front of the sunk cube (some chains
    pass glass and a flagged vertex), a second one in front of the bare sheet and an unflagged pbr cube, which ends chains; `light`: plus `path_light_fp64`'s small area light
    (R_light).  `photo=False`: the same objects without the flag."""
    out = [chrome_sphere(photo),
           dict(pd.cube_object(SUNK_CUBE, FROSTED), photo=photo),
           dict(pd.cube_object(DIFFUSE_CUBE, po.DIFFUSE_08), photo=photo),
           pd.cube_object(GLASS_CUBE, po.GLASS),
           pd.cube_object(FAR_GLASS_CUBE, po.GLASS),
           pd.cube_object(PBR_CUBE, GREY)]
    if light:
        Vl, Tl = pl.quad(pl.LIGHT_QUAD)
        out.append({"vertices": Vl, "triangles": Tl, "bsdf": pl.QUAD_LIGHT})
    return out


photograph = tf.photograph


def merged(V, T, objects):
    """`path_objects_fp64.merged` with each table entry carrying its object's "photo"."""
    Vm, Tm, table = pob.merged(V, T, objects)
    for entry, ob in zip(table, objects):
        entry["photo"] = bool(ob.get("photo"))
    return Vm, Tm, table


def chain(o64, s, max_depth, seed, sample=0, pixels=None):
    """The camera chain of sample `sample` of every pixel (or of `pixels`) of scene `s` -> `path_through_fp64.chain`'s record with
    "thr" [N,3] a colour, and "glass", "flagged" [N]: the chain passed a dielectric vertex, a flagged one."""
    H, W, n_scene = s["H"], s["W"], s["n_scene"]
    P = s["V"][s["T"]]
    o, d = pd.camera_rays(H, W, seed, sample, pixels)
    N = o.shape[0]
    pix = np.arange(H * W, dtype=np.uint32) if pixels is None else np.asarray(pixels, dtype=np.uint32)
    base = pf.pcg(pf.pcg(pf.pcg(np.uint32(seed)) + pix) + np.uint32(sample))
    nt = P.shape[0]
    ng_all = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    ng_all *= np.where(((ng_all * P[:, 0]).sum(-1, keepdims=True) > 0) & (np.arange(nt) < n_scene)[:, None], -1.0, 1.0)
    ng_all /= np.linalg.norm(ng_all, axis=-1, keepdims=True)
    kind_of = np.full(nt, "", dtype=object)
    keeps = np.zeros(nt, bool)
    par, mat = np.zeros((nt, 3)), np.zeros((nt, 5))
    smooth_of, corner = np.zeros(nt, bool), np.zeros((nt, 3, 3))
    for ob in s["table"]:
        sl = slice(ob["first_tri"], ob["first_tri"] + ob["n_tri"])
        b = ob["bsdf"]
        kind_of[sl] = b["type"]
        keeps[sl] = b["type"] == "dielectric" or bool(ob.get("photo"))
        assert not (ob.get("photo") and b["type"] in ("dielectric", "area")), "the flag belongs to a diffuse, pbr or roughdielectric object"
        assert not (ob.get("photo") and (ob.get("corner_colors") is not None or ob.get("corner_uv") is not None)), "not stated here"
        if b["type"] == "dielectric":
            par[sl] = [b["int_ior"], b["ext_ior"], 0.0]
        elif b["type"] == "roughdielectric":
            par[sl] = rough_params(b)
        elif b["type"] == "pbr":
            ca, cr, cm = pp.pbr_constants(b)
            mat[sl] = [*ca, cr, cm]
        elif b["type"] == "diffuse":
            par[sl] = np.broadcast_to(np.asarray(b["reflectance"], np.float64), (3,))
        if ob.get("corner_normals") is not None:
            smooth_of[sl], corner[sl] = True, np.asarray(ob["corner_normals"], np.float64)
    out = {"k": np.full(N, -1), "p": np.zeros((N, 3)), "thr": np.ones((N, 3)), "q": np.full(N, -1), "o": np.zeros((N, 3)), "d": np.zeros((N, 3)),
           "covered": np.zeros(N, bool), "back": np.zeros(N, bool), "cut": np.zeros(N, bool), "glass": np.zeros(N, bool),
           "flagged": np.zeros(N, bool)}
    thr = np.ones((N, 3))
    glass, flagged = np.zeros(N, bool), np.zeros(N, bool)
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
            out["glass"][ids], out["flagged"][ids] = glass[ids], flagged[ids]
            if ids.size:
                out["q"][ids] = pf.texel(o64, p[front], H, W)
        go = keeps[k]                                              # every other vertex ends the chain
        if depth + 1 >= max_depth:
            out["cut"][idx[go]] = True
            break
        kind = kind_of[k]
        go &= ((ng * wo).sum(-1) > 0) | (kind == "dielectric") | (kind == "roughdielectric")   # a one-sided object seen from behind
        idx, k, p, wo, ng, kind = idx[go], k[go], p[go], wo[go], ng[go], kind[go]
        if idx.size == 0:
            break
        ns = ng.copy()
        sm = smooth_of[k]
        if sm.any():
            bu, bv = ps.barycentrics(P[k[sm]], o[idx[sm]], d[idx[sm]])
            ns[sm] = ps.shading_normal(corner[k[sm]], bu, bv, ng[sm], wo[sm])[0]
        eps = 1e-5 * (1 + np.abs(p).max(-1))
        u6, u7, u8 = (pf.rng_u(base[idx], depth, c) for c in (6, 7, 8))
        wi, wgt = np.zeros((idx.size, 3)), np.zeros((idx.size, 3))
        side = np.ones(idx.size)
        sel = kind == "dielectric"
        if sel.any():
            w_, g_, _, _, _ = ps.sample_dielectric_shading(par[k[sel], 0], par[k[sel], 1], ng[sel], ns[sel], wo[sel], u6[sel])
            wi[sel], wgt[sel] = w_, g_[:, None]
            side[sel] = np.where((ng[sel] * w_).sum(-1) > 0, 1.0, -1.0)
            glass[idx[sel]] = True
        sel = kind == "pbr"
        if sel.any():                                              # the next ray starts at p + eps ng; a sample below the face ends the path
            cm = mat[k[sel]]
            w_, _, g_ = o64.sample_brdf(u6[sel], np.stack([u7[sel], u8[sel]], -1), wo[sel], ns[sel], cm[:, :3], cm[:, 3], cm[:, 4])
            wi[sel], wgt[sel] = w_, np.where(((ng[sel] * w_).sum(-1) > 0)[:, None], g_, 0.0)
        sel = kind == "diffuse"
        if sel.any():
            w_, _ = po.sample_diffuse(ns[sel], u7[sel], u8[sel])
            wi[sel], wgt[sel] = w_, np.where(((ng[sel] * w_).sum(-1) > 0)[:, None], par[k[sel]], 0.0)
        sel = kind == "roughdielectric"
        if sel.any():
            for pr in np.unique(par[k[sel]], axis=0):
                s2 = sel & (par[k] == pr).all(-1)
                sp = rough_sample(pr, ng[s2], ns[s2], wo[s2], np.stack([u6[s2], u7[s2], u8[s2]], -1))
                wi[s2], wgt[s2] = sp["wi"], sp["weight"][:, None]
                side[s2] = np.where((ng[s2] * sp["wi"]).sum(-1) > 0, 1.0, -1.0)
        flagged[idx[kind != "dielectric"]] = True
        thr[idx] *= wgt
        o[idx], d[idx] = p + (side * eps)[:, None] * ng, wi
        alive[idx] = (thr[idx] > 0).any(-1)
    return out


def chains(o64, s, max_depth, seed, sample=0):
    key = ("reflect chain", max_depth, seed, sample)
    if key not in s:
        s[key] = chain(o64, s, max_depth, seed, sample)
    return s[key]


def _walk(o64, s, tab, table, max_depth, lanes, closest=None):
    return pob.replay_objects(o64, s["V"], s["T"], s["a"], s["r"], s["m"], s["env"], tab, s["H"], s["W"], max_depth, 0, table, closest=closest,
                              lanes=lanes)[0]


def reference(o64, s, tab, photo, max_depth, seed, sample=0):
    """One sample of every pixel -> {"chain": `chain`'s record, "see" [H,W] bool, "with": L_with, "lchain": L_chain and "tail": the tail
    without the objects (both 0 off the see-through lanes), "touched" [H,W]: some traversal of the walk with the objects after the landing
    ray returns an inserted triangle, "fg", "through", "delta", "alpha": the outputs, "scale": `path_diff_fp64.reference`'s}.  Computed
    once per (max_depth, seed, sample) of a scene and kept in it; delta, alpha and the scale are `path_diff_fp64.reference`'s."""
    key = ("reflect", max_depth, seed, sample)
    if key not in s:
        H, W, n_scene = s["H"], s["W"], s["n_scene"]
        base = pd.reference(o64, s, tab, max_depth, seed, sample)
        ch = chains(o64, s, max_depth, seed, sample)
        see = ch["k"] >= 0
        P = s["V"][s["T"]]
        P_scene = P[:n_scene]
        lchain, tail, touched = np.zeros((H * W, 3)), np.zeros((H * W, 3)), np.zeros(H * W, bool)
        table = tf.tail_table(s["table"])
        for k in np.unique(ch["k"][see]):                          # the two cut walks, every lane of one landing depth at once
            ln = np.nonzero(ch["k"] == k)[0]
            lanes = (ln, np.full(ln.size, seed), np.full(ln.size, sample))
            lchain[ln] = _walk(o64, s, tab, s["table"], int(k) + 1, lanes)
            tail[ln] = -_walk(o64, s, tab, table, int(k) + 1, lanes)
        for lane in np.nonzero(see)[0]:
            for objects_after, tb in ((False, table), (True, s["table"])):
                if objects_after and max_depth <= ch["k"][lane] + 1:
                    continue
                landed = [False]

                def closest(o, d):
                    if landed[0]:
                        if objects_after:
                            t, k = pf.brute(P, o, d)
                            touched[lane] |= bool((k >= n_scene).any())
                            return t, k
                        return pf.brute(P_scene, o, d)
                    landed[0] = o.shape[0] == 1 and np.allclose(o[0], ch["o"][lane], rtol=0, atol=1e-9) and np.allclose(d[0], ch["d"][lane], rtol=0, atol=1e-9)
                    return pf.brute(P, o, d)

                L = _walk(o64, s, tab, tb, max_depth, ([lane], [seed], [sample]), closest)
                if not objects_after:
                    assert landed[0], lane
                    tail[lane] += L[0]
        if any(ob["bsdf"]["type"] == "area" for ob in s["table"]):   # a light changes n_e, and through it every emitter sample
            touched |= see
        tail, lchain = tail.reshape(H, W, 3), lchain.reshape(H, W, 3)
        see = see.reshape(H, W)
        c = base["c"]
        through = np.where(see[..., None], ch["thr"].reshape(H, W, 3) * photo.astype(np.float64).reshape(-1, 3)[np.maximum(ch["q"], 0)].reshape(H, W, 3), 0.0)
        s[key] = {"chain": ch, "see": see, "with": base["with"], "lchain": lchain, "tail": tail, "touched": touched.reshape(H, W) & see,
                  "fg": np.where(c[..., None], base["with"] - tail, 0.0), "through": through, "delta": base["delta"], "alpha": base["alpha"],
                  "scale": base["scale"]}
    return s[key]


def preconditions(s, o64, tab, seeds=(0, 1, 2)):
    """The reference's own preconditions on scene R, asserted first in each test: at sample 0 of `seeds` with max_depth 6 a see-through
    share of at least 0.2, at least 20 landings at depth >= 2, at least 20 chains holding both a dielectric and a flagged vertex, at
    least 20 landings with a touched tail and at least 20 with an untouched one."""
    for seed in seeds:
        ref = reference(o64, s, tab, s["photo"], 6, seed)
        ch = ref["chain"]
        see = ch["k"] >= 0
        assert see.mean() >= 0.2, (seed, see.mean())
        assert (ch["k"] >= 2).sum() >= 20, (seed, int((ch["k"] >= 2).sum()))
        assert (see & ch["glass"] & ch["flagged"]).sum() >= 20, (seed, int((see & ch["glass"] & ch["flagged"]).sum()))
        assert ref["touched"].sum() >= 20 and (ref["see"] & ~ref["touched"]).sum() >= 20, (seed, int(ref["touched"].sum()), int((ref["see"] & ~ref["touched"]).sum()))
