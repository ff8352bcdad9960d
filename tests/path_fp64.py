"""fp64 restatement of the path render with every sampling decision recorded, and the derivative of the
fixed-seed estimator with the sampling detached, for the gradient tests (tests/test_path_grad_host.py, tests/test_gpu_path_grad.py).

`replay` walks one sample of each pixel (all of them, or a list) as the integrator does (the oracle's sample_brdf / eval_brdf /
world_to_screen, a brute-force intersection, the restated RNG, the fp32 envmap tables the kernel reads) and records, per path vertex,
what the backward pass holds constant: directions, the texel each vertex reads, the emitter samples and their MIS weights over pdf,
the BSDF samples' 1/(pdf + 1e-6), the escaped rays' texels and MIS weights.  `held_radiance` re-evaluates the radiance of those
recorded paths for any maps and envmap (the estimator as a function of the parameters, sampling held); `held_grad` is its exact
derivative, formed as the kernel forms it (emitter terms through f_e; the BSDF-sample factor through f_s with the radiance after the
vertex) but without cancellation.  Both take a list of records too (samples 0..S-1: the spp-S estimator is their mean).

No BVH and no library code: the default intersection is a numpy brute force over every triangle; `TorchBrute` is the same in
float64 torch, chunked over rays, for meshes of real size (on the GPU when a test has one)."""
import math

import numpy as np

FOV = 35.0


def pcg(v):
    v = np.atleast_1d(np.asarray(v, dtype=np.uint32))
    s = v * np.uint32(747796405) + np.uint32(2891336453)
    w = ((s >> ((s >> np.uint32(28)) + np.uint32(4))) ^ s) * np.uint32(277803737)
    return (w >> np.uint32(22)) ^ w


def rng_u(base, vertex, dim):
    return (pcg(base + np.uint32(vertex * 16 + dim)) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def brute(P, o, d):
    """closest hit of rays o[N,3] + t d[N,3] (t > 0) on triangles P[T,3,3] -> t (inf = miss), index (-1)."""
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    pv = np.cross(d[:, None], e2[None])
    det = (e1[None] * pv).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        tv = o[:, None] - P[None, :, 0]
        u = (tv * pv).sum(-1) / det
        qv = np.cross(tv, e1[None])
        v = (d[:, None] * qv).sum(-1) / det
        t = (e2[None] * qv).sum(-1) / det
    t = np.where((det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0), t, np.inf)
    k = t.argmin(1)
    tk = t[np.arange(k.shape[0]), k]
    return tk, np.where(np.isfinite(tk), k, -1)


class TorchBrute:
    """`brute` in float64 torch over every triangle P[T,3,3] (no BVH), chunked over rays to about `budget` ray-triangle pairs.
    `closest(o, d)` -> (t, index) as `brute`; `occluded(o, d)` -> any hit; `hits(o, d)` adds the hit's smallest barycentric margin."""

    def __init__(self, P, device="cpu", budget=1 << 23):
        import torch

        self.torch, self.device = torch, torch.device(device)
        P = torch.as_tensor(np.ascontiguousarray(P, dtype=np.float64), device=self.device)
        self.v0, self.e1, self.e2 = P[:, 0], P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        self.chunk = max(1, budget // max(1, P.shape[0]))

    def hits(self, o, d):
        torch = self.torch
        o = torch.as_tensor(np.ascontiguousarray(o, dtype=np.float64), device=self.device)
        d = torch.as_tensor(np.ascontiguousarray(d, dtype=np.float64), device=self.device)
        ts, ks, ms = [], [], []
        for c0 in range(0, o.shape[0], self.chunk):
            oo, dd = o[c0:c0 + self.chunk, None, :], d[c0:c0 + self.chunk, None, :]
            pv = torch.linalg.cross(dd.expand(-1, self.e2.shape[0], -1), self.e2[None].expand(dd.shape[0], -1, -1))
            det = (self.e1[None] * pv).sum(-1)
            tv = oo - self.v0[None]
            u = (tv * pv).sum(-1) / det
            qv = torch.linalg.cross(tv, self.e1[None].expand(dd.shape[0], -1, -1))
            v = (dd * qv).sum(-1) / det
            t = (self.e2[None] * qv).sum(-1) / det
            t = torch.where((det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t > 0), t, torch.full_like(t, math.inf))
            tk, k = t.min(1)
            rows = torch.arange(k.shape[0], device=self.device)
            ts.append(tk)
            ks.append(torch.where(torch.isfinite(tk), k, torch.full_like(k, -1)))
            ms.append(torch.minimum(torch.minimum(u, v), 1 - u - v)[rows, k])
        if not ts:
            return np.zeros(0), np.zeros(0, np.int64), np.zeros(0)
        return tuple(torch.cat(x).cpu().numpy() for x in (ts, ks, ms))

    def closest(self, o, d):
        t, k, _ = self.hits(o, d)
        return t, k

    def occluded(self, o, d):
        return np.isfinite(self.hits(o, d)[0])


def texel(o64, p, H, W):
    """The texel a hit point p[N,3] reads: the inverse of the render's camera, whose focal length (W/2)/tan(fov_x/2) holds on both
    axes.  That is a6 world_to_screen given the camera's vertical field of view (fov_x itself when H = W), floor, clamp."""
    fov_y = 2.0 * math.atan(math.tan(math.radians(FOV) / 2.0) * H / W)
    tp = np.empty(p.shape[0], np.int64)
    for q in range(p.shape[0]):
        s = o64.world_to_screen(p[q], fov_y, W / H, 0.01, 10000.0, W, H)
        tp[q] = int(np.clip(np.floor(s[1]), 0, H - 1)) * W + int(np.clip(np.floor(s[0]), 0, W - 1))
    return tp


def env_texel(d, He, We):
    th = np.arccos(np.clip(d[:, 1], -1, 1))
    ph = np.mod(np.arctan2(d[:, 0], -d[:, 2]), 2 * np.pi)
    return np.minimum((th * He / np.pi).astype(np.int64), He - 1) * We + np.minimum((ph * We / (2 * np.pi)).astype(np.int64), We - 1)


def mis(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        w = a * a / (a * a + b * b)
    return np.where(np.isfinite(w), w, 0.0)


def groove_scene(H=24, W=24):
    """A V-groove (walls facing each other: occlusion and inter-reflection) with a step across its lower rows."""
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = 2.0 + 0.07 * (W / 2 - np.abs(j - (W - 1) / 2))
    d[2 * H // 3:] -= 0.35
    return d.astype(np.float32)


def groove_maps(H, W, rng):
    a = rng.uniform(0.2, 0.9, (H, W, 3)).astype(np.float32)
    r = rng.uniform(0.25, 0.9, (H, W, 1)).astype(np.float32)
    m = rng.uniform(0.0, 1.0, (H, W, 1)).astype(np.float32)
    return a, r, m


def groove_env(rng, He=8, We=16):
    env = rng.gamma(2.0, 0.4, (He, We, 3)).astype(np.float32)
    env[1, 3] = [30.0, 28.0, 25.0]     # a sun: emitter sampling matters
    return env


def replay(o64, V, T, a, r, m, env, tab, H, W, max_depth, seed, pixels=None, sample=0, closest=None, occluded=None):
    """Sample `sample` of every pixel, or of the flat pixel indices `pixels` (rows in that order), fp64 -> (L, record); L is [H,W,3]
    for every pixel, [len(pixels),3] for a list.  V: the mesh's vertices rounded to fp32 as the BVH stores them.  `closest(o, d)` ->
    (t, index) and `occluded(o, d)` -> bool: the intersection routines (default: `brute` over every triangle)."""
    He, We = env.shape[:2]
    envf = env.reshape(-1, 3).astype(np.float64)
    pdf_tab = tab["pdf"].reshape(-1).astype(np.float64)
    row_cdf, col_cdf = tab["row_cdf"], tab["col_cdf"]
    have_tab = tab["row_cdf"][-1] > 0
    P = V[T]
    if closest is None:
        closest = lambda o, d: brute(P, o, d)
    if occluded is None:
        occluded = lambda o, d: np.isfinite(brute(P, o, d)[0])
    nrm = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    nrm *= np.where((nrm * P[:, 0]).sum(-1, keepdims=True) > 0, -1.0, 1.0)
    nrm /= np.maximum(np.linalg.norm(nrm, axis=-1, keepdims=True), 1e-300)
    pix = np.arange(H * W, dtype=np.uint32) if pixels is None else np.asarray(pixels, dtype=np.int64).astype(np.uint32)
    N = pix.size
    base = pcg(pcg(pcg(np.uint32(seed)) + pix) + np.uint32(sample))
    ii, jj = pix // W, pix % W
    f = (W / 2.0) / math.tan(math.radians(FOV) / 2.0)
    x = jj - 0.5 + rng_u(base, 0, 0)
    y = ii - 0.5 + rng_u(base, 0, 1)
    d = np.stack([(x - (W - 1) / 2) / f, -(y - (H - 1) / 2) / f, -np.ones(N)], -1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.zeros((N, 3))
    L, thr, prev = np.zeros((N, 3)), np.ones((N, 3)), np.zeros(N)
    alive = np.ones(N, bool)
    A, R, M = a.reshape(-1, 3).astype(np.float64), r.reshape(-1).astype(np.float64), m.reshape(-1).astype(np.float64)
    # "pix" of a vertex / escape: its row (= its pixel when every pixel is replayed); rec["pixels"]: the pixel of each row
    rec = {"H": H, "W": W, "He": He, "We": We, "pixels": pix.astype(np.int64), "full": pixels is None, "escapes": [], "vertices": []}
    for depth in range(max_depth + 1):
        idx = np.nonzero(alive)[0]
        if idx.size == 0:
            break
        t, k = closest(o[idx], d[idx])
        miss = k < 0
        im = idx[miss]
        if im.size:
            tx = env_texel(d[im], He, We)
            w = np.ones(im.size) if depth == 0 else mis(prev[im], pdf_tab[tx] if have_tab else 0.0)
            L[im] += thr[im] * envf[tx] * w[:, None]
            rec["escapes"].append({"depth": depth, "pix": im, "tx": tx, "w": w})
        alive[im] = False
        if depth + 1 >= max_depth:
            alive[:] = False
            break
        idx, t, k = idx[~miss], t[~miss], k[~miss]
        n = nrm[k]
        wo = -d[idx]
        front = (n * wo).sum(-1) > 0
        alive[idx[~front]] = False
        idx, t, k, n, wo = idx[front], t[front], k[front], n[front], wo[front]
        if idx.size == 0:
            continue
        p = o[idx] + t[:, None] * d[idx]
        tp = texel(o64, p, H, W)
        av, rv, mv = A[tp], R[tp], M[tp]
        po = p + (1e-5 * (1 + np.abs(p).max(-1)))[:, None] * n
        b = base[idx]
        vert = {"depth": depth, "pix": idx, "tp": tp, "wo": wo, "n": n, "em": np.zeros(idx.size, bool), "wl": np.zeros((idx.size, 3)),
                "te": np.zeros(idx.size, np.int64), "we": np.zeros(idx.size)}
        if have_tab:
            u0, u1, u2, u3 = (rng_u(b, depth, c) for c in (2, 3, 4, 5))
            row = np.searchsorted(row_cdf[:He], u0, side="right") - 1
            col = np.array([np.searchsorted(col_cdf[rr, :We], uu, side="right") - 1 for rr, uu in zip(row, u1)])
            c0, c1 = np.cos(row * np.pi / He), np.cos((row + 1) * np.pi / He)
            ct = c0 + (c1 - c0) * u2
            st = np.sqrt(np.maximum(1 - ct * ct, 0))
            ph = (col + u3) * 2 * np.pi / We
            wl = np.stack([st * np.sin(ph), ct, -st * np.cos(ph)], -1)
            te = row * We + col
            pe = pdf_tab[te]
            fb, pb = o64.eval_brdf(wl, wo, n, av, rv, mv)
            ok = (pe > 0) & ((n * wl).sum(-1) > 0) & (fb > 0).any(-1)
            if ok.any():
                vis = np.zeros(idx.size, bool)
                vis[np.nonzero(ok)[0]] = ~occluded(po[ok], wl[ok])
                w = np.where(vis, mis(pe, pb) / np.where(pe > 0, pe, 1.0), 0.0)
                L[idx] += thr[idx] * fb * envf[te] * w[:, None]
                vert.update(em=vis, wl=wl, te=te, we=w)
        s1, s2a, s2b = (rng_u(b, depth, c) for c in (6, 7, 8))
        wi, pdf, wgt = o64.sample_brdf(s1, np.stack([s2a, s2b], -1), wo, n, av, rv, mv)
        vert["wi"] = wi
        vert["ip"] = np.where(pdf > 1e-6, 1.0 / (pdf + 1e-6), 0.0)
        rec["vertices"].append(vert)
        thr[idx] *= wgt
        dead = ~(thr[idx] > 0).any(-1)
        alive[idx[dead]] = False
        prev[idx] = pdf
        o[idx], d[idx] = po, wi
    return (L.reshape(H, W, 3) if pixels is None else L), rec


def replay_spp(o64, V, T, a, r, m, env, tab, H, W, max_depth, seed, spp, **kw):
    """The spp-`spp` estimator: the mean of the replays of samples 0..spp-1 -> (L, [record per sample])."""
    Ls, recs = zip(*(replay(o64, V, T, a, r, m, env, tab, H, W, max_depth, seed, sample=s, **kw) for s in range(spp)))
    return sum(Ls) / spp, list(recs)


def _terms(o64, rec, a, r, m, env):
    """Per depth of the recorded paths: throughput arriving at each vertex, emitter terms, BSDF values; escape terms."""
    N = rec["pixels"].size
    A, R, M = a.reshape(-1, 3).astype(np.float64), r.reshape(-1).astype(np.float64), m.reshape(-1).astype(np.float64)
    E = env.reshape(-1, 3).astype(np.float64)
    thr = np.ones((N, 3))
    escapes = {}
    for es in rec["escapes"]:
        escapes[es["depth"]] = es
    out = []
    for dep in range(len(rec["vertices"]) + 1):
        row = {"S": np.zeros((N, 3)), "E": np.zeros((N, 3))}
        if dep in escapes:
            es = escapes[dep]
            row["S"][es["pix"]] = thr[es["pix"]] * E[es["tx"]] * es["w"][:, None]
            row["esc"], row["esc_thr"] = es, thr[es["pix"]].copy()
        if dep < len(rec["vertices"]):
            v = rec["vertices"][dep]
            pix, tp = v["pix"], v["tp"]
            row["v"] = v
            row["thr"] = thr[pix].copy()
            fe, _ = o64.eval_brdf(v["wl"], v["wo"], v["n"], A[tp], R[tp], M[tp])
            fe = np.where(v["em"][:, None], fe, 0.0)
            row["fe"] = fe
            row["E"][pix] = thr[pix] * fe * E[v["te"]] * v["we"][:, None]
            fs, _ = o64.eval_brdf(v["wi"], v["wo"], v["n"], A[tp], R[tp], M[tp])
            row["fs"] = fs
            nthr = np.zeros((N, 3))
            nthr[pix] = thr[pix] * fs * v["ip"][:, None]
            thr = nthr
        out.append(row)
    return out


def held_radiance(o64, rec, a, r, m, env):
    """The radiance of the recorded paths under the maps a, r, m and the envmap env (sampling held), shaped as `replay`'s L; for a
    list of records (one per sample), their mean."""
    if isinstance(rec, (list, tuple)):
        return sum(held_radiance(o64, x, a, r, m, env) for x in rec) / len(rec)
    rows = _terms(o64, rec, a, r, m, env)
    L = sum(row["S"] + row["E"] for row in rows)
    return L.reshape(rec["H"], rec["W"], 3) if rec["full"] else L


def held_grad(o64, rec, a, r, m, env, d_out):
    """d (sum d_out . held_radiance) / d (a, r, m, env): dict of arrays shaped like the inputs.  d_out: [H,W,3], the image's (a record
    of some pixels reads their rows of it); for a list of records, the gradient of their mean."""
    if isinstance(rec, (list, tuple)):
        gs = [held_grad(o64, x, a, r, m, env, d_out) for x in rec]
        return {k: sum(g[k] for g in gs) / len(gs) for k in gs[0]}
    H, W = rec["H"], rec["W"]
    g = d_out.reshape(H * W, 3).astype(np.float64)[rec["pixels"]]
    A, R, M = a.reshape(-1, 3).astype(np.float64), r.reshape(-1).astype(np.float64), m.reshape(-1).astype(np.float64)
    E = env.reshape(-1, 3).astype(np.float64)
    rows = _terms(o64, rec, a, r, m, env)
    N = rec["pixels"].size
    d_a, d_r, d_m, d_env = np.zeros((H * W, 3)), np.zeros(H * W), np.zeros(H * W), np.zeros(E.shape)
    tail = np.zeros((N, 3))                           # radiance after the BSDF sample of the current vertex
    for k in range(len(rows) - 1, -1, -1):
        row = rows[k]
        if "esc" in row:
            es = row["esc"]
            np.add.at(d_env, es["tx"], g[es["pix"]] * row["esc_thr"] * es["w"][:, None])
        if "v" in row:
            v = row["v"]
            pix, tp = v["pix"], v["tp"]
            # BSDF-sample factor: everything after this vertex carries f_s
            with np.errstate(divide="ignore", invalid="ignore"):
                gs = np.where(row["fs"] > 0, g[pix] * tail[pix] / row["fs"], 0.0)
            gs = np.where(v["ip"][:, None] > 0, gs, 0.0)
            ga, gr, gm, _ = o64.eval_brdf_grad(v["wi"], v["wo"], v["n"], A[tp], R[tp], M[tp], gs)
            np.add.at(d_a, tp, ga)
            np.add.at(d_r, tp, gr)
            np.add.at(d_m, tp, gm)
            # emitter term through f_e and Le
            em = v["em"]
            if em.any():
                ge = g[pix] * row["thr"] * E[v["te"]] * v["we"][:, None]
                ga, gr, gm, _ = o64.eval_brdf_grad(v["wl"][em], v["wo"][em], v["n"][em], A[tp[em]], R[tp[em]], M[tp[em]], ge[em])
                np.add.at(d_a, tp[em], ga)
                np.add.at(d_r, tp[em], gr)
                np.add.at(d_m, tp[em], gm)
                np.add.at(d_env, v["te"][em], (g[pix] * row["thr"] * row["fe"] * v["we"][:, None])[em])
            tail = tail + row["E"]
        tail = tail + row["S"]
    return {"a": d_a.reshape(H, W, 3), "r": d_r.reshape(H, W, 1), "m": d_m.reshape(H, W, 1), "env": d_env.reshape(env.shape)}


def contributions(rec):
    """How many terms the backward pass rounds into each element (fixed point): per map texel its vertices
    (one rounding of the vertex's whole material gradient), per envmap texel its escapes and visible emitter samples; summed over a
    list of records.  -> {"maps": [H,W,1], "env": [He,We,1]} (an upper bound: a term that is exactly 0 costs nothing)."""
    if isinstance(rec, (list, tuple)):
        cs = [contributions(x) for x in rec]
        return {k: sum(c[k] for c in cs) for k in cs[0]}
    H, W, He, We = rec["H"], rec["W"], rec["He"], rec["We"]
    maps, env = np.zeros(H * W), np.zeros(He * We)
    for v in rec["vertices"]:
        np.add.at(maps, v["tp"], 1)
        np.add.at(env, v["te"][v["em"]], 1)
    for es in rec["escapes"]:
        np.add.at(env, es["tx"], 1)
    return {"maps": maps.reshape(H, W, 1), "env": env.reshape(He, We, 1)}


def touched(rec):
    """Flat indices of the map texels and of the envmap texels that the recorded paths of each row read: ([set per row], [set per row])."""
    if isinstance(rec, (list, tuple)):
        parts = [touched(x) for x in rec]
        return [set().union(*(p[0][i] for p in parts)) for i in range(len(parts[0][0]))], \
            [set().union(*(p[1][i] for p in parts)) for i in range(len(parts[0][1]))]
    N = rec["pixels"].size
    maps, env = [set() for _ in range(N)], [set() for _ in range(N)]
    for v in rec["vertices"]:
        for q, t in zip(v["pix"], v["tp"]):
            maps[q].add(int(t))
        for q, t in zip(v["pix"][v["em"]], v["te"][v["em"]]):
            env[q].add(int(t))
    for es in rec["escapes"]:
        for q, t in zip(es["pix"], es["tx"]):
            env[q].add(int(t))
    return maps, env
