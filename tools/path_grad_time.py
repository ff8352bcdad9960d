#!/usr/bin/env python3
"""Time the path render's forward and backward passes on the indoor2 fixture: the reference's final maps,
MaterialNet's depth mesh and the 16 x 32 envmap of tests/golden/indoor2.npz, 512 x 512, spp 64, max_depth 4.

    python tools/path_grad_time.py [--spp 64] [--max_depth 4] [--reps 3]

Prints hip-event times of one frame of each pass and the rays each traced (the backward pass replays every path twice).  For kernel
times, run it under `rocprofv3 --kernel-trace --stats -- python tools/path_grad_time.py`."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--max_depth", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    from materialist_amd import mesh, pathtrace

    dev = torch.device("cuda:0")
    z = np.load(os.path.join(ROOT, "tests", "golden", "indoor2.npz"))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    a = t(z["ref_albedo_u8"].astype(np.float32) / 255.0)
    r = t(z["ref_roughness_u8"].astype(np.float32)[..., None] / 255.0).clamp(0.07, 1.0)
    m = t(z["ref_metallic_u8"].astype(np.float32)[..., None] / 255.0)
    env = z["ref_envmap_f32"]
    depth = z["depth_pred_f32"]
    depth = 2 * depth.max() - depth
    H, W = depth.shape
    rm = mesh.reference_mesh(depth, 35.0)
    tracer = pathtrace.PathTracer(rm["vertices"], rm["triangles"], H, W, 35.0)
    tabs = tracer.tables(env)
    d_out = t(np.random.default_rng(0).normal(size=(H, W, 3)))
    kw = dict(spp=args.spp, max_depth=args.max_depth, seed=1, tables=tabs)
    grads = {k: torch.zeros(s, device=dev) for k, s in (("a", (H, W, 3)), ("r", (H, W, 1)), ("m", (H, W, 1)), ("env", env.shape))}
    tracer.render(a, r, m, env, **kw)
    tracer.render_bwd(a, r, m, env, d_out, grads=grads, **kw)
    torch.cuda.synchronize()
    res = {}
    for name in ("forward", "backward"):
        rays = torch.zeros(H, W, dtype=torch.int32, device=dev)
        ms = []
        for rep in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if name == "forward":
                tracer.render(a, r, m, env, rays=rays if rep == 0 else None, **kw)
            else:
                tracer.render_bwd(a, r, m, env, d_out, grads=grads, rays=rays if rep == 0 else None, **kw)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        n = float(rays.to(torch.float64).sum())
        res[name] = (min(ms), n)
        print(f"{name}: {H}x{W} spp {args.spp} max_depth {args.max_depth}: {min(ms):.1f} ms (min of {args.reps}), {n / 1e6:.1f} Mrays, "
              f"{n / 1e3 / min(ms):.0f} Mrays/s")
    print(f"backward / forward: {res['backward'][0] / res['forward'][0]:.2f}x")
    print("grad norms:", {k: float(v.norm()) for k, v in grads.items()})


if __name__ == "__main__":
    main()
