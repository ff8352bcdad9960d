#!/usr/bin/env python3
"""Time one 512 x 512 frame of tests/golden/indoor2.npz with a 1280-triangle sphere and a diffuse cube in front of the depth mesh
(the frame of tests/test_gpu_path_oi.py::test_indoor2_frame_with_objects and of tools/rough_object_frame.py, spp 32, max_depth 16): the
sphere as a vertex-coloured diffuse object (`path_kernel<ColorObjects>`, a colour per vertex) and the same sphere uniformly diffuse
without the flag (`path_kernel<ObjTable>`, the parent's kernel), in one process, alternating, hip events, the best and the median of
`--repeats` timed frames after a warm-up of each.  Writes profiles/color_object_frame.txt's lines to --out.  Neither sampler depends on
the colour: both frames walk the same paths and trace the same rays; the coloured one reads 36 B more per coloured hit.
Needs a GPU: there is no fallback."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", required=True)
    ap.add_argument("--repeats", type=int, default=7)
    a_ = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("color_object_frame.py needs a GPU")
    import path_oi_fp64 as po
    import path_oi_smooth_fp64 as ps
    from materialist_amd import mesh, pathtrace as pt

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
    z0 = 0.6 * float(depth[depth > 0].min())
    Vs, Ts, _ = ps.icosphere((-0.10 * z0, 0.0, -z0), 0.09 * z0, 3)
    Vc, Tc = po.cube((0.13 * z0, -0.05 * z0, -z0), 0.13 * z0, (0.3, 0.6, 0.2))
    assert Ts.shape[0] == 1280
    cube = {"vertices": Vc, "triangles": Tc, "bsdf": po.DIFFUSE_08}
    colors = np.random.default_rng(5).random(Vs.shape)
    cases = [("sphere vertex-coloured diffuse, reflectance 0.8 x a colour per vertex + diffuse cube (path_kernel<ColorObjects>)",
              [{"vertices": Vs, "triangles": Ts, "bsdf": po.DIFFUSE_08, "colors": colors}, cube]),
             ("sphere uniformly diffuse, reflectance 0.8, no flag + diffuse cube (path_kernel<ObjTable>, the parent's kernel)",
              [{"vertices": Vs, "triangles": Ts, "bsdf": po.DIFFUSE_08}, cube])]
    tracers = [pt.PathTracer(rm["vertices"], rm["triangles"], H, W, 35.0, objects=ob) for _, ob in cases]
    tabs = tracers[0].tables(env)
    kw = dict(spp=32, max_depth=16, seed=1, tables=tabs)
    times, n_rays = [[], []], [0.0, 0.0]
    for tr in tracers:                                                   # warm-up of each
        assert bool(torch.isfinite(tr.render(a, r, m, env, **kw)).all())
    torch.cuda.synchronize()
    for _ in range(a_.repeats):
        for k, tr in enumerate(tracers):                                 # alternating
            rays = torch.zeros(H, W, dtype=torch.int32, device=dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr.render(a, r, m, env, rays=rays, **kw)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
            n_rays[k] = float(rays.to(torch.float64).sum())
    lines = ["512x512 indoor2 frame, spp 32, max_depth 16, a 1280-triangle sphere and a 12-triangle cube in front of the depth mesh; hip events, one process, alternating"]
    for k, (label, _) in enumerate(cases):
        best, med = min(times[k]), float(np.median(times[k]))
        lines.append(f"{label}: {best:.2f} ms (best of {a_.repeats} after a warm-up; median {med:.2f}, worst {max(times[k]):.2f}), "
                     f"{n_rays[k] / 1e6:.2f} Mrays, {n_rays[k] / 1e3 / best:.0f} Mrays/s, n_colored_objects {tracers[k].stats['n_colored_objects']}")
    lines.append(f"coloured / uncoloured: best {min(times[0]) / min(times[1]):.4f}, median {np.median(times[0]) / np.median(times[1]):.4f}; "
                 f"rays {n_rays[0] / n_rays[1]:.6f}")
    os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
    with open(a_.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
