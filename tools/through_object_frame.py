#!/usr/bin/env python3
"""Time the see-through differential render of one 512 x 512 frame of tests/golden/indoor2.npz (the frame of
tools/diff_object_frame.py, spp 32, max_depth 16) with the 1280-triangle sphere as clear smooth glass and the diffuse cube beside it,
over a fixed synthetic photograph: `PathTracer.render_diff_through` (`path_kernel<ThroughObjects>`) against `PathTracer.render_diff`
(`path_kernel<DiffObjects>`, the baseline) on the same table in the same process.  Alternating, hip events, the best and the median of
`--repeats` timed frames after a warm-up of each.  Also: the rays of each, the share of samples with each kind of second walk, the
share of see-through samples whose tail was untouched, and (with `--isa`, the gfx950 assembly of matpbr_path.hip as
`hipcc -S --cuda-device-only` with build.py's flags writes it) the registers, waves per SIMD, scratch and LDS of both kernels.  Writes
profiles/through_object_frame.txt's lines to --out.  Needs a GPU: there is no fallback."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", required=True)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--isa", default=None, help="the gfx950 assembly of matpbr_path.hip: registers and waves per SIMD are read from it")
    a_ = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("through_object_frame.py needs a GPU")
    import path_oi_fp64 as po
    import path_oi_smooth_fp64 as ps
    from diff_object_frame import kernel_resources
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
    Vs, Ts, Ns = ps.icosphere((-0.10 * z0, 0.0, -z0), 0.09 * z0, 3)
    Vc, Tc = po.cube((0.13 * z0, -0.05 * z0, -z0), 0.13 * z0, (0.3, 0.6, 0.2))
    assert Ts.shape[0] == 1280
    objects = [{"vertices": Vs, "triangles": Ts, "bsdf": po.GLASS, "normals": Ns}, {"vertices": Vc, "triangles": Tc, "bsdf": po.DIFFUSE_08}]
    tracer = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, 35.0, objects=objects)
    photo = t(np.random.default_rng(3).gamma(2.0, 0.5, (H, W, 3)))
    tabs = tracer.tables(env)
    kw = dict(spp=32, max_depth=16, seed=1, tables=tabs)
    runs = [("render_diff_through (path_kernel<ThroughObjects>)", lambda rays: tracer.render_diff_through(a, r, m, env, photo, rays=rays, **kw)),
            ("render_diff (path_kernel<DiffObjects>)", lambda rays: tracer.render_diff(a, r, m, env, rays=rays, **kw))]
    fg, delta, alpha, through, rewalked = runs[0][1](None)                  # warm-up of each
    d_fg, d_delta, d_alpha, d_rewalked = runs[1][1](None)
    assert all(bool(torch.isfinite(x).all()) for x in (fg, delta, alpha, through, d_fg))
    torch.cuda.synchronize()
    times, n_rays = [[] for _ in runs], [0.0] * len(runs)
    for _ in range(a_.repeats):
        for k, (_, run) in enumerate(runs):                                # alternating
            rays = torch.zeros(H, W, dtype=torch.int32, device=dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(rays)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
            n_rays[k] = float(rays.to(torch.float64).sum())
    lines = ["512x512 indoor2 frame, spp 32, max_depth 16, a 1280-triangle smooth clear-glass sphere and a 12-triangle diffuse cube in front of the "
             "depth mesh, a fixed synthetic photograph; hip events, one process, alternating"]
    for k, (label, _) in enumerate(runs):
        best, med = min(times[k]), float(np.median(times[k]))
        lines.append(f"{label}: {best:.2f} ms (best of {a_.repeats} after a warm-up; median {med:.2f}, worst {max(times[k]):.2f}), "
                     f"{n_rays[k] / 1e6:.2f} Mrays, {n_rays[k] / 1e3 / best:.0f} Mrays/s")
    lines.append(f"render_diff_through / render_diff: time best {min(times[0]) / min(times[1]):.4f}, median "
                 f"{np.median(times[0]) / np.median(times[1]):.4f}; rays {n_rays[0] / n_rays[1]:.4f}")
    n_samples = H * W * kw["spp"]
    # delta's second walks are render_diff's own count (the two kernels give the same delta); the rest are the landings' tails
    n_delta, n_all = float(d_rewalked.to(torch.float64).sum()), float(rewalked.to(torch.float64).sum())
    n_tail = n_all - n_delta
    # a see-through sample is one that added to `through`: per pixel only its mean is kept, so the count comes from the one-sample frames
    see = 0.0
    for s in range(4):
        one = tracer.render_diff_through(a, r, m, env, photo, spp=1, max_depth=16, seed=1000 + s, tables=tabs)
        see += float((one[3] > 0).any(-1).double().mean())
    see /= 4
    lines.append(f"second walks: {n_all / n_samples:.4f} of {n_samples} samples; for delta (samples that miss the objects and met one) "
                 f"{n_delta / n_samples:.4f}; tails of see-through samples {n_tail / n_samples:.4f}; delta's bits equal render_diff's: "
                 f"{bool(torch.equal(delta, d_delta) and torch.equal(alpha, d_alpha))}")
    lines.append(f"samples whose camera ray lands on an object {float(alpha.double().mean()):.4f}; see-through samples (over 4 one-sample frames) "
                 f"{see:.4f} of all; see-through samples whose tail was untouched (no second walk, exactly thr photo[q]) "
                 f"{max(0.0, 1.0 - (n_tail / n_samples) / see) if see > 0 else float('nan'):.4f} of them")
    if a_.isa:
        for name, (v, alloc, waves, scratch, lds) in kernel_resources(a_.isa, ("ThroughObjects", "DiffObjects")).items():
            lines.append(f"path_kernel<{name}>: {v} VGPRs ({alloc} allocated), {waves} waves per SIMD, scratch {scratch} B, LDS {lds} B per workgroup")
    else:
        lines.append("registers: no --isa given")
    os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
    with open(a_.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
