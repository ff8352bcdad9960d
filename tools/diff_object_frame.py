#!/usr/bin/env python3
"""Time the differential render of one 512 x 512 frame of tests/golden/indoor2.npz with a 1280-triangle sphere and a diffuse cube in
front of the depth mesh (the frame of tools/texture_object_frame.py, spp 32, max_depth 16) against the two-render alternative on the
kernels that were there before it: `PathTracer.render_diff` (`path_kernel<DiffObjects>`, one launch sequence, the second walk only
where the first met an object) against `PathTracer.render` with the objects (`path_kernel<ObjTable>`) plus `PathTracer.render` of the
scene alone (`path_kernel<NoObjects>`).  One process, alternating, hip events, the best and the median of `--repeats` timed frames
after a warm-up of each.  Also: the share of samples walked twice, the rays, and (with `--isa`, the gfx950 assembly of matpbr_path.hip
as `hipcc -S --cuda-device-only` with build.py's flags writes it) the registers and the waves per SIMD of the kernels.  Writes
profiles/diff_object_frame.txt's lines to --out.  Needs a GPU: there is no fallback."""
import argparse
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

VGPRS_PER_SIMD, VGPR_GRANULE, MAX_WAVES = 512, 8, 8                      # gfx950: one file for arch and accumulation registers


def kernel_resources(isa_path, names=("DiffObjects", "TexObjects", "ObjTable", "NoObjects")):
    """Per `path_kernel<name>`: (VGPRs, allocated, waves per SIMD, scratch bytes, LDS bytes) from the assembly's .amdhsa_ directives."""
    text = open(isa_path).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, flags=re.S):
        d = dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
        for name in names:
            if f"path_kernelINS_{len(name)}{name}E" in m.group(1):
                v = int(d["next_free_vgpr"])
                alloc = -(-v // VGPR_GRANULE) * VGPR_GRANULE
                out[name] = (v, alloc, min(MAX_WAVES, VGPRS_PER_SIMD // alloc), int(d["private_segment_fixed_size"]), int(d["group_segment_fixed_size"]))
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", required=True)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--isa", default=None, help="the gfx950 assembly of matpbr_path.hip: registers and waves per SIMD are read from it")
    a_ = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("diff_object_frame.py needs a GPU")
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
    objects = [{"vertices": Vs, "triangles": Ts, "bsdf": po.DIFFUSE_08}, {"vertices": Vc, "triangles": Tc, "bsdf": po.DIFFUSE_08}]
    with_objects = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, 35.0, objects=objects)
    alone = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, 35.0)
    tabs = with_objects.tables(env)
    kw = dict(spp=32, max_depth=16, seed=1, tables=tabs)
    runs = [("render_diff (path_kernel<DiffObjects>)", lambda rays: with_objects.render_diff(a, r, m, env, rays=rays, **kw)),
            ("render with the objects (path_kernel<ObjTable>)", lambda rays: with_objects.render(a, r, m, env, rays=rays, **kw)),
            ("render of the scene alone (path_kernel<NoObjects>)", lambda rays: alone.render(a, r, m, env, rays=rays, **kw))]
    fg, delta, alpha, rewalked = runs[0][1](None)                          # warm-up of each
    Lw, L0 = runs[1][1](None), runs[2][1](None)
    assert all(bool(torch.isfinite(x).all()) for x in (fg, delta, alpha, Lw, L0))
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
    lines = ["512x512 indoor2 frame, spp 32, max_depth 16, a 1280-triangle diffuse sphere and a 12-triangle diffuse cube in front of the depth mesh; "
             "hip events, one process, alternating"]
    for k, (label, _) in enumerate(runs):
        best, med = min(times[k]), float(np.median(times[k]))
        lines.append(f"{label}: {best:.2f} ms (best of {a_.repeats} after a warm-up; median {med:.2f}, worst {max(times[k]):.2f}), "
                     f"{n_rays[k] / 1e6:.2f} Mrays, {n_rays[k] / 1e3 / best:.0f} Mrays/s")
    two = [x + y for x, y in zip(times[1], times[2])]
    lines.append(f"render_diff / (the two renders): best {min(times[0]) / min(two):.4f}, median {np.median(times[0]) / np.median(two):.4f}; "
                 f"the two renders together {min(two):.2f}-{max(two):.2f} ms (median {np.median(two):.2f}); rays {n_rays[0] / (n_rays[1] + n_rays[2]):.4f}")
    n_samples = H * W * kw["spp"]
    share = float(rewalked.to(torch.float64).sum()) / n_samples
    lines.append(f"samples walked twice: {share:.4f} of {n_samples}; pixels with a second walk {float((rewalked > 0).double().mean()):.4f}; "
                 f"samples whose camera ray lands on an object {float(alpha.double().mean()):.4f}; pixels that keep the photograph's bits "
                 f"(no second walk, no coverage) {float(((rewalked == 0) & (alpha == 0)).double().mean()):.4f}")
    free = (alpha == 0)[..., None]
    diff = ((delta - (Lw - L0)).abs() * free).max().item()
    lines.append(f"delta against render(with) - render(alone) where alpha = 0: largest absolute difference {diff:.3e} (mean radiance {float(Lw.mean()):.3f})")
    if a_.isa:
        for name, (v, alloc, waves, scratch, lds) in kernel_resources(a_.isa).items():
            lines.append(f"path_kernel<{name}>: {v} VGPRs ({alloc} allocated), {waves} waves per SIMD, scratch {scratch} B, LDS {lds} B per workgroup")
    else:
        lines.append("registers: no --isa given")
    os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
    with open(a_.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
