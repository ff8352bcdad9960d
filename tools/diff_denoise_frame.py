#!/usr/bin/env python3
"""Quality and cost of the differential render's denoiser on the frame of tools/diff_object_frame.py (512 x 512 of
tests/golden/indoor2.npz, a 1280-triangle diffuse sphere and a diffuse cube in front of the depth mesh, max_depth 16).  Quality: the
composite of two spp-16 halves through `PathTracer.denoise_diff` and the plain spp-32 composite, both against an spp-2048 composite into
the same photograph (a converged render of the scene alone), as gamma-2.2 PSNR over the image and over the touched pixels alone, and the
share of pixels that keep the photograph's bits with the filter and without.  Cost: prepare + levels + finish (`denoise_diff`) against
`denoise` (matpbr_path_denoise, the yardstick) on the same geom and alb, one process, alternating, hip events, the best and the median
of `--repeats` after a warm-up; the steps on their own; and (with `--isa`, the gfx950 assembly of matpbr_path.hip) the registers and the
waves per SIMD of the filter's kernels.  Writes profiles/diff_denoise_frame.txt's lines to --out.  Needs a GPU: there is no fallback."""
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
KERNELS = ("denoise_prepare_kernel", "denoise_level_kernel", "denoise_diff_prepare_kernel", "denoise_diff_level_kernel", "denoise_diff_finish_kernel")


def kernel_resources(isa_path):
    """Per kernel of KERNELS: (VGPRs, allocated, waves per SIMD, scratch bytes, LDS bytes) from the assembly's .amdhsa_ directives."""
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", open(isa_path).read(), flags=re.S):
        d = dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
        for name in KERNELS:
            if f"{len(name)}{name}E" in m.group(1):
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
        raise SystemExit("diff_denoise_frame.py needs a GPU")
    import path_oi_fp64 as po
    import path_oi_smooth_fp64 as ps
    from materialist_amd import mesh, pathtrace as pt
    from materialist_amd.relight import albedo_guide

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
    objects = [{"vertices": Vs, "triangles": Ts, "bsdf": po.DIFFUSE_08}, {"vertices": Vc, "triangles": Tc, "bsdf": po.DIFFUSE_08}]
    tracer = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, 35.0, objects=objects)
    alone = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, 35.0)
    tabs = tracer.tables(env)
    diff = lambda spp, seed: tracer.render_diff(a, r, m, env, spp=spp, max_depth=16, seed=seed, tables=tabs)[:3]
    photo = alone.render(a, r, m, env, spp=512, max_depth=16, seed=7, tables=alone.tables(env))
    ref = pt.composite(*diff(2048, 100), photo).cpu().numpy().astype(np.float64)
    plain = pt.composite(*diff(32, 1), photo)
    A, B = diff(16, 1), diff(16, 2)
    geom = tracer.features()
    guide = albedo_guide(geom, a, [ob["bsdf"] for ob in objects])
    photo_np = photo.cpu().numpy()
    touched = (plain.cpu().numpy().view(np.uint32) != photo_np.view(np.uint32)).any(-1)
    gam = lambda x: np.clip(x, 0, 1) ** (1 / 2.2)
    psnr = lambda x, sel: float(-10 * np.log10(np.mean((gam(x.cpu().numpy().astype(np.float64)) - gam(ref))[sel] ** 2)))
    keeps = lambda x: float((x.cpu().numpy().view(np.uint32) == photo_np.view(np.uint32)).all(-1).mean())
    everywhere = np.ones((H, W), bool)
    lines = ["512x512 indoor2 frame, max_depth 16, a 1280-triangle diffuse sphere and a 12-triangle diffuse cube in front of the depth mesh; the "
             "photograph is a converged render of the scene alone; reference: the spp-2048 composite; gamma-2.2 PSNR",
             f"touched pixels (the plain spp-32 composite differs from the photograph): {touched.mean():.4f}",
             f"plain spp-32 composite: {psnr(plain, everywhere):.2f} dB over the image, {psnr(plain, touched):.2f} dB over the touched pixels; "
             f"keeps the photograph's bits in {keeps(plain):.4f} of the pixels"]
    for levels in (5, 4, 3):
        den = pt.composite(*tracer.denoise_diff(A, B, guide, geom, 1.0, levels=levels), photo)
        assert bool(torch.isfinite(den).all())
        lines.append(f"two spp-16 halves through denoise_diff, L = {levels}: {psnr(den, everywhere):.2f} dB over the image, {psnr(den, touched):.2f} dB "
                     f"over the touched pixels; keeps the photograph's bits in {keeps(den):.4f} of the pixels")
    # cost: the chains alternating, then the steps on their own
    dA, dB = A[1].abs(), B[1].abs()                                     # radiance-like inputs for the yardstick, the same geom and alb

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    cv, cov = pt.denoise_diff_prepare(A, B, geom, 1.0)
    cv0 = pt.denoise_prepare(dA, dB, geom)
    runs = [("denoise_diff (prepare + 5 levels + finish)", lambda: tracer.denoise_diff(A, B, guide, geom, 1.0)),
            ("denoise (matpbr_path_denoise: prepare + 5 levels)", lambda: tracer.denoise(dA, dB, guide, geom)),
            ("denoise_diff_prepare", lambda: pt.denoise_diff_prepare(A, B, geom, 1.0)),
            ("denoise_prepare", lambda: pt.denoise_prepare(dA, dB, geom)),
            ("denoise_diff_finish", lambda: pt.denoise_diff_finish(cv, cov, A, B, geom, 1.0))]
    for l in (0, 2, 4):
        runs.append((f"denoise_diff_level {l}", lambda l=l: pt.denoise_diff_level(cv, cov, geom, guide, l)))
        runs.append((f"denoise_level {l}", lambda l=l: pt.denoise_level(cv0, geom, guide, l)))
    for _, run in runs:
        run()
    torch.cuda.synchronize()
    times = [[] for _ in runs]
    for _ in range(a_.repeats):
        for k, (_, run) in enumerate(runs):
            times[k].append(timed(run)[0])
    lines.append(f"cost, hip events, one process, alternating, best of {a_.repeats} after a warm-up (median); the steps on their own include the "
                 "wrapper's allocation of their output")
    for k, (label, _) in enumerate(runs):
        lines.append(f"{label}: {min(times[k]) * 1e3:.1f} us ({float(np.median(times[k])) * 1e3:.1f})")
    lines.append(f"denoise_diff / denoise: best {min(times[0]) / min(times[1]):.3f}, median {np.median(times[0]) / np.median(times[1]):.3f}; per tap "
                 "the new level reads 64 B against 60 B")
    if a_.isa:
        for name, (v, alloc, waves, scratch, lds) in kernel_resources(a_.isa).items():
            lines.append(f"{name}: {v} VGPRs ({alloc} allocated), {waves} waves per SIMD, scratch {scratch} B, LDS {lds} B per workgroup")
    else:
        lines.append("registers: no --isa given")
    os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
    with open(a_.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
