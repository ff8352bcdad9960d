#!/usr/bin/env python3
"""Quality and cost of the differential render's denoiser on the frame of tools/diff_object_frame.py (512 x 512 of
tests/golden/indoor2.npz, a 1280-triangle diffuse sphere and a diffuse cube in front of the depth mesh, max_depth 16).  Quality: the
composite of two spp-16 halves through `PathTracer.denoise_diff` and the plain spp-32 composite, both against an spp-2048 composite into
the same photograph (a converged render of the scene alone), as gamma-2.2 PSNR over the image and over the touched pixels alone, and the
share of pixels that keep the photograph's bits with the filter and without.  Cost: prepare + levels + finish (`denoise_diff`) against
`denoise` (matpbr_path_denoise, the yardstick) on the same geom and alb, one process, alternating, hip events, the best and the median
of `--repeats` after a warm-up; the steps on their own; and (with `--isa`, the gfx950 assembly of matpbr_path.hip) the registers and the
waves per SIMD of the filter's kernels.  Writes profiles/diff_denoise_frame.txt's lines to --out.  Needs a GPU: there is no fallback."""
import numpy as np
import torch

import object_frame_lib as fl  # puts the repository and tests/ on the path

import path_oi_fp64 as po
from materialist_amd import pathtrace as pt
from materialist_amd.relight import albedo_guide

KERNELS = ("denoise_prepare_kernel", "denoise_level_kernel", "denoise_diff_prepare_kernel", "denoise_diff_level_kernel", "denoise_diff_finish_kernel")


def main(argv=None):
    a_ = fl.arguments(__doc__, "diff_denoise_frame.py", 7, argv, isa=True)
    f = fl.indoor2_frame()
    a, r, m, env, H, W = f.a, f.r, f.m, f.env, f.H, f.W
    objects = [fl.sphere(f, po.DIFFUSE_08), f.cube]
    tracer, alone = fl.tracer(f, objects), fl.tracer(f)
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
    _, times, _ = fl.alternate(f, [lambda rays, run=run: run() for _, run in runs], a_.repeats, count_rays=False)
    lines.append(f"cost, hip events, one process, alternating, best of {a_.repeats} after a warm-up (median); the steps on their own include the "
                 "wrapper's allocation of their output")
    for k, (label, _) in enumerate(runs):
        lines.append(f"{label}: {min(times[k]) * 1e3:.1f} us ({float(np.median(times[k])) * 1e3:.1f})")
    lines.append(f"denoise_diff / denoise: best {min(times[0]) / min(times[1]):.3f}, median {np.median(times[0]) / np.median(times[1]):.3f}; per tap "
                 "the new level reads 64 B against 60 B")
    fl.write_lines(a_.out, lines + fl.resource_lines(a_.isa, KERNELS, prefix="", label="{}"))


if __name__ == "__main__":
    main()
