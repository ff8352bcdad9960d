#!/usr/bin/env python3
"""Time a medium inside the glass sphere of one 512 x 512 frame of tests/golden/indoor2.npz (the frame of tools/diff_object_frame.py,
spp 32, max_depth 16; the 1280-triangle sphere as clear smooth glass and the diffuse cube beside it).  In one process, alternating:
`PathTracer.render` of the clear sphere (`path_kernel<SmoothObjects>`, the twin) against the same sphere tinted (sigma_a
alone) and cloudy (sigma_s x diameter = 1), both `path_kernel<MediumObjects>`; and `PathTracer.render_diff_through` of the clear
sphere (`path_kernel<ThroughObjects>`) against the tinted one (`path_kernel<MediumDiff<ThroughObjects>>`) over a fixed synthetic
photograph.  Hip events, the best and the median of `--repeats` timed frames after a warm-up of each, the rays of each, and the clear
twin's own spread (worst / best), which is what a tinted object is expected to lie inside: its ray count is the twin's.  With `--isa`
(the gfx950 assembly of matpbr_path.hip as `hipcc -S --cuda-device-only` with build.py's flags writes it) the registers, waves per
SIMD, scratch and LDS of the five kernels with media.  Writes profiles/medium_object_frame.txt's lines to --out.  Needs a GPU: there
is no fallback."""
import numpy as np
import torch

import object_frame_lib as fl  # puts the repository and tests/ on the path

import path_oi_fp64 as po


def main(argv=None):
    a_ = fl.arguments(__doc__, "medium_object_frame.py", 7, argv, isa=True)
    f = fl.indoor2_frame()
    a, r, m, env, H, W = f.a, f.r, f.m, f.env, f.H, f.W
    diameter = 2 * 0.09 * f.z0
    media = {"clear": None, "tinted": {"color": [0.9, 0.45, 0.15], "at": diameter}, "cloudy": {"color": [0.9, 0.45, 0.15], "at": diameter,
                                                                                                "scatter": 1.0 / diameter, "g": 0.5}}
    tracers = {name: fl.tracer(f, [fl.sphere(f, po.GLASS if med is None else dict(po.GLASS, medium=med), normals=f.Ns), f.cube])
               for name, med in media.items()}
    assert [tracers[k].stats["n_medium_objects"] for k in media] == [0, 1, 1]
    photo = f.t(np.random.default_rng(3).gamma(2.0, 0.5, (H, W, 3)))
    tabs = tracers["clear"].tables(env)
    kw = dict(spp=32, max_depth=16, seed=1, tables=tabs)
    renders = fl.render_runs(f, [tracers[k] for k in media])
    through = [lambda rays, tr=tracers[k]: tr.render_diff_through(a, r, m, env, photo, rays=rays, **kw) for k in ("clear", "tinted")]
    labels = [f"render, {k} sphere" for k in media] + [f"render_diff_through, {k} sphere" for k in ("clear", "tinted")]
    warm, times, n_rays = fl.alternate(f, renders + through, a_.repeats)
    assert all(bool(torch.isfinite(x).all()) for x in warm[:3]) and all(bool(torch.isfinite(x).all()) for out in warm[3:] for x in out[:4])
    lines = ["512x512 indoor2 frame, spp 32, max_depth 16, a 1280-triangle smooth clear-glass sphere (clear, tinted: sigma_a alone, cloudy: sigma_s x "
             "diameter = 1, g 0.5) and a 12-triangle diffuse cube in front of the depth mesh, a fixed synthetic photograph; hip events, one process, "
             "alternating"]
    for k, label in enumerate(labels):
        lines.append(fl.time_line(label, times[k], n_rays[k], a_.repeats))
    for what, twin, others in (("render", 0, (1, 2)), ("render_diff_through", 3, (4,))):
        lines.append(f"{what}, the clear twin's own spread: worst / best {max(times[twin]) / min(times[twin]):.4f}, median / best "
                     f"{np.median(times[twin]) / min(times[twin]):.4f}")
        for k in others:
            lines.append(f"{labels[k]} / clear: time best {min(times[k]) / min(times[twin]):.4f}, median "
                         f"{np.median(times[k]) / np.median(times[twin]):.4f}; rays {n_rays[k] / n_rays[twin]:.4f}")
    fl.write_lines(a_.out, lines + fl.resource_lines(a_.isa, ("MediumObjects",)) +
                   (fl.resource_lines(a_.isa, ("DiffObjects", "ThroughObjects", "RatioObjects", "RatioThroughObjects"), prefix="path_kernelINS_10MediumDiffINS_",
                                      label="path_kernel<MediumDiff<{}>>") if a_.isa else []))


if __name__ == "__main__":
    main()
