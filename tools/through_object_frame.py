#!/usr/bin/env python3
"""Time the see-through differential render of one 512 x 512 frame of tests/golden/indoor2.npz (the frame of
tools/diff_object_frame.py, spp 32, max_depth 16) with the 1280-triangle sphere as clear smooth glass and the diffuse cube beside it,
over a fixed synthetic photograph: `PathTracer.render_diff_through` (`path_kernel<ThroughObjects>`) against `PathTracer.render_diff`
(`path_kernel<DiffObjects>`, the baseline) on the same table in the same process.  Alternating, hip events, the best and the median of
`--repeats` timed frames after a warm-up of each.  Also: the rays of each, the share of samples with each kind of second walk, the
share of see-through samples whose tail was untouched, and (with `--isa`, the gfx950 assembly of matpbr_path.hip as
`hipcc -S --cuda-device-only` with build.py's flags writes it) the registers, waves per SIMD, scratch and LDS of both kernels.  Writes
profiles/through_object_frame.txt's lines to --out.  Needs a GPU: there is no fallback."""
import numpy as np
import torch

import object_frame_lib as fl  # puts the repository and tests/ on the path

import path_oi_fp64 as po


def main(argv=None):
    a_ = fl.arguments(__doc__, "through_object_frame.py", 7, argv, isa=True)
    f = fl.indoor2_frame()
    a, r, m, env, H, W = f.a, f.r, f.m, f.env, f.H, f.W
    tracer = fl.tracer(f, [fl.sphere(f, po.GLASS, normals=f.Ns), f.cube])
    photo = f.t(np.random.default_rng(3).gamma(2.0, 0.5, (H, W, 3)))
    tabs = tracer.tables(env)
    kw = dict(spp=32, max_depth=16, seed=1, tables=tabs)
    runs = [("render_diff_through (path_kernel<ThroughObjects>)", lambda rays: tracer.render_diff_through(a, r, m, env, photo, rays=rays, **kw)),
            ("render_diff (path_kernel<DiffObjects>)", lambda rays: tracer.render_diff(a, r, m, env, rays=rays, **kw))]
    ((fg, delta, alpha, through, rewalked), (d_fg, d_delta, d_alpha, d_rewalked)), times, n_rays = fl.alternate(f, [run for _, run in runs], a_.repeats)
    assert all(bool(torch.isfinite(x).all()) for x in (fg, delta, alpha, through, d_fg))
    lines = ["512x512 indoor2 frame, spp 32, max_depth 16, a 1280-triangle smooth clear-glass sphere and a 12-triangle diffuse cube in front of the "
             "depth mesh, a fixed synthetic photograph; hip events, one process, alternating"]
    for k, (label, _) in enumerate(runs):
        lines.append(fl.time_line(label, times[k], n_rays[k], a_.repeats))
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
    fl.write_lines(a_.out, lines + fl.resource_lines(a_.isa, ("ThroughObjects", "DiffObjects")))


if __name__ == "__main__":
    main()
