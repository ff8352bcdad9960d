#!/usr/bin/env python3
"""Time the differential render of one 512 x 512 frame of tests/golden/indoor2.npz with a 1280-triangle sphere and a diffuse cube in
front of the depth mesh (the frame of tools/texture_object_frame.py, spp 32, max_depth 16) against the two-render alternative on the
kernels that were there before it: `PathTracer.render_diff` (`path_kernel<DiffObjects>`, one launch sequence, the second walk only
where the first met an object) against `PathTracer.render` with the objects (`path_kernel<ObjTable>`) plus `PathTracer.render` of the
scene alone (`path_kernel<NoObjects>`).  One process, alternating, hip events, the best and the median of `--repeats` timed frames
after a warm-up of each.  Also: the share of samples walked twice, the rays, and (with `--isa`, the gfx950 assembly of matpbr_path.hip
as `hipcc -S --cuda-device-only` with build.py's flags writes it) the registers and the waves per SIMD of the kernels.  Writes
profiles/diff_object_frame.txt's lines to --out.  Needs a GPU: there is no fallback."""
import numpy as np
import torch

import object_frame_lib as fl  # puts the repository and tests/ on the path

import path_oi_fp64 as po


def main(argv=None):
    a_ = fl.arguments(__doc__, "diff_object_frame.py", 7, argv, isa=True)
    f = fl.indoor2_frame()
    a, r, m, env, H, W = f.a, f.r, f.m, f.env, f.H, f.W
    with_objects, alone = fl.tracer(f, [fl.sphere(f, po.DIFFUSE_08), f.cube]), fl.tracer(f)
    kw = dict(spp=32, max_depth=16, seed=1, tables=with_objects.tables(env))
    runs = [("render_diff (path_kernel<DiffObjects>)", lambda rays: with_objects.render_diff(a, r, m, env, rays=rays, **kw)),
            ("render with the objects (path_kernel<ObjTable>)", lambda rays: with_objects.render(a, r, m, env, rays=rays, **kw)),
            ("render of the scene alone (path_kernel<NoObjects>)", lambda rays: alone.render(a, r, m, env, rays=rays, **kw))]
    ((fg, delta, alpha, rewalked), Lw, L0), times, n_rays = fl.alternate(f, [run for _, run in runs], a_.repeats)
    assert all(bool(torch.isfinite(x).all()) for x in (fg, delta, alpha, Lw, L0))
    lines = ["512x512 indoor2 frame, spp 32, max_depth 16, a 1280-triangle diffuse sphere and a 12-triangle diffuse cube in front of the depth mesh; "
             "hip events, one process, alternating"]
    for k, (label, _) in enumerate(runs):
        lines.append(fl.time_line(label, times[k], n_rays[k], a_.repeats))
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
    fl.write_lines(a_.out, lines + fl.resource_lines(a_.isa, ("DiffObjects", "TexObjects", "ObjTable", "NoObjects")))


if __name__ == "__main__":
    main()
