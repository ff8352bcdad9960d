#!/usr/bin/env python3
"""Time the differential render of a material edit over one 512 x 512 frame of tests/golden/indoor2.npz (the frame the other *_frame.py
tools time, without objects; spp 32, max_depth 16 and, `render_real`'s default, 4): roughness 0.2 inside a centred disc of radius
0.3 H, the transparency edit's mask.  `PathTracer.render_edit_diff` (`path_kernel<MapEdit<NoObjects>>`, one launch sequence, the
second walk only where the first read a masked texel) against the two-render alternative on the kernels that were there before it:
`PathTracer.render` of the edited maps plus `PathTracer.render` of the fitted ones (`path_kernel<NoObjects>` twice).  One process,
alternating, hip events, the best and the median of `--repeats` timed frames after a warm-up of each.  Also: the rays, the share of
samples walked twice, the share of pixels that keep the photograph's bits, and (with `--isa`, the gfx950 assembly of matpbr_path.hip
as `hipcc -S --cuda-device-only` with build.py's flags writes it) the registers and the waves per SIMD of the kernels.  Writes
profiles/edit_composite_frame.txt's lines to --out.  Needs a GPU: there is no fallback."""
import numpy as np
import torch

import object_frame_lib as fl  # puts the repository and tests/ on the path


def main(argv=None):
    a_ = fl.arguments(__doc__, "edit_composite_frame.py", 7, argv, isa=True)
    f = fl.indoor2_frame()
    a, r, m, env, H, W = f.a, f.r, f.m, f.env, f.H, f.W
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    mask = torch.from_numpy((i - (H - 1) / 2) ** 2 + (j - (W - 1) / 2) ** 2 < (0.3 * H) ** 2).to(f.dev)
    r_e = r.clone()
    r_e[mask] = 0.2
    tracer = fl.tracer(f)
    tabs = tracer.tables(env)
    lines = ["512x512 indoor2 frame, spp 32, no objects, roughness 0.2 inside a centred disc of radius 0.3 H "
             f"({float(mask.double().mean()):.4f} of the texels); hip events, one process, alternating"]
    for max_depth in (16, 4):
        kw = dict(spp=32, max_depth=max_depth, seed=1, tables=tabs)
        runs = [("render_edit_diff (path_kernel<MapEdit<NoObjects>>)", lambda rays: tracer.render_edit_diff(a, r, m, env, (a, r_e, m), mask, rays=rays, **kw)),
                ("render of the edited maps (path_kernel<NoObjects>)", lambda rays: tracer.render(a, r_e, m, env, rays=rays, **kw)),
                ("render of the fitted maps (path_kernel<NoObjects>)", lambda rays: tracer.render(a, r, m, env, rays=rays, **kw))]
        ((delta, base, rewalked), Le, Lf), times, n_rays = fl.alternate(f, [run for _, run in runs], a_.repeats)
        assert all(bool(torch.isfinite(x).all()) for x in (delta, base, Le, Lf))
        lines.append(f"max_depth {max_depth}:")
        for k, (label, _) in enumerate(runs):
            lines.append("  " + fl.time_line(label, times[k], n_rays[k], a_.repeats))
        two = [x + y for x, y in zip(times[1], times[2])]
        n_samples = H * W * kw["spp"]
        share = float(rewalked.to(torch.float64).sum()) / n_samples
        lines.append(f"  render_edit_diff / (the two renders): best {min(times[0]) / min(two):.4f}, median {np.median(times[0]) / np.median(two):.4f}; "
                     f"the two renders together {min(two):.2f}-{max(two):.2f} ms (median {np.median(two):.2f}); rays "
                     f"{n_rays[0] / (n_rays[1] + n_rays[2]):.4f} (expected (1 + share walked twice) / 2 = {(1 + share) / 2:.4f})")
        lines.append(f"  samples walked twice: {share:.4f} of {n_samples}; pixels with a second walk {float((rewalked > 0).double().mean()):.4f}; pixels "
                     f"that keep the photograph's bits (no second walk) {float((rewalked == 0).double().mean()):.4f}")
        lines.append(f"  base + delta against render(edited): largest absolute difference {float((base + delta - Le).abs().max()):.3e}; base against "
                     f"render(fitted): {float((base - Lf).abs().max()):.3e}, the same bits: {bool(torch.equal(base, Lf))} (mean radiance {float(Lf.mean()):.3f})")
    lines += fl.resource_lines(a_.isa, ("NoObjects", "ShadeNormals"), "path_kernelINS_7MapEditINS_", "path_kernel<MapEdit<{}>>")
    if a_.isa:
        lines += fl.resource_lines(a_.isa, ("NoObjects", "ShadeNormals"))
    fl.write_lines(a_.out, lines)


if __name__ == "__main__":
    main()
