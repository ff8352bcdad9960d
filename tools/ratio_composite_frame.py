#!/usr/bin/env python3
"""Time ratio shadow transfer on one 512 x 512 frame of tests/golden/indoor2.npz (the frame of tools/diff_object_frame.py: the
1280-triangle sphere and the cube diffuse, spp 32, max_depth 16): `PathTracer.render_diff_ratio` (`path_kernel<RatioObjects>`) against
`PathTracer.render_diff` (`path_kernel<DiffObjects>`, the twin without `base`) on the same table in the same process, and
`composite_ratio` against `composite` over the frame's sums.  Alternating, hip events, the best and the median of `--repeats` timed calls
after a warm-up of each, and the twin's own spread to read the ratio against.  Then the quality experiment of
tests/test_path_ratio_host.py at the frame's size: the frame's maps are the truth, the same maps with the albedo halved the fit; the
photograph is `base` and the true picture `base + delta` of the true maps' render, both composites come from the fitted maps' sums of
the same samples, and the PSNR of each against the true picture is taken over the shadow pixels (alpha = 0 and the true delta negative
in every channel), peak = the true picture's largest value there.  With `--isa` (the gfx950 assembly of matpbr_path.hip as
`hipcc -S --cuda-device-only` with build.py's flags writes it) the registers, waves per SIMD, scratch and LDS of the kernels.  Writes
profiles/ratio_composite_frame.txt's lines to --out.  Needs a GPU: there is no fallback."""
import numpy as np
import torch

import object_frame_lib as fl  # puts the repository and tests/ on the path

import path_oi_fp64 as po


def _psnr(got, truth, mask):
    err = (got - truth)[mask].double()
    return float(10.0 * torch.log10(truth[mask].double().max() ** 2 / (err * err).mean()))


def main(argv=None):
    from materialist_amd import pathtrace as pt

    a_ = fl.arguments(__doc__, "ratio_composite_frame.py", 7, argv, isa=True)
    f = fl.indoor2_frame()
    a, r, m, env, H, W = f.a, f.r, f.m, f.env, f.H, f.W
    tracer = fl.tracer(f, [fl.sphere(f, po.DIFFUSE_08), f.cube])
    kw = dict(spp=32, max_depth=16, seed=1, tables=tracer.tables(env))
    runs = [("render_diff_ratio (path_kernel<RatioObjects>)", lambda rays: tracer.render_diff_ratio(a, r, m, env, rays=rays, **kw)),
            ("render_diff (path_kernel<DiffObjects>)", lambda rays: tracer.render_diff(a, r, m, env, rays=rays, **kw))]
    ((fg, delta, base, alpha, rewalked), twin), times, n_rays = fl.alternate(f, [run for _, run in runs], a_.repeats)
    assert all(bool(torch.isfinite(x).all()) for x in (fg, delta, base, alpha))
    same = all(bool(torch.equal(x, y)) for x, y in zip((fg, delta, alpha, rewalked), twin))
    lines = ["512x512 indoor2 frame, spp 32, max_depth 16, a 1280-triangle diffuse sphere and a 12-triangle diffuse cube in front of the depth mesh; "
             "hip events, one process, alternating"]
    for k, (label, _) in enumerate(runs):
        lines.append(fl.time_line(label, times[k], n_rays[k], a_.repeats))
    best, med = min(times[0]) / min(times[1]), float(np.median(times[0]) / np.median(times[1]))
    spread = max(times[1]) / min(times[1])
    lines.append(f"render_diff_ratio / render_diff: time best {best:.4f}, median {med:.4f}; rays {n_rays[0] / n_rays[1]:.4f}; render_diff's own spread "
                 f"(worst / best) {spread:.4f}: the ratio of the bests lies {'inside' if 1.0 / spread <= best <= spread else 'outside'} it; fg, delta, "
                 f"alpha, rewalked bit-identical to render_diff's: {same}")
    free = float((alpha == 0).double().mean())
    lines.append(f"samples whose camera ray lands on an object {float(alpha.double().mean()):.4f}; pixels with alpha = 0 {free:.4f}; samples walked twice "
                 f"{float(rewalked.double().sum()) / (H * W * kw['spp']):.4f}; the extra traffic is 12 B of read-add-write per uncovered sample per pixel")
    # the composites over the frame's sums, a synthetic photograph
    photo = f.t(np.random.default_rng(3).gamma(2.0, 0.5, (H, W, 3)))
    comps = [("composite_ratio (composite_ratio_kernel)", lambda rays: pt.composite_ratio(fg, delta, base, alpha, photo, 1.0)),
             ("composite (composite_kernel)", lambda rays: pt.composite(fg, delta, alpha, photo, 1.0))]
    _, ctimes, _ = fl.alternate(f, [run for _, run in comps], a_.repeats, count_rays=False)
    for k, (label, _) in enumerate(comps):
        lines.append(f"{label}: {min(ctimes[k]) * 1e3:.1f} us (best of {a_.repeats} after a warm-up; median {float(np.median(ctimes[k])) * 1e3:.1f}, worst "
                     f"{max(ctimes[k]) * 1e3:.1f}), host wrapper included")
    dark = ((delta < 0) & (base > 0)).double().mean()
    lines.append(f"composite_ratio / composite: best {min(ctimes[0]) / min(ctimes[1]):.4f}, median {np.median(ctimes[0]) / np.median(ctimes[1]):.4f}; "
                 f"channels on the ratio branch (delta < 0 < base) {float(dark):.4f}")
    # quality: true maps -> the photograph and the true picture; the albedo halved -> both composites
    shadow = (alpha == 0) & (delta < 0).all(-1)
    truth, shot = base + delta, base
    f_fg, f_delta, f_base, f_alpha, _ = tracer.render_diff_ratio(0.5 * a, r, m, env, **kw)
    additive, ratio = pt.composite(f_fg, f_delta, f_alpha, shot, 1.0), pt.composite_ratio(f_fg, f_delta, f_base, f_alpha, shot, 1.0)
    depth = float((shot - truth)[shadow].double().mean())
    lines.append(f"quality, fitted albedo = 0.5 x true, same samples: shadow pixels {int(shadow.sum())} of {H * W} (mean depth {depth:.4e}, mean true "
                 f"radiance {float(truth[shadow].double().mean()):.4f}); PSNR against the true-map picture over them: additive "
                 f"{_psnr(additive, truth, shadow):.2f} dB, ratio {_psnr(ratio, truth, shadow):.2f} dB; mean absolute error: additive "
                 f"{float((additive - truth)[shadow].abs().double().mean()):.4e}, ratio {float((ratio - truth)[shadow].abs().double().mean()):.4e}")
    lines += fl.resource_lines(a_.isa, ("RatioObjects", "RatioThroughObjects", "ThroughObjects", "DiffObjects"))
    if a_.isa:   # not a template: its mangled name is the anonymous namespace's, then the length and the name
        lines += fl.resource_lines(a_.isa, ("composite_ratio_kernel", "composite_kernel"), prefix="_GLOBAL__N_1", label="{}")
    fl.write_lines(a_.out, lines)


if __name__ == "__main__":
    main()
