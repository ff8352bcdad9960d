#!/usr/bin/env python3
"""Time the walk under two environments over one 512 x 512 frame of tests/golden/indoor2.npz (the frame the other *_frame.py tools
time, without objects; spp 32, max_depth 16 and, `render_real`'s default, 4): B is the frame's envmap A rolled by a quarter turn.
`PathTracer.render_relight` (`path_kernel<Relight<NoObjects>>`, one launch sequence, the closest hits, the texels and the BSDF samples
once per vertex, the emitter sample once per envmap) against the two-render alternative on the kernels that were there before it:
`PathTracer.render` under A plus `PathTracer.render` under B (`path_kernel<NoObjects>` twice).  One process, alternating, hip events,
the best and the median of `--repeats` timed frames after a warm-up of each.  Also: the rays (those of the two renders less the
closest hits of one, which a render under an all-zero envmap counts), both radiances against the renders, the quotient composite's
time, and (with `--isa`, the gfx950 assembly of matpbr_path.hip as `hipcc -S --cuda-device-only` with build.py's flags writes it)
the registers and the waves per SIMD of the kernels.  Writes profiles/relight_composite_frame.txt's lines to --out.  Needs a GPU:
there is no fallback."""
import numpy as np
import torch

import object_frame_lib as fl  # puts the repository and tests/ on the path


def main(argv=None):
    a_ = fl.arguments(__doc__, "relight_composite_frame.py", 7, argv, isa=True)
    from materialist_amd import pathtrace as pt

    f = fl.indoor2_frame()
    a, r, m, H, W = f.a, f.r, f.m, f.H, f.W
    env = np.ascontiguousarray(f.env, dtype=np.float32)
    env_b = np.ascontiguousarray(np.roll(env, env.shape[1] // 4, axis=1))
    tracer = fl.tracer(f)
    tabs, tabs_b, tabs_z = tracer.tables(env), tracer.tables(env_b), tracer.tables(np.zeros_like(env))
    lines = [f"512x512 indoor2 frame, spp 32, no objects, B = the {env.shape[0]} x {env.shape[1]} envmap A rolled by {env.shape[1] // 4} columns "
             "(a quarter turn); hip events, one process, alternating; one run on one machine"]
    for max_depth in (16, 4):
        kw = dict(spp=32, max_depth=max_depth, seed=1)
        runs = [("render_relight (path_kernel<Relight<NoObjects>>)",
                 lambda rays: tracer.render_relight(a, r, m, env, env_b, rays=rays, tables=tabs, new_tables=tabs_b, **kw)),
                ("render under A (path_kernel<NoObjects>)", lambda rays: tracer.render(a, r, m, env, rays=rays, tables=tabs, **kw)),
                ("render under B (path_kernel<NoObjects>)", lambda rays: tracer.render(a, r, m, env_b, rays=rays, tables=tabs_b, **kw)),
                ("render under the all-zero envmap (the closest hits alone)",
                 lambda rays: tracer.render(a, r, m, np.zeros_like(env), rays=rays, tables=tabs_z, **kw))]
        ((base, relit), La, Lb, _), times, n_rays = fl.alternate(f, [run for _, run in runs], a_.repeats)
        assert all(bool(torch.isfinite(x).all()) for x in (base, relit, La, Lb))
        lines.append(f"max_depth {max_depth}:")
        for k, (label, _) in enumerate(runs):
            lines.append("  " + fl.time_line(label, times[k], n_rays[k], a_.repeats))
        two = [x + y for x, y in zip(times[1], times[2])]
        lines.append(f"  render_relight / (the two renders): best {min(times[0]) / min(two):.4f}, median {np.median(times[0]) / np.median(two):.4f}; "
                     f"the two renders together {min(two):.2f}-{max(two):.2f} ms (median {np.median(two):.2f}); rays "
                     f"{n_rays[0] / (n_rays[1] + n_rays[2]):.4f} of theirs, {n_rays[0] - (n_rays[1] + n_rays[2] - n_rays[3]):+.0f} off "
                     f"rays(A) + rays(B) - rays(zero)")
        lines.append(f"  base against render(A): largest absolute difference {float((base - La).abs().max()):.3e}, the same bits: "
                     f"{bool(torch.equal(base, La))}; relit against render(B): {float((relit - Lb).abs().max()):.3e}, the same bits: "
                     f"{bool(torch.equal(relit, Lb))} (mean radiance {float(La.mean()):.3f} and {float(Lb.mean()):.3f})")
        photo = La.clone()
        (out,), ctimes, _ = fl.alternate(f, [lambda rays: pt.composite_relight(base, relit, photo, floor=0.01 * float(La.mean()))], a_.repeats,
                                         count_rays=False)
        g = (relit + 0.01 * La.mean()) / (base + 0.01 * La.mean())
        lines.append(f"  composite_relight: {min(ctimes[0]):.3f} ms (best of {a_.repeats}); the ratio g: median {float(g.median()):.3f}, "
                     f"0.01 and 0.99 quantiles {float(g.flatten().quantile(0.01)):.3f} and {float(g.flatten().quantile(0.99)):.3f}")
    lines += fl.resource_lines(a_.isa, ("NoObjects", "ShadeNormals"), "path_kernelINS_7RelightINS_", "path_kernel<Relight<{}>>")
    if a_.isa:
        lines += fl.resource_lines(a_.isa, ("NoObjects", "ShadeNormals"), "path_kernelINS_7MapEditINS_", "path_kernel<MapEdit<{}>>")
        lines += fl.resource_lines(a_.isa, ("NoObjects", "ShadeNormals"))
    fl.write_lines(a_.out, lines)


if __name__ == "__main__":
    main()
