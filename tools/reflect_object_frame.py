#!/usr/bin/env python3
"""Time the differential render with the photograph reflected in inserted objects on one 512 x 512 frame of tests/golden/indoor2.npz
(the frame of tools/diff_object_frame.py, spp 32, max_depth 16) with the 1280-triangle sphere as smooth chrome (pbr, roughness 0.1,
metallic 1) and the diffuse cube beside it, over a fixed synthetic photograph: `PathTracer.render_diff_through` on the table whose
sphere and cube carry "photo" (`path_kernel<Reflect<ThroughObjects>>`) against the same call on the same table without the flag
(`path_kernel<ThroughObjects>`, the baseline) in the same process.  Alternating, hip events, the best and the median of `--repeats`
timed frames after a warm-up of each, and the unflagged twin's own spread.  Also: the rays of each, the share of samples walked twice,
the share of see-through samples, the quality figure of tests/test_gpu_path_reflect.py::test_it_helps_where_the_fit_is_off at frame
size, and (with `--isa`, the gfx950 assembly of matpbr_path.hip as `hipcc -S --cuda-device-only` with build.py's flags writes it) the
registers, waves per SIMD, scratch and LDS of the new kernels.  No ratio is fixed in advance: the flagged render walks more tails
twice.  Writes profiles/reflect_object_frame.txt's lines to --out.  Needs a GPU: there is no fallback."""
import numpy as np
import torch

import object_frame_lib as fl  # puts the repository and tests/ on the path

CHROME = {"type": "pbr", "albedo": (0.95, 0.93, 0.88), "roughness": 0.1, "metallic": 1.0}


def main(argv=None):
    from materialist_amd import pathtrace as pt

    a_ = fl.arguments(__doc__, "reflect_object_frame.py", 7, argv, isa=True)
    f = fl.indoor2_frame()
    a, r, m, env, H, W = f.a, f.r, f.m, f.env, f.H, f.W
    objects = lambda flag: [dict(fl.sphere(f, CHROME, normals=f.Ns), photo=flag), dict(f.cube, photo=flag)]
    on, off = fl.tracer(f, objects(True)), fl.tracer(f, objects(False))
    assert on.stats["n_photo_objects"] == 2 and off.stats["n_photo_objects"] == 0
    photo = f.t(np.random.default_rng(3).gamma(2.0, 0.5, (H, W, 3)))
    tabs = on.tables(env)
    kw = dict(spp=32, max_depth=16, seed=1, tables=tabs)
    runs = [("flagged: render_diff_through (path_kernel<Reflect<ThroughObjects>>)", lambda rays: on.render_diff_through(a, r, m, env, photo, rays=rays, **kw)),
            ("unflagged: render_diff_through (path_kernel<ThroughObjects>)", lambda rays: off.render_diff_through(a, r, m, env, photo, rays=rays, **kw))]
    ((fg, delta, alpha, through, rewalked), (u_fg, u_delta, u_alpha, u_through, u_rewalked)), times, n_rays = fl.alternate(f, [run for _, run in runs], a_.repeats)
    assert all(bool(torch.isfinite(x).all()) for x in (fg, delta, alpha, through, u_fg))
    lines = ["512x512 indoor2 frame, spp 32, max_depth 16, a 1280-triangle smooth chrome sphere (pbr, roughness 0.1, metallic 1) and a 12-triangle "
             "diffuse cube in front of the depth mesh, both flagged against neither, a fixed synthetic photograph; hip events, one process, "
             "alternating; one run on one box"]
    for k, (label, _) in enumerate(runs):
        lines.append(fl.time_line(label, times[k], n_rays[k], a_.repeats))
    lines.append(f"flagged / unflagged: time best {min(times[0]) / min(times[1]):.4f}, median {np.median(times[0]) / np.median(times[1]):.4f}; rays "
                 f"{n_rays[0] / n_rays[1]:.4f}; the unflagged twin's own spread {min(times[1]):.2f} - {max(times[1]):.2f} ms "
                 f"({max(times[1]) / min(times[1]):.4f})")
    n_samples = H * W * kw["spp"]
    n_on, n_off = float(rewalked.to(torch.float64).sum()), float(u_rewalked.to(torch.float64).sum())
    see = [0.0, 0.0]
    for k, tr in enumerate((on, off)):
        for s in range(4):
            one = tr.render_diff_through(a, r, m, env, photo, spp=1, max_depth=16, seed=1000 + s, tables=tabs)
            see[k] += float((one[3] > 0).any(-1).double().mean()) / 4
    lines.append(f"samples walked twice: flagged {n_on / n_samples:.4f} of {n_samples}, unflagged {n_off / n_samples:.4f}; samples whose camera ray lands "
                 f"on an object {float(alpha.double().mean()):.4f}; see-through samples (over 4 one-sample frames) flagged {see[0]:.4f} of all, unflagged "
                 f"{see[1]:.4f}; delta's and alpha's bits equal: {bool(torch.equal(delta, u_delta) and torch.equal(alpha, u_alpha))}")
    # the quality figure: the photograph a render of the scene alone under the maps with metallic 0, "the fit" the albedo halved
    m0 = torch.zeros_like(m)
    alone = fl.tracer(f)
    shot = alone.render(a, r, m0, env, spp=256, max_depth=4, seed=100, tables=tabs)
    truth = on.render(a, r, m0, env, spp=256, max_depth=4, seed=101, tables=tabs)
    ball = on.features()[..., 7] == 1.0                                          # pixels whose centre ray lands on the sphere
    errs = {True: [], False: []}
    for seed in range(8):
        for flag, tr in ((True, on), (False, off)):
            g, d, al, th, _ = tr.render_diff_through(0.5 * a, r, m0, env, shot, spp=32, max_depth=4, seed=seed, tables=tabs)
            errs[flag].append(float((pt.composite(g + th, d, al, shot) - truth).abs()[ball].mean()))
    gain = np.asarray(errs[False]) - np.asarray(errs[True])
    lines.append(f"where the fit is off (the photograph a spp-256 render under metallic 0, the fit's albedo halved, max_depth 4, spp 32, 8 seeds): mean "
                 f"absolute error against the spp-256 render with the objects over the sphere's {int(ball.sum())} pixels, unflagged "
                 f"{np.mean(errs[False]):.5f}, flagged {np.mean(errs[True]):.5f}; the gain is {gain.mean() / (gain.std(ddof=1) / np.sqrt(gain.size)):.1f} "
                 f"standard errors of the difference")
    fl.write_lines(a_.out, lines + fl.resource_lines(a_.isa, ("ThroughObjects", "RatioThroughObjects"), "path_kernelINS_7ReflectINS_",
                                                     "path_kernel<Reflect<{}>>")
                   + (fl.resource_lines(a_.isa, ("ThroughObjects", "RatioThroughObjects"), "path_kernelINS_7ReflectINS_10MediumDiffINS_",
                                        "path_kernel<Reflect<MediumDiff<{}>>>") if a_.isa else [])
                   + (fl.resource_lines(a_.isa, ("ThroughObjects",)) if a_.isa else []))


if __name__ == "__main__":
    main()
