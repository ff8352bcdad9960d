#!/usr/bin/env python3
"""Time one 512 x 512 frame of tests/golden/indoor2.npz with a 1280-triangle sphere and a diffuse cube in front of the depth mesh
(the frame of tests/test_gpu_path_oi.py::test_indoor2_frame_with_objects, spp 32, max_depth 16): the sphere as rough glass
(`path_kernel<RoughObjects>`, alpha 0.1) and the same sphere as clear glass (`path_kernel<ObjTable>`), in one process, alternating,
hip events, the best of `--repeats` timed frames after a warm-up of each.  Writes profiles/rough_object_frame.txt's lines to --out.
Rough glass takes an emitter sample and a shadow ray at every vertex where clear glass takes none: it traces more rays.
Needs a GPU: there is no fallback."""
import object_frame_lib as fl  # puts the repository and tests/ on the path

import path_oi_fp64 as po


def main(argv=None):
    a_ = fl.arguments(__doc__, "rough_object_frame.py", 3, argv, alpha=0.1)
    f = fl.indoor2_frame()
    cases = [("sphere as rough glass, 1.49 / 1.000277, alpha %g + diffuse cube (path_kernel<RoughObjects>)" % a_.alpha,
              [fl.sphere(f, {"type": "roughdielectric", "int_ior": 1.49, "ext_ior": 1.000277, "alpha": a_.alpha}), f.cube]),
             ("sphere as clear glass, 1.49 / 1.000277 + diffuse cube (path_kernel<ObjTable>, the parent's kernel)", [fl.sphere(f, po.GLASS), f.cube])]
    tracers = [fl.tracer(f, ob) for _, ob in cases]
    _, times, n_rays = fl.alternate(f, fl.render_runs(f, tracers), a_.repeats)
    lines = [fl.HEADER]
    for k, (label, _) in enumerate(cases):
        best = min(times[k])
        lines.append(f"{label}: {best:.1f} ms (best of {a_.repeats} after a warm-up), {n_rays[k] / 1e6:.1f} Mrays, {n_rays[k] / 1e3 / best:.0f} Mrays/s, "
                     f"n_rough_objects {tracers[k].stats['n_rough_objects']}")
    fl.write_lines(a_.out, lines)


if __name__ == "__main__":
    main()
