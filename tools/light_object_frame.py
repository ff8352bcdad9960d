#!/usr/bin/env python3
"""Time one 512 x 512 frame of tests/golden/indoor2.npz with a 1280-triangle sphere and a diffuse cube in front of the depth mesh
(the frame of tests/test_gpu_path_oi.py::test_indoor2_frame_with_objects, spp 32, max_depth 16): the sphere as an area light
(`path_kernel<LightObjects>`) and the same sphere as a diffuse object (`path_kernel<ObjTable>`), in one process, alternating, hip
events, the best of `--repeats` timed frames after a warm-up of each.  Writes profiles/light_object_frame.txt's lines to --out.
Needs a GPU: there is no fallback."""
import object_frame_lib as fl  # puts the repository and tests/ on the path

import path_oi_fp64 as po


def main(argv=None):
    a_ = fl.arguments(__doc__, "light_object_frame.py", 3, argv, radiance=20.0)
    f = fl.indoor2_frame()
    cases = [("sphere as an area light, radiance %g + diffuse cube (path_kernel<LightObjects>)" % a_.radiance,
              [fl.sphere(f, {"type": "area", "radiance": a_.radiance}), f.cube]),
             ("sphere as a diffuse object, reflectance 0.8 + diffuse cube (path_kernel<ObjTable>, the parent's kernel)",
              [fl.sphere(f, po.DIFFUSE_08), f.cube])]
    tracers = [fl.tracer(f, ob) for _, ob in cases]
    _, times, n_rays = fl.alternate(f, fl.render_runs(f, tracers), a_.repeats)
    lines = [fl.HEADER]
    for k, (label, _) in enumerate(cases):
        best = min(times[k])
        lines.append(f"{label}: {best:.1f} ms (best of {a_.repeats} after a warm-up), {n_rays[k] / 1e6:.1f} Mrays, {n_rays[k] / 1e3 / best:.0f} Mrays/s, "
                     f"n_lights {tracers[k].stats['n_lights']}")
    fl.write_lines(a_.out, lines)


if __name__ == "__main__":
    main()
