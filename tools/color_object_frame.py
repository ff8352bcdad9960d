#!/usr/bin/env python3
"""Time one 512 x 512 frame of tests/golden/indoor2.npz with a 1280-triangle sphere and a diffuse cube in front of the depth mesh
(the frame of tests/test_gpu_path_oi.py::test_indoor2_frame_with_objects and of tools/rough_object_frame.py, spp 32, max_depth 16): the
sphere as a vertex-coloured diffuse object (`path_kernel<ColorObjects>`, a colour per vertex) and the same sphere uniformly diffuse
without the flag (`path_kernel<ObjTable>`, the parent's kernel), in one process, alternating, hip events, the best and the median of
`--repeats` timed frames after a warm-up of each.  Writes profiles/color_object_frame.txt's lines to --out.  Neither sampler depends on
the colour: both frames walk the same paths and trace the same rays; the coloured one reads 36 B more per coloured hit.
Needs a GPU: there is no fallback."""
import numpy as np
import object_frame_lib as fl  # puts the repository and tests/ on the path

import path_oi_fp64 as po


def main(argv=None):
    a_ = fl.arguments(__doc__, "color_object_frame.py", 7, argv)
    f = fl.indoor2_frame()
    colors = np.random.default_rng(5).random(f.Vs.shape)
    cases = [("sphere vertex-coloured diffuse, reflectance 0.8 x a colour per vertex + diffuse cube (path_kernel<ColorObjects>)",
              [fl.sphere(f, po.DIFFUSE_08, colors=colors), f.cube]),
             ("sphere uniformly diffuse, reflectance 0.8, no flag + diffuse cube (path_kernel<ObjTable>, the parent's kernel)",
              [fl.sphere(f, po.DIFFUSE_08), f.cube])]
    tracers = [fl.tracer(f, ob) for _, ob in cases]
    _, times, n_rays = fl.alternate(f, fl.render_runs(f, tracers), a_.repeats)
    lines = [fl.HEADER]
    for k, (label, _) in enumerate(cases):
        lines.append(fl.time_line(label, times[k], n_rays[k], a_.repeats) + f", n_colored_objects {tracers[k].stats['n_colored_objects']}")
    lines.append(f"coloured / uncoloured: best {min(times[0]) / min(times[1]):.4f}, median {np.median(times[0]) / np.median(times[1]):.4f}; "
                 f"rays {n_rays[0] / n_rays[1]:.6f}")
    fl.write_lines(a_.out, lines)


if __name__ == "__main__":
    main()
