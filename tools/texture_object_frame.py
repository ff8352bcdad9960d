#!/usr/bin/env python3
"""Time one 512 x 512 frame of tests/golden/indoor2.npz with a 1280-triangle sphere and a diffuse cube in front of the depth mesh
(the frame of tests/test_gpu_path_oi.py::test_indoor2_frame_with_objects and of tools/color_object_frame.py, spp 32, max_depth 16), four
ways: the sphere as a diffuse object textured with a 1024 x 1024 base-colour image (`path_kernel<TexObjects>`) and the same sphere
untextured (`path_kernel<ObjTable>`, the parent's kernel); the sphere as a PBR object with a 1024 x 1024 base-colour and a 1024 x 1024
orm image (`path_kernel<TexObjects>`) and the same sphere untextured (`path_kernel<PbrObjects>`, the parent's kernel).  One process,
alternating, hip events, the best and the median of `--repeats` timed frames after a warm-up of each.  Writes
profiles/texture_object_frame.txt's lines to --out.  A base-colour image changes no path: the first pair traces the same rays, and
the textured frame reads 24 B of coordinates and four 16 B texels more per textured hit.  An orm image changes the roughness and the
metallic, so the second pair's paths differ.
Needs a GPU: there is no fallback."""
import numpy as np

import object_frame_lib as fl  # puts the repository and tests/ on the path

import path_oi_fp64 as po

SIDE = 1024


def images(rng):
    """A base-colour and an orm image [SIDE,SIDE,3] in [0, 1]: smooth waves under per-texel noise, so that neighbouring hits read
    neighbouring texels of different value."""
    y, x = np.meshgrid(np.arange(SIDE) / SIDE, np.arange(SIDE) / SIDE, indexing="ij")
    wave = 0.5 + 0.25 * np.stack([np.sin(14 * np.pi * x), np.sin(10 * np.pi * y), np.sin(6 * np.pi * (x + y))], -1)
    base = np.clip(wave + 0.2 * (rng.random((SIDE, SIDE, 3)) - 0.5), 0.0, 1.0)
    orm = np.clip(wave[..., ::-1] + 0.2 * (rng.random((SIDE, SIDE, 3)) - 0.5), 0.0, 1.0)
    return base.astype(np.float32), orm.astype(np.float32)


def main(argv=None):
    a_ = fl.arguments(__doc__, "texture_object_frame.py", 7, argv)
    f = fl.indoor2_frame()
    n = (f.Vs - f.centre) / np.linalg.norm(f.Vs - f.centre, axis=-1, keepdims=True)
    uv = 2.0 * np.stack([np.arctan2(n[:, 0], n[:, 2]) / (2 * np.pi) + 0.5, np.arccos(np.clip(n[:, 1], -1, 1)) / np.pi], -1)   # the image twice around
    base, orm = images(np.random.default_rng(5))
    pbr = {"type": "pbr", "albedo": (0.8, 0.8, 0.8), "roughness": 0.5, "metallic": 0.5}
    cases = [(f"sphere diffuse, reflectance 0.8 x a {SIDE} x {SIDE} base-colour image + diffuse cube (path_kernel<TexObjects>)",
              [fl.sphere(f, po.DIFFUSE_08, uv=uv, texture=base), f.cube]),
             ("sphere uniformly diffuse, reflectance 0.8, no flag + diffuse cube (path_kernel<ObjTable>, the parent's kernel)",
              [fl.sphere(f, po.DIFFUSE_08), f.cube]),
             (f"sphere PBR, albedo 0.8, roughness 0.5, metallic 0.5 x a {SIDE} x {SIDE} base-colour and a {SIDE} x {SIDE} orm image + diffuse cube (path_kernel<TexObjects>)",
              [fl.sphere(f, pbr, uv=uv, texture=base, orm_texture=orm), f.cube]),
             ("sphere PBR, albedo 0.8, roughness 0.5, metallic 0.5, no flag + diffuse cube (path_kernel<PbrObjects>, the parent's kernel)",
              [fl.sphere(f, pbr), f.cube])]
    tracers = [fl.tracer(f, ob) for _, ob in cases]
    assert [tr.stats["n_textured_objects"] for tr in tracers] == [1, 0, 1, 0]
    _, times, n_rays = fl.alternate(f, fl.render_runs(f, tracers), a_.repeats)
    lines = [fl.HEADER]
    for k, (label, _) in enumerate(cases):
        lines.append(fl.time_line(label, times[k], n_rays[k], a_.repeats) + f", n_textured_objects {tracers[k].stats['n_textured_objects']}")
    for name, (p, q) in (("base colour, diffuse: textured / untextured", (0, 1)), ("base colour + orm, PBR: textured / untextured", (2, 3))):
        lines.append(f"{name}: best {min(times[p]) / min(times[q]):.4f}, median {np.median(times[p]) / np.median(times[q]):.4f}; "
                     f"rays {n_rays[p] / n_rays[q]:.6f}; the twin's own spread {min(times[q]):.2f}-{max(times[q]):.2f} ms")
    fl.write_lines(a_.out, lines)


if __name__ == "__main__":
    main()
