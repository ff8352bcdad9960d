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
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

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
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", required=True)
    ap.add_argument("--repeats", type=int, default=7)
    a_ = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("texture_object_frame.py needs a GPU")
    import path_oi_fp64 as po
    import path_oi_smooth_fp64 as ps
    from materialist_amd import mesh, pathtrace as pt

    dev = torch.device("cuda:0")
    z = np.load(os.path.join(ROOT, "tests", "golden", "indoor2.npz"))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    a = t(z["ref_albedo_u8"].astype(np.float32) / 255.0)
    r = t(z["ref_roughness_u8"].astype(np.float32)[..., None] / 255.0).clamp(0.07, 1.0)
    m = t(z["ref_metallic_u8"].astype(np.float32)[..., None] / 255.0)
    env = z["ref_envmap_f32"]
    depth = z["depth_pred_f32"]
    depth = 2 * depth.max() - depth
    H, W = depth.shape
    rm = mesh.reference_mesh(depth, 35.0)
    z0 = 0.6 * float(depth[depth > 0].min())
    centre = np.array([-0.10 * z0, 0.0, -z0])
    Vs, Ts, _ = ps.icosphere(tuple(centre), 0.09 * z0, 3)
    Vc, Tc = po.cube((0.13 * z0, -0.05 * z0, -z0), 0.13 * z0, (0.3, 0.6, 0.2))
    assert Ts.shape[0] == 1280
    cube = {"vertices": Vc, "triangles": Tc, "bsdf": po.DIFFUSE_08}
    n = (Vs - centre) / np.linalg.norm(Vs - centre, axis=-1, keepdims=True)
    uv = 2.0 * np.stack([np.arctan2(n[:, 0], n[:, 2]) / (2 * np.pi) + 0.5, np.arccos(np.clip(n[:, 1], -1, 1)) / np.pi], -1)   # the image twice around
    base, orm = images(np.random.default_rng(5))
    pbr = {"type": "pbr", "albedo": (0.8, 0.8, 0.8), "roughness": 0.5, "metallic": 0.5}
    sphere = lambda bsdf, **extra: {"vertices": Vs, "triangles": Ts, "bsdf": bsdf, **extra}
    cases = [(f"sphere diffuse, reflectance 0.8 x a {SIDE} x {SIDE} base-colour image + diffuse cube (path_kernel<TexObjects>)",
              [sphere(po.DIFFUSE_08, uv=uv, texture=base), cube]),
             ("sphere uniformly diffuse, reflectance 0.8, no flag + diffuse cube (path_kernel<ObjTable>, the parent's kernel)",
              [sphere(po.DIFFUSE_08), cube]),
             (f"sphere PBR, albedo 0.8, roughness 0.5, metallic 0.5 x a {SIDE} x {SIDE} base-colour and a {SIDE} x {SIDE} orm image + diffuse cube (path_kernel<TexObjects>)",
              [sphere(pbr, uv=uv, texture=base, orm_texture=orm), cube]),
             ("sphere PBR, albedo 0.8, roughness 0.5, metallic 0.5, no flag + diffuse cube (path_kernel<PbrObjects>, the parent's kernel)",
              [sphere(pbr), cube])]
    tracers = [pt.PathTracer(rm["vertices"], rm["triangles"], H, W, 35.0, objects=ob) for _, ob in cases]
    assert [tr.stats["n_textured_objects"] for tr in tracers] == [1, 0, 1, 0]
    tabs = tracers[0].tables(env)
    kw = dict(spp=32, max_depth=16, seed=1, tables=tabs)
    times, n_rays = [[] for _ in cases], [0.0] * len(cases)
    for tr in tracers:                                                   # warm-up of each
        assert bool(torch.isfinite(tr.render(a, r, m, env, **kw)).all())
    torch.cuda.synchronize()
    for _ in range(a_.repeats):
        for k, tr in enumerate(tracers):                                 # alternating
            rays = torch.zeros(H, W, dtype=torch.int32, device=dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr.render(a, r, m, env, rays=rays, **kw)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
            n_rays[k] = float(rays.to(torch.float64).sum())
    lines = ["512x512 indoor2 frame, spp 32, max_depth 16, a 1280-triangle sphere and a 12-triangle cube in front of the depth mesh; hip events, one process, alternating"]
    for k, (label, _) in enumerate(cases):
        best, med = min(times[k]), float(np.median(times[k]))
        lines.append(f"{label}: {best:.2f} ms (best of {a_.repeats} after a warm-up; median {med:.2f}, worst {max(times[k]):.2f}), "
                     f"{n_rays[k] / 1e6:.2f} Mrays, {n_rays[k] / 1e3 / best:.0f} Mrays/s, n_textured_objects {tracers[k].stats['n_textured_objects']}")
    for name, (p, q) in (("base colour, diffuse: textured / untextured", (0, 1)), ("base colour + orm, PBR: textured / untextured", (2, 3))):
        lines.append(f"{name}: best {min(times[p]) / min(times[q]):.4f}, median {np.median(times[p]) / np.median(times[q]):.4f}; "
                     f"rays {n_rays[p] / n_rays[q]:.6f}; the twin's own spread {min(times[q]):.2f}-{max(times[q]):.2f} ms")
    os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
    with open(a_.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
