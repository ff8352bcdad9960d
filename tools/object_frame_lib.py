"""What the *_frame.py tools share: the 512 x 512 frame of tests/golden/indoor2.npz with a 1280-triangle sphere and a cube in front of
the depth mesh (the frame of tests/test_gpu_path_oi.py::test_indoor2_frame_with_objects), the alternating hip-event timer, the
registers of a kernel read from the gfx950 assembly, and the writer of a tool's lines.  Needs a GPU: there is no fallback."""
import argparse
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FOV = 35.0
HEADER = ("512x512 indoor2 frame, spp 32, max_depth 16, a 1280-triangle sphere and a 12-triangle cube in front of the depth mesh; hip events, "
          "one process, alternating")
VGPRS_PER_SIMD, VGPR_GRANULE, MAX_WAVES = 512, 8, 8                      # gfx950: one file for arch and accumulation registers


def arguments(doc, tool, repeats, argv=None, isa=False, **more):
    """The tool's options (--out, --repeats, --isa where it reads registers, `more`: name -> default of a float option), parsed from
    `argv` (None: the command line); ends the tool where there is no GPU."""
    ap = argparse.ArgumentParser(description=doc)
    ap.add_argument("--out", required=True)
    ap.add_argument("--repeats", type=int, default=repeats)
    if isa:
        ap.add_argument("--isa", default=None, help="the gfx950 assembly of matpbr_path.hip: registers and waves per SIMD are read from it")
    for name, default in more.items():
        ap.add_argument("--" + name, type=float, default=default)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool} needs a GPU")
    return args


def indoor2_frame():
    """The frame on cuda:0: the maps a, r, m, the envmap, the depth mesh rm, H, W, the distance z0 the objects stand at, the uploader
    t, and the sphere (Vs, Ts, Ns, its centre) and the cube (a diffuse object) placed in it."""
    import path_oi_fp64 as po
    import path_oi_smooth_fp64 as ps
    from materialist_amd import mesh

    dev = torch.device("cuda:0")
    z = np.load(os.path.join(ROOT, "tests", "golden", "indoor2.npz"))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
    depth = z["depth_pred_f32"]
    depth = 2 * depth.max() - depth
    z0 = 0.6 * float(depth[depth > 0].min())
    centre = np.array([-0.10 * z0, 0.0, -z0])
    Vs, Ts, Ns = ps.icosphere(tuple(centre), 0.09 * z0, 3)
    Vc, Tc = po.cube((0.13 * z0, -0.05 * z0, -z0), 0.13 * z0, (0.3, 0.6, 0.2))
    assert Ts.shape[0] == 1280
    return SimpleNamespace(dev=dev, t=t, a=t(z["ref_albedo_u8"].astype(np.float32) / 255.0),
                           r=t(z["ref_roughness_u8"].astype(np.float32)[..., None] / 255.0).clamp(0.07, 1.0),
                           m=t(z["ref_metallic_u8"].astype(np.float32)[..., None] / 255.0), env=z["ref_envmap_f32"], H=depth.shape[0], W=depth.shape[1],
                           rm=mesh.reference_mesh(depth, FOV), z0=z0, centre=centre, Vs=Vs, Ts=Ts, Ns=Ns,
                           cube={"vertices": Vc, "triangles": Tc, "bsdf": po.DIFFUSE_08})


def sphere(f, bsdf, **extra):
    return {"vertices": f.Vs, "triangles": f.Ts, "bsdf": bsdf, **extra}


def tracer(f, objects=None):
    from materialist_amd import pathtrace as pt

    return pt.PathTracer(f.rm["vertices"], f.rm["triangles"], f.H, f.W, FOV, objects=objects)


def alternate(f, runs, repeats, count_rays=True):
    """Each of `runs` (functions of `rays`, an int32 [H,W] counter or None) once as a warm-up, then `repeats` rounds of all of them in
    turn under hip events -> (what the warm-ups returned, per run its times in ms, per run the rays of its last timed call)."""
    warm = [run(None) for run in runs]
    torch.cuda.synchronize()
    times, n_rays = [[] for _ in runs], [0.0] * len(runs)
    for _ in range(repeats):
        for k, run in enumerate(runs):
            rays = torch.zeros(f.H, f.W, dtype=torch.int32, device=f.dev) if count_rays else None
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(rays)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
            if count_rays:
                n_rays[k] = float(rays.to(torch.float64).sum())
    return warm, times, n_rays


def render_runs(f, tracers, spp=32, max_depth=16, seed=1):
    """`render` of each tracer over the frame's maps under one set of envmap tables, as `alternate` takes them; the warm-up's render
    must be finite."""
    kw = dict(spp=spp, max_depth=max_depth, seed=seed, tables=tracers[0].tables(f.env))

    def run_of(tr):
        def run(rays):
            out = tr.render(f.a, f.r, f.m, f.env, rays=rays, **kw)
            assert rays is not None or bool(torch.isfinite(out).all())
            return out
        return run

    return [run_of(tr) for tr in tracers]


def time_line(label, times, n_rays, repeats):
    best = min(times)
    return (f"{label}: {best:.2f} ms (best of {repeats} after a warm-up; median {float(np.median(times)):.2f}, worst {max(times):.2f}), "
            f"{n_rays / 1e6:.2f} Mrays, {n_rays / 1e3 / best:.0f} Mrays/s")


def kernel_resources(isa_path, names=("DiffObjects", "TexObjects", "ObjTable", "NoObjects"), prefix="path_kernelINS_"):
    """Per kernel whose mangled name holds prefix + len(name) + name + "E" (`path_kernel<name>` by default): (VGPRs, allocated, waves
    per SIMD, scratch bytes, LDS bytes) from the assembly's .amdhsa_ directives."""
    text = open(isa_path).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, flags=re.S):
        d = dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
        for name in names:
            if f"{prefix}{len(name)}{name}E" in m.group(1):
                v = int(d["next_free_vgpr"])
                alloc = -(-v // VGPR_GRANULE) * VGPR_GRANULE
                out[name] = (v, alloc, min(MAX_WAVES, VGPRS_PER_SIMD // alloc), int(d["private_segment_fixed_size"]), int(d["group_segment_fixed_size"]))
    return out


def resource_lines(isa_path, names, prefix="path_kernelINS_", label="path_kernel<{}>"):
    if not isa_path:
        return ["registers: no --isa given"]
    return [f"{label.format(name)}: {v} VGPRs ({alloc} allocated), {waves} waves per SIMD, scratch {scratch} B, LDS {lds} B per workgroup"
            for name, (v, alloc, waves, scratch, lds) in kernel_resources(isa_path, names, prefix).items()]


def write_lines(out, lines):
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
