"""What the path tests share (tests/test_gpu_path*.py, tests/test_path*_host.py, the denoiser's two files): the library loader behind
their `pt` / `path_lib` fixtures, the tolerance reporter, the bit / parity / footprint helpers and the groove-plus-objects scene.  A
plain module beside path_fp64.py: no fixtures, nothing pytest collects."""
import os

import numpy as np
import pytest

import path_fp64 as pf

FOV = pf.FOV


def load(gpu=False):
    """materialist_amd.pathtrace with libmatpbr_path.so built; `gpu`: skip the caller where there is no GPU."""
    from materialist_amd import build, pathtrace

    build.build_path_library()
    if gpu:
        import torch

        if not torch.cuda.is_available():
            pytest.skip("needs a GPU")
    return pathtrace


def reporter(print_tag, file_tag):
    """-> report(what, value): prints `[print_tag] what: value` and appends `file_tag<TAB>what<TAB>value` to $MATPBR_TOLERANCE_REPORT."""
    def report(what, value):
        print(f"[{print_tag}] {what}: {value}")
        path = os.environ.get("MATPBR_TOLERANCE_REPORT")
        if path:
            with open(path, "a") as f:
                f.write(f"{file_tag}\t{what}\t{value}\n")

    return report


def bits(x):
    return x.cpu().numpy().view(np.uint32)


def parity(got, ref):
    """The renders' criterion: per-pixel error (the worst channel) relative to max(|ref|, mean |ref|) -> (share of pixels within 1e-3,
    the errors)."""
    err = (np.abs(got - ref) / np.maximum(np.abs(ref), np.abs(ref).mean())).max(-1)
    return float((err <= 1e-3).mean()), err


def footprints(objects, H, W, n=9):
    """Per pixel, from an n x n grid of rays over its footprint [j - 1/2, j + 1/2] x [i - 1/2, i + 1/2] (corners included) and the
    objects' projected vertices: (every ray hits an object, no ray hits and no vertex projects into the footprint)."""
    f = (W / 2.0) / np.tan(np.radians(FOV) / 2.0)
    g = np.linspace(-0.5, 0.5, n)
    y, x = np.meshgrid((np.arange(H)[:, None] + g[None]).reshape(-1), (np.arange(W)[:, None] + g[None]).reshape(-1), indexing="ij")
    d = np.stack([(x - (W - 1) / 2) / f, -(y - (H - 1) / 2) / f, -np.ones_like(x)], -1).reshape(-1, 3)
    P = np.concatenate([np.asarray(ob["vertices"], np.float64)[np.asarray(ob["triangles"])] for ob in objects])
    hit = np.isfinite(pf.brute(P, np.zeros_like(d), d)[0]).reshape(H, n, W, n)
    vert = np.zeros((H, W), bool)
    for ob in objects:
        v = np.asarray(ob["vertices"], np.float64)
        px, py = v[:, 0] / -v[:, 2] * f + (W - 1) / 2, -v[:, 1] / -v[:, 2] * f + (H - 1) / 2
        for a, b in zip(px, py):
            vert[max(int(np.floor(b - 0.5)), 0):int(np.ceil(b + 0.5)) + 1, max(int(np.floor(a - 0.5)), 0):int(np.ceil(a + 0.5)) + 1] = True
    return hit.all(axis=(1, 3)), ~hit.any(axis=(1, 3)) & ~vert


def erode(mask):
    m = np.pad(mask, 1, constant_values=False)
    return np.logical_and.reduce([m[1 + di:m.shape[0] - 1 + di, 1 + dj:m.shape[1] - 1 + dj] for di in (-1, 0, 1) for dj in (-1, 0, 1)])


def raw_args(tracer, maps, spp, max_depth, seed, spp_per_launch, out):
    """The arguments of a forward entry point up to `stream`, for calls past `PathTracer.render` -> (the tensors to keep alive, args)."""
    import torch

    keep = tracer._inputs(*maps, None)
    return keep, (*tracer._frame(*keep, spp, max_depth, seed, spp_per_launch), out.data_ptr(), None, torch.cuda.current_stream().cuda_stream)


def object_tail(tracer, entry="matpbr_path_render_objects_rough"):
    """The object arguments of the forward entry point `entry` after `stream`, for calls past `PathTracer.render`: the prefix it takes
    (all eight by default) of the tracer's nine object arguments, its four texture arguments and its medium records."""
    from materialist_amd import pathtrace

    full = (*tracer.object_args()[:9], *tracer._texture_args(), tracer.media_arg())
    return full[:len(full) if entry == pathtrace.MEDIA_ENTRY else pathtrace.OBJECT_ENTRIES[entry]]


def groove_with_objects(pt, objects, merged):
    """The groove at 24 x 20 (a partial tile) with `objects` in front of it; `merged`: the restatement's table builder.  -> the maps,
    the envmap, the mesh `rm`, the merged V, T, table and the tracer."""
    from materialist_amd import mesh

    H, W = 20, 24
    rm = mesh.reference_mesh(pf.groove_scene(H, W), FOV)
    rng = np.random.default_rng(11)
    a, r, m = pf.groove_maps(H, W, rng)
    env = pf.groove_env(rng)
    V, T, table = merged(rm["vertices"], rm["triangles"], objects)
    tracer = pt.PathTracer(rm["vertices"], rm["triangles"], H, W, FOV, objects=objects)
    return {"rm": rm, "a": a, "r": r, "m": m, "env": env, "H": H, "W": W, "objects": objects, "V": V, "T": T, "table": table, "tracer": tracer}


def recorded_walk(entry):
    """What the walk that `path_objects_fp64.replay_objects` replaced returned for `entry` ("smooth", "pbr", "lights", "texture") on
    its own table scene over the groove at 12 x 10, max_depth 6, seed 1, recorded before the copies were folded into one
    (tests/golden/gen_path_replay_chain.py) -> {"L": the render, key: each array of its record}."""
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "path_replay_chain.npz")) as z:
        return {k.split(".", 1)[1]: z[k] for k in z.files if k.startswith(entry + ".")}


def synthetic_output(tmp, name="case", H=32, W=32, edit=False):
    """An output directory of the pipeline as the command lines read it, H x W: best_results/ (the groove's maps, a flat normal map,
    the envmap), depthPred.exr and the mesh <name>.ply -> its path.  `edit`: plus best_results/mask.png (a disc) and an RGBA
    best_results/bg.png, as trans_edit.py reads them -> (its path, the mask)."""
    from materialist_amd import mesh
    from materialist_amd.imageio_exr import write_exr
    from materialist_amd.imageio_hdr import write_hdr

    rng = np.random.default_rng(2)
    scene = os.path.join(tmp, name)
    br = os.path.join(scene, "best_results")
    os.makedirs(br)
    a, r, m = pf.groove_maps(H, W, rng)
    write_exr(os.path.join(br, "albedo.exr"), a)
    write_exr(os.path.join(br, "roughness.exr"), np.repeat(r, 3, -1))
    write_exr(os.path.join(br, "metallic.exr"), np.repeat(m, 3, -1))
    write_exr(os.path.join(br, "normal.exr"), np.tile(np.array([0, 0, 1], np.float32), (H, W, 1)))
    write_hdr(os.path.join(br, "envmap.hdr"), pf.groove_env(rng))
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    pred = (1.0 + 0.3 * (j > W // 2) + 0.002 * i).astype(np.float32)         # depthPred.exr: the pipeline flips it to 2 max - d
    write_exr(os.path.join(scene, "depthPred.exr"), np.repeat(pred[..., None], 3, -1))
    rm = mesh.reference_mesh(2 * pred.max() - pred, FOV)
    mesh.write_ply(os.path.join(scene, f"{name}.ply"), rm["vertices"], rm["triangles"])
    if not edit:
        return scene
    from PIL import Image

    mask = (i - 15) ** 2 + (j - 14) ** 2 < 81
    Image.fromarray(np.repeat((mask * 255).astype(np.uint8)[..., None], 3, -1), "RGB").save(os.path.join(br, "mask.png"))
    Image.fromarray(rng.integers(0, 256, (H, W, 4), dtype=np.uint8), "RGBA").save(os.path.join(br, "bg.png"))
    return scene, mask
