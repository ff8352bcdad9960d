#!/usr/bin/env python3
"""Time moving inserted objects ("Moving inserted objects") on the 512 x 512 frame of tests/golden/indoor2.npz
(the frame of tools/pbr_object_frame.py: the 1280-triangle sphere as a smooth chrome ball, and the cube).  Three measurements, each
alternating in one process, the best and the median of `--repeats` timed calls after a warm-up:
  * the move itself: `PathTracer.move_objects` (checks, the move launch, the refit launch; hip events and wall clock) against what the
    static route costs for the same new pose: `build_bvh` of the merged mesh plus the upload of its nodes and triangles (wall clock, the
    device idle at both ends); then the same with a 100 000-triangle sphere in the ball's place;
  * the price in the render: `render` and `render_diff` through the grafted BVH and through the merged BVH of the same pose, at rest and
    with the ball spun 45 degrees (the grafted tree keeps its rest-pose topology, the merged one is rebuilt), with the rays and the
    twin's own spread;
  * one 36-frame spin of the ball in the ratio composite at spp 32 x 1: wall time per frame, split into move, features, render and write.
With `--isa` the registers, scratch and LDS of the two new kernels.  Writes profiles/moving_objects_frame.txt's lines to --out.  Needs a
GPU: there is no fallback."""
import ctypes
import os
import tempfile
import time

import numpy as np
import torch

import object_frame_lib as fl  # puts the repository and tests/ on the path

import path_oi_fp64 as po

CHROME = {"type": "pbr", "albedo": (0.95, 0.93, 0.88), "roughness": 0.1, "metallic": 1.0}


def _uv_sphere(centre, radius, n_lon=250, n_lat=201):
    """A latitude-longitude sphere of 2 n_lon (n_lat - 1) triangles, outward winding -> (V, T, N)."""
    th = np.linspace(0.0, np.pi, n_lat + 1)
    ph = np.linspace(0.0, 2 * np.pi, n_lon, endpoint=False)
    n = np.stack([np.sin(th)[:, None] * np.cos(ph)[None], np.cos(th)[:, None] * np.ones_like(ph)[None], np.sin(th)[:, None] * np.sin(ph)[None]], -1).reshape(-1, 3)
    idx = np.arange((n_lat + 1) * n_lon).reshape(n_lat + 1, n_lon)
    a, b, c, d = idx[:-1], np.roll(idx[:-1], -1, 1), idx[1:], np.roll(idx[1:], -1, 1)
    upper = np.stack([a, b, c], -1)[1:].reshape(-1, 3)               # the cap rows keep one triangle a cell: the other has no area
    lower = np.stack([b, d, c], -1)[:-1].reshape(-1, 3)
    return n * radius + np.asarray(centre), np.concatenate([upper, lower]).astype(np.int32), n


def _wall(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3, out


def _stats(times, unit=1.0, digits=3):
    return f"best {min(times) * unit:.{digits}f}, median {float(np.median(times)) * unit:.{digits}f}, worst {max(times) * unit:.{digits}f}"


def _move_against_rebuild(f, pt, ball, repeats, label):
    """Alternating: `move_objects` to a fresh pose, and the static route to the same pose (`merge_scene`'s arrays moved on the host are not
    counted: `build_bvh` of the moved merged mesh and the upload alone)."""
    objects = [ball, f.cube]
    tracer = pt.PathTracer(f.rm["vertices"], f.rm["triangles"], f.H, f.W, fl.FOV, objects=objects, movable=True)
    n_scene = f.rm["triangles"].shape[0]
    poses = [[{"rotate": {"axis": (0, 1, 0), "deg": 10.0 * (k + 1)}}, {"translate": (0.0, 0.001 * k, 0.0)}] for k in range(repeats + 1)]
    ev, wall, static, build, upload = [], [], [], [], []
    for k, pose in enumerate(poses):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(f.dev)
        t0 = time.perf_counter()
        e0.record()
        tracer.move_objects(pose)
        e1.record()
        torch.cuda.synchronize(f.dev)
        w = (time.perf_counter() - t0) * 1e3
        # the static route to the same pose
        moved = [dict(ob, vertices=pt.apply_similarity(pt.similarity(tr, pivot=0.5 * (ob["vertices"].min(0) + ob["vertices"].max(0))), ob["vertices"]))
                 for ob, tr in zip(objects, pose)]
        V, T, _ = pt.merge_objects(f.rm["vertices"], f.rm["triangles"], moved)
        t_build, bvh = _wall(lambda: pt.build_bvh(V, T, n_scene), f.dev)
        t_up, _ = _wall(lambda: (torch.from_numpy(bvh["nodes"]).to(f.dev), torch.from_numpy(bvh["tris"]).to(f.dev)), f.dev)
        if k:                                                         # the first round is the warm-up
            ev.append(e0.elapsed_time(e1)), wall.append(w), build.append(t_build), upload.append(t_up), static.append(t_build + t_up)
    mb = (bvh["nodes"].nbytes + bvh["tris"].nbytes) / 1e6
    # the library call alone (the two launches, without the binding's checks in Python), 20 calls between one pair of events
    records, mv = tracer.poses(poses[-1]), tracer._move
    fn, table = pt.symbol("matpbr_path_objects_move"), pt._table_ptrs(tracer.objects)[0]
    ptr = lambda x: None if x is None else x.data_ptr()
    raw = []
    for k in range(repeats + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(f.dev)
        e0.record()
        for _ in range(20):
            pt.check(fn(tracer.nodes.data_ptr(), tracer.tris.data_ptr(), mv["rest_tris"].data_ptr(), n_scene, tracer.stats["n_object_tris"], mv["first_object_node"],
                        mv["n_object_nodes"], mv["node_level"].data_ptr(), mv["object_depth"], table, len(tracer.objects), ctypes.cast(records, ctypes.c_void_p),
                        mv["pad"], ptr(mv["rest_nrm"]), ptr(tracer.obj_nrm), None, None, 0, None, torch.cuda.current_stream(f.dev).cuda_stream),
                     "matpbr_path_objects_move")
        e1.record()
        torch.cuda.synchronize(f.dev)
        if k:
            raw.append(e0.elapsed_time(e1) / 20)
    return [f"{label}: {tracer.stats['n_object_tris']} object triangles, {tracer._move['n_object_nodes']} object nodes, object depth "
            f"{tracer._move['object_depth']}; scene {n_scene} triangles",
            f"  move_objects (checks + move launch + refit launch), hip events: {_stats(ev, 1e3, 1)} us; wall clock to idle: {_stats(wall, 1e3, 1)} us "
            f"(best of {repeats} after a warm-up)",
            f"  matpbr_path_objects_move alone (both launches back to back, 20 calls between one pair of hip events): {_stats(raw, 1e3, 1)} us a call",
            f"  static route to the same pose, wall clock: build_bvh of the merged mesh {_stats(build)} ms + upload of {mb:.1f} MB {_stats(upload)} ms = "
            f"{_stats(static)} ms",
            f"  static / move: {min(static) / min(wall):.0f}x by the bests' wall clock ({min(static) * 1e3 / (min(ev) * 1e3):.0f}x against the hip events), "
            f"{float(np.median(static)) / float(np.median(wall)):.0f}x by the medians"]


def _render_price(f, pt, ball, repeats, deg):
    """`render` and `render_diff` through the grafted and the merged BVH of one pose."""
    objects = [ball, f.cube]
    pose = [{"rotate": {"axis": (0, 1, 0), "deg": deg}}, None]
    grafted = pt.PathTracer(f.rm["vertices"], f.rm["triangles"], f.H, f.W, fl.FOV, objects=objects, movable=True)
    grafted.move_objects(pose)
    sim = pt.similarity(pose[0], pivot=0.5 * (ball["vertices"].min(0) + ball["vertices"].max(0)))
    moved = dict(ball, vertices=pt.apply_similarity(sim, ball["vertices"]), normals=pt.apply_similarity(sim, ball["normals"], vectors=True))
    merged = fl.tracer(f, [moved if deg else ball, f.cube])
    kw = dict(spp=32, max_depth=16, seed=1, tables=grafted.tables(f.env))
    lines = []
    for name in ("render", "render_diff"):
        runs = [lambda rays, tr=tr: getattr(tr, name)(f.a, f.r, f.m, f.env, rays=rays, **kw) for tr in (grafted, merged)]
        warm, times, n_rays = fl.alternate(f, runs, repeats)
        first = [w if name == "render" else w[0] for w in warm]
        assert all(bool(torch.isfinite(x).all()) for x in first)
        close = float(((first[0] - first[1]).abs() <= 1e-3 * first[1].abs().clamp_min(float(first[1].abs().mean()))).all(-1).double().mean())
        lines.append(fl.time_line(f"  {name}, grafted BVH (depth {grafted.stats['depth']}, {grafted.stats['n_nodes']} nodes)", times[0], n_rays[0], repeats))
        lines.append(fl.time_line(f"  {name}, merged BVH (depth {merged.stats['depth']}, {merged.stats['n_nodes']} nodes)", times[1], n_rays[1], repeats))
        best, spread = min(times[0]) / min(times[1]), max(times[1]) / min(times[1])
        lines.append(f"  {name}, grafted / merged: time best {best:.4f}, median {float(np.median(times[0]) / np.median(times[1])):.4f}; rays "
                     f"{n_rays[0] / n_rays[1]:.4f}; the merged twin's own spread (worst / best) {spread:.4f}: the ratio of the bests lies "
                     f"{'inside' if 1.0 / spread <= best <= spread else 'outside'} it; pixels of the two pictures within 1e-3: {close:.4f}")
    return [f"ball spun {deg:g} degrees about y:"] + lines


def _spin(f, pt, ball, frames=36):
    from materialist_amd import loss
    from materialist_amd.pipeline import write_png

    tracer = pt.PathTracer(f.rm["vertices"], f.rm["triangles"], f.H, f.W, fl.FOV, objects=[ball, f.cube], movable=True)
    tabs = tracer.tables(f.env)
    photo = f.t(np.random.default_rng(3).gamma(2.0, 0.5, (f.H, f.W, 3)))
    split = {k: [] for k in ("move", "features", "render", "write")}
    with tempfile.TemporaryDirectory() as tmp:
        for k in range(frames + 1):                                   # frame 0 twice: the first is the warm-up
            pose = [{"rotate": {"axis": (0, 1, 0), "deg": 10.0 * max(k - 1, 0)}}, None]
            t_move, _ = _wall(lambda: tracer.move_objects(pose), f.dev)
            t_feat, _ = _wall(lambda: tracer.features(), f.dev)

            def render():
                fg, delta, base, alpha, _ = tracer.render_diff_ratio(f.a, f.r, f.m, f.env, 32, 16, 1, tables=tabs)
                return pt.composite_ratio(fg, delta, base, alpha, photo, 1.0)

            t_render, img = _wall(render, f.dev)
            t_write, _ = _wall(lambda: write_png(os.path.join(tmp, f"frame_{k:04d}.png"), loss.linear_to_srgb(img.clamp_min(0)).clamp(0, 1).cpu().numpy()), f.dev)
            if k:
                for key, t in zip(split, (t_move, t_feat, t_render, t_write)):
                    split[key].append(t)
    total = sum(float(np.mean(v)) for v in split.values())
    return [f"{frames}-frame spin of the chrome ball, ratio composite, spp 32 x 1, max_depth 16, wall clock per frame (mean over the frames; median): "
            + ", ".join(f"{key} {float(np.mean(v)):.3f} ms ({float(np.median(v)):.3f})" for key, v in split.items())
            + f"; {total:.1f} ms a frame, {total * frames / 1e3:.2f} s for the {frames} frames"]


def main(argv=None):
    from materialist_amd import pathtrace as pt

    a_ = fl.arguments(__doc__, "moving_objects_frame.py", 7, argv, isa=True)
    f = fl.indoor2_frame()
    ball = fl.sphere(f, CHROME, normals=f.Ns)
    Vb, Tb, Nb = _uv_sphere(f.centre, 0.09 * f.z0)
    big = {"vertices": Vb, "triangles": Tb, "bsdf": CHROME, "normals": Nb}
    lines = ["512x512 indoor2 frame, a 1280-triangle smooth chrome sphere and a 12-triangle diffuse cube in front of the depth mesh; one process, alternating"]
    lines += _move_against_rebuild(f, pt, ball, a_.repeats, "the frame's objects")
    lines += _move_against_rebuild(f, pt, big, a_.repeats, "a 100 000-triangle sphere in the ball's place")
    lines.append("the price in the render, spp 32, max_depth 16, hip events:")
    for deg in (0.0, 45.0):
        lines += _render_price(f, pt, ball, a_.repeats, deg)
    lines += _spin(f, pt, ball)
    if a_.isa:
        lines += fl.resource_lines(a_.isa, ("objects_move_kernel", "objects_refit_kernel"), prefix="_GLOBAL__N_1", label="{}")
    fl.write_lines(a_.out, lines)


if __name__ == "__main__":
    main()
