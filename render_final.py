#!/usr/bin/env python3
"""Command line of the forward-only re-render, same flags as the reference's render_final.py (:420-449); `--mode rolling`
(the function the reference ships but never wires) is available.  See materialist_amd/relight.py."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter, description="re-render an optimised scene under new lighting")
    ap.add_argument("--env_path", required=False, default=None, type=str)
    ap.add_argument("--save_name", required=True, type=str)
    ap.add_argument("--mode", required=True, type=str, help="real, rolling, or oi (object insertion: <scene>/oi.ply as glass and <scene>/oi2.ply as a diffuse object, or the objects of --oi_scene, path traced)")
    ap.add_argument("--input_path", required=False, default=None, type=str)
    ap.add_argument("--save_path", required=False, default=None, type=str)
    ap.add_argument("--frames", type=int, default=36)
    ap.add_argument("--rotation_step", type=float, default=10.0)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--edit_albedo", type=float, nargs=3, default=None, metavar=("DH", "DS", "DV"),
                    help="HSV shift of the albedo inside best_results/mask.png (the reference's `edit` dict, hard-wired to None in its CLI)")
    ap.add_argument("--edit_roughness", type=float, default=None, help="constant roughness inside the mask")
    ap.add_argument("--edit_metallic", type=float, default=None, help="constant metallic inside the mask")
    ap.add_argument("--edit_composite", action="store_true",
                    help="--mode real --integrator path with an --edit_*: differential rendering of the edit: the photograph with what the "
                         "edited maps change, inter-reflection included, not a re-render of the fitted scene; pixels no edited texel reaches "
                         "keep the photograph's bits.  Writes mi_ec_<name>_<env>_<edit flag>.exr / .png.  Not with --denoise atrous or an "
                         "--env_scale other than 1")
    ap.add_argument("--edit_photo", type=str, default=None, metavar="PATH",
                    help="--edit_composite: the photograph, of the maps' size (default <scene>/gt_image.exr, linear; a .png holds display values)")
    ap.add_argument("--edit_transfer", choices=["additive", "ratio"], default=None,
                    help="--edit_composite: additive (the default) = the model's difference is added to the photograph; ratio = where the edit "
                         "darkens a channel the photograph is dimmed by the share of light the model loses, so a badly fitted albedo cancels")
    ap.add_argument("--relight_composite", action="store_true",
                    help="--mode real or rolling with --integrator path: relighting in the photograph: the photograph times the model's "
                         "radiance under the new envmap (--env_path times --env_scale; a rolling frame's rolled envmap) over its radiance "
                         "under the fitted best_results/envmap.hdr, both from one walk, not a re-render of the fitted scene.  Writes "
                         "mi_rc_<name>_<env>_.exr / .png, or rolling_rc_<name>_<env>.mp4 / .gif and their frames.  Not with an --edit_* flag, "
                         "--edit_composite or --mode oi")
    ap.add_argument("--relight_photo", type=str, default=None, metavar="PATH",
                    help="--relight_composite: the photograph, of the maps' size (default <scene>/gt_image.exr, linear; a .png holds display values)")
    ap.add_argument("--relight_floor", type=float, default=None, metavar="F",
                    help="--relight_composite: the radiance added to both sides of the ratio, which bounds it where the model is dark "
                         "(default: 0.01 x the frame's mean radiance under the fitted envmap)")
    ap.add_argument("--integrator", choices=("sh", "path"), default="sh",
                    help="sh: the deterministic render (direct light under SH25, no shadows); path: the path tracer on the scene's .ply "
                         "(Mitsuba's `path` as the reference renders its final images: shadows, inter-reflection, the envmap's texels); "
                         "ignored by --mode oi, which always path traces")
    ap.add_argument("--max_depth", type=int, default=4, help="--integrator path: Mitsuba's max_depth (1 emission, 2 direct + shadows, 4 the reference's)")
    ap.add_argument("--seed", type=int, default=0, help="--integrator path and --mode oi: random seed")
    ap.add_argument("--shading_normals", choices=("face", "map"), default="face",
                    help="--integrator path: face = shade with the mesh's face normals (default); map = shade with best_results/normal.exr")
    ap.add_argument("--denoise", choices=("off", "atrous"), default="off",
                    help="--integrator path and --mode oi: atrous = split every render into two halves of spp/2 with independent seeds and pass "
                         "their mean through the variance-guided a-trous filter (needs an even --spp); off = the plain average")
    ap.add_argument("--oi_iters", type=int, default=10, help="--mode oi: renders averaged (seeds seed, seed + 1, ...)")
    ap.add_argument("--oi_normals", choices=["flat", "vertex"], default="flat",
                    help="--mode oi: flat = face normals; vertex = each .ply shades smooth with its vertex normals (angle-weighted ones if it has none)")
    ap.add_argument("--oi_colors", choices=["none", "vertex", "vertex_linear"], default="none",
                    help="--mode oi without --oi_scene: tint oi2.ply, the diffuse object, with its file's vertex colours (red green blue): vertex = "
                         "decoded from display values to linear; vertex_linear = as written (an --oi_scene entry says \"colors\" itself)")
    ap.add_argument("--oi_texture", type=str, default=None, metavar="PATH",
                    help="--mode oi without --oi_scene: texture oi2.ply, the diffuse object, with this image over its file's per-vertex texture "
                         "coordinates (s t, u v or texture_u texture_v): a PNG holds display values, an .exr or .hdr linear ones in [0, 1] (an "
                         "--oi_scene entry says \"texture\" and, a pbr one, \"orm_texture\" itself)")
    ap.add_argument("--oi_scene", type=str, default=None, metavar="FILE.json",
                    help='--mode oi: an object list, {"objects": [{"ply": path relative to the file, "bsdf": {"type": "pbr", "albedo": [r, g, b], '
                         '"roughness": r, "metallic": m} (or a "dielectric" or "diffuse" one, or {"type": "roughdielectric", "int_ior": n, "ext_ior": n, "alpha": a}, frosted glass, or {"type": "area", "radiance": [r, g, b]}, a lamp), "normals": "flat" or "vertex"}, ...]}, at most 8 '
                         "objects; with it <scene>/oi.ply and <scene>/oi2.ply are not looked for and --oi_normals is ignored")
    ap.add_argument("--oi_tint", type=float, nargs=3, default=None, metavar=("R", "G", "B"),
                    help="--mode oi without --oi_scene: tint oi.ply, the glass, with an absorbing medium inside it: the colour, each channel in "
                         "(0, 1], that white light has after --oi_tint_at inside the glass (an --oi_scene entry says \"medium\": {\"color\": [r, g, b], "
                         "\"at\": d} or {\"sigma_a\": [r, g, b], \"scatter\": s, \"g\": g} itself, on a dielectric or roughdielectric object)")
    ap.add_argument("--oi_tint_at", type=float, default=None, metavar="D",
                    help="--oi_tint: the distance, in scene units, at which the glass has that colour (default: the largest side of the "
                         "mesh's bounding box)")
    ap.add_argument("--env_scale", type=float, default=1.0, metavar="S",
                    help="--integrator path and --mode oi: multiply the envmap by S before its sampling tables are built (1 = the same bits as "
                         "without it; 0 with an area light in --oi_scene = the night shot, lit by the lamp alone)")
    ap.add_argument("--oi_composite", action="store_true",
                    help="--mode oi: differential rendering (Debevec 1998): the photograph with the objects, their shadows, bounce light and "
                         "reflections added, not a re-render of the fitted scene; pixels nothing reaches keep the photograph's bits.  Writes "
                         "mi_oic_<name>_<env>.exr / .png.  Not with --denoise atrous or an --env_scale other than 1")
    ap.add_argument("--oi_composite_denoise", action="store_true",
                    help="--oi_composite: split every frame into two differential renders of spp/2 with independent seeds and pass each "
                         "pixel's own layer (the object where it is seen, else what it adds to and takes from the scene) through the "
                         "a-trous filter before the composite (needs an even --spp); pixels farther than the filter's reach from every "
                         "touched one keep the photograph's bits")
    ap.add_argument("--oi_see_through", action="store_true",
                    help="--oi_composite: behind clear inserted glass (a dielectric object, flat or smooth) show the photograph, refracted, "
                         "plus what the objects change in the light of the point seen, instead of the re-rendered fitted scene.  It does not "
                         "cover rough (frosted) glass, which stays re-rendered, nor paths that leave the glass towards another object, a "
                         "lamp or the envmap")
    ap.add_argument("--oi_reflect_photo", action="store_true",
                    help="--oi_composite (implies --oi_see_through): what an inserted diffuse, pbr or rough-glass object reflects of the scene "
                         "is the photograph, not the re-rendered fitted scene: a chrome ball mirrors the room as photographed.  It holds for "
                         "every such object whose --oi_scene entry does not say \"photo\": false (of the default pair, oi2.ply).  The "
                         "photograph is taken as the light a point sends in every direction, and with --oi_composite_denoise the reflected "
                         "photograph is not filtered")
    ap.add_argument("--oi_shadows", choices=["additive", "ratio"], default="additive",
                    help="--oi_composite: how what the objects darken reaches the photograph: additive = the model's difference is added "
                         "(the default); ratio = the photograph is dimmed, per channel, by the share of light the model loses, so a badly "
                         "fitted albedo cancels and the photograph's texture stays inside a shadow (what the objects brighten stays additive)")
    ap.add_argument("--oi_photo", type=str, default=None, metavar="PATH",
                    help="--oi_composite: the photograph, of the maps' size (default <scene>/gt_image.exr, linear, as the pipeline writes it; a "
                         ".png holds display values and is decoded as the pipeline decodes its input)")
    ap.add_argument("--oi_frames", type=int, default=1, metavar="N",
                    help="--mode oi with --oi_scene: N > 1 renders a video of the objects whose entry carries a \"motion\" ({\"spin\": {\"axis\": "
                         "[x, y, z], \"deg_per_frame\": a}, \"slide\": [dx, dy, dz]}), each frame with the options given, into "
                         "<out>/oi_animation/frame_%%04d.png and mi_oi[c]_<name>_<env>.mp4 / .gif; 1 = a still, a \"transform\" baked in")
    ap.add_argument("--oi_max_depth", type=int, default=16, help="--mode oi: Mitsuba's max_depth (a camera path through glass needs 5 to see light)")
    a = ap.parse_args(argv)
    if a.shading_normals == "map" and (a.integrator != "path" or a.mode == "oi"):
        ap.error("--shading_normals map needs --integrator path and --mode real or rolling (inserted objects know no normal map)")
    if not (a.env_scale >= 0 and a.env_scale < float("inf")):
        ap.error("--env_scale must be finite and >= 0")
    if a.env_scale != 1.0 and a.mode != "oi" and a.integrator != "path":
        ap.error("--env_scale needs --integrator path (or --mode oi): the sh render projects the envmap as it is")
    if a.oi_composite and a.mode != "oi":
        ap.error("--oi_composite needs --mode oi")
    if a.oi_photo is not None and not a.oi_composite:
        ap.error("--oi_photo needs --oi_composite")
    if a.oi_composite and a.denoise == "atrous":
        ap.error("--oi_composite knows no --denoise atrous: the filter takes a radiance image, not a signed difference "
                 "(--oi_composite_denoise runs the differential render's own filter)")
    if a.oi_composite_denoise and not a.oi_composite:
        ap.error("--oi_composite_denoise needs --oi_composite")
    if a.oi_see_through and not a.oi_composite:
        ap.error("--oi_see_through needs --oi_composite")
    if a.oi_reflect_photo and not a.oi_composite:
        ap.error("--oi_reflect_photo needs --oi_composite")
    if a.oi_shadows != "additive" and not a.oi_composite:
        ap.error("--oi_shadows ratio needs --oi_composite")
    if a.oi_composite_denoise and (a.spp < 2 or a.spp % 2):
        ap.error("--oi_composite_denoise splits every frame into two halves of spp/2 samples: --spp must be even")
    if a.oi_composite and a.env_scale != 1.0:
        ap.error("--oi_composite needs --env_scale 1: the photograph was taken under the envmap as it is and is not dimmed")
    if a.edit_composite and a.mode != "real":
        ap.error("--edit_composite needs --mode real (--mode oi composites inserted objects with --oi_composite; a rolling envmap relights "
                 "every pixel, which is no edit)")
    if a.edit_composite and a.integrator != "path":
        ap.error("--edit_composite needs --integrator path")
    if a.edit_composite and a.edit_albedo is None and a.edit_roughness is None and a.edit_metallic is None:
        ap.error("--edit_composite needs an edit: --edit_albedo, --edit_roughness or --edit_metallic")
    if a.edit_composite and a.denoise == "atrous":
        ap.error("--edit_composite knows no --denoise atrous: the filter takes a radiance image, not a signed difference")
    if a.edit_composite and a.env_scale != 1.0:
        ap.error("--edit_composite needs --env_scale 1: the photograph was taken under the envmap as it is and is not dimmed")
    if a.edit_photo is not None and not a.edit_composite:
        ap.error("--edit_photo needs --edit_composite")
    if a.edit_transfer is not None and not a.edit_composite:
        ap.error("--edit_transfer needs --edit_composite")
    if (a.relight_photo is not None or a.relight_floor is not None) and not a.relight_composite:
        ap.error("--relight_photo and --relight_floor need --relight_composite")
    if a.oi_tint is not None and (a.mode != "oi" or a.oi_scene is not None):
        ap.error("--oi_tint needs --mode oi without --oi_scene (an --oi_scene entry says \"medium\" itself)")
    if a.oi_tint is not None and not all(0 < c <= 1 for c in a.oi_tint):
        ap.error("--oi_tint: every channel must lie in (0, 1]")
    if a.oi_tint_at is not None and (a.oi_tint is None or not (0 < a.oi_tint_at < float("inf"))):
        ap.error("--oi_tint_at needs --oi_tint and must be finite and > 0")
    if a.oi_frames < 1:
        ap.error("--oi_frames must be at least 1")
    if a.oi_frames > 1 and (a.mode != "oi" or a.oi_scene is None):
        ap.error("--oi_frames N > 1 needs --mode oi and an --oi_scene in which an object has a \"motion\"")
    if a.denoise == "atrous":
        if a.mode != "oi" and a.integrator != "path":
            ap.error("--denoise atrous needs --integrator path (or --mode oi): the sh render is deterministic and has no noise to filter")
        if a.spp < 2 or a.spp % 2:
            ap.error("--denoise atrous splits every render into two halves of spp/2 samples: --spp must be even")
    return a


def main(argv=None):
    a = parse_args(argv)
    from materialist_amd import relight

    edit = {"albedo": a.edit_albedo, "roughness": a.edit_roughness, "metallic": a.edit_metallic}
    it = {"integrator": a.integrator, "max_depth": a.max_depth, "seed": a.seed, "shading_normals": a.shading_normals, "denoise": a.denoise,
          "env_scale": a.env_scale}
    rc = {"relight_composite": True, "relight_photo": a.relight_photo, "relight_floor": a.relight_floor} if a.relight_composite else {}
    if a.relight_composite and a.mode == "oi":
        raise ValueError("--relight_composite knows no --mode oi: inserted objects and lights are not in the walk under two envmaps "
                         "(--oi_composite puts objects into the photograph under the fitted light)")
    if a.mode == "real":
        ec = {"composite": True, "photo_path": a.edit_photo, "transfer": a.edit_transfer or "additive"} if a.edit_composite else {}
        print("Wrote file to", relight.render_real(a.save_name, a.env_path, a.input_path, a.save_path, a.spp, edit=edit, **it, **ec, **rc))
    elif a.mode == "rolling":
        res = relight.render_rolling_envmap(a.save_name, a.env_path, a.frames, a.rotation_step, a.input_path, a.save_path, a.spp, edit=edit,
                                            **it, **rc)
        print(f"Animation saved to {res['gif']}\nIndividual frames saved to {res['animation_dir']}")
    elif a.mode == "oi":
        res = relight.render_oi(a.save_name, a.env_path, a.input_path, a.save_path, a.spp, a.oi_iters, a.oi_max_depth, a.seed,
                                object_normals=a.oi_normals, denoise=a.denoise, objects_file=a.oi_scene,
                                env_scale=a.env_scale, object_colors=a.oi_colors, object_texture=a.oi_texture,
                                **({"composite": True, "photo_path": a.oi_photo} if a.oi_composite else {}),
                                **({"composite_denoise": True} if a.oi_composite_denoise else {}),
                                **({"see_through": True} if a.oi_see_through else {}),
                                **({"shadows": a.oi_shadows} if a.oi_shadows != "additive" else {}),
                                **({"frames": a.oi_frames} if a.oi_frames != 1 else {}),
                                **({"tint": a.oi_tint, "tint_at": a.oi_tint_at} if a.oi_tint is not None else {}),
                                **({"reflect_photo": True} if a.oi_reflect_photo else {}))
        if a.oi_frames > 1:
            print(f"Animation saved to {res['mp4']}\nIndividual frames saved to {res['animation_dir']}")
        else:
            print("Wrote file to", res)
    else:
        raise ValueError("Invalid mode")


if __name__ == "__main__":
    main()
