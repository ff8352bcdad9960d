#!/usr/bin/env python3
"""Command line of the inverse-rendering pipeline, same flags as the reference's inverse_img_w_mi.py (:771-801) plus
`--size`, `--spp`, `--num_epochs`, `--pred_dir`, `--integrator` / `--max_depth` / `--seed` / `--shading_normals`.  Runs on libmatpbr.so (MI355X); see materialist_amd/pipeline.py."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Single-image inverse rendering on the matpbr HIP kernels")
    ap.add_argument("--img_inverse_path", type=str, required=True)
    ap.add_argument("--save_name", type=str, required=True)
    ap.add_argument("--opt_src", type=str, required=True, default="arm", help="'arm' subsets, or 'skip' to resume from best_results/")
    ap.add_argument("--opt_order", type=str, nargs="+", default=["arm"])
    ap.add_argument("--use_mask", action="store_true")
    ap.add_argument("--opt_env_from", type=int, default=0)
    ap.add_argument("--save_path", type=str, default=None)
    ap.add_argument("--model_name", type=str, default="pos_mlp", choices=["pos_mlp", "none"],
                    help="the reference parses and ignores this flag (it always runs pos_mlp, F4); here it is honoured, default pos_mlp")
    ap.add_argument("--size", type=int, default=512, help="render resolution (the reference hard-codes 512)")
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--num_epochs", type=int, default=5000)
    ap.add_argument("--pred_dir", type=str, default=None, help="directory with *Pred.exr/png initial maps (MaterialNet output layout)")
    ap.add_argument("--matnet_weights", type=str, default=None, help="matnet_weights.pth (Lez/MatNet on the HF hub) for the MaterialNet initial guess")
    ap.add_argument("--geometry", type=str, default="mesh", choices=["mesh", "depth"],
                    help="per-pixel geometric normals: from the reference's mesh of the depth map, gap closing at depth edges included (mesh_recon.py, "
                         "default), or central differences of the depth map itself")
    ap.add_argument("--integrator", choices=("sh", "path"), default="sh",
                    help="render the fit goes through: sh = the deterministic render (direct light, SH25, default); path = the path-traced "
                         "render of the depth mesh with its backward pass (shadows and inter-reflection, as the reference's Mitsuba `path`)")
    ap.add_argument("--max_depth", type=int, default=4, help="--integrator path: Mitsuba's max_depth (1 emission, 2 direct + shadows, 4 the reference's)")
    ap.add_argument("--seed", type=int, default=0, help="--integrator path: seed of the sequence each render draws its seed from")
    ap.add_argument("--shading_normals", choices=("face", "map"), default="face",
                    help="--integrator path: face = shade with the mesh's face normals (default); map = 'n' in --opt_order is accepted and the "
                         "path render shades with, and fits, the normal map")
    args = ap.parse_args(argv)
    if args.shading_normals == "map" and args.integrator != "path":
        ap.error("--shading_normals map needs --integrator path")
    if args.integrator == "path" and args.shading_normals == "face" and "n" in "".join(args.opt_order):
        ap.error(f"--integrator path shades with the mesh's face normals: it cannot optimise normals ('n' in --opt_order {' '.join(args.opt_order)})")
    if args.integrator == "path" and not 1 <= args.max_depth <= 16:
        ap.error("--max_depth must lie in 1..16")
    return args


def main(argv=None):
    args = parse_args(argv)
    from materialist_amd.pipeline import inverse_image

    res = inverse_image(args.img_inverse_path, args.save_name, args.opt_src, args.opt_order, args.use_mask, args.opt_env_from,
                        args.save_path, args.model_name, size=args.size, spp=args.spp, num_epochs=args.num_epochs, pred_dir=args.pred_dir,
                        matnet_weights=args.matnet_weights, geometry=args.geometry, integrator=args.integrator, max_depth=args.max_depth,
                        seed=args.seed, shading_normals=args.shading_normals)
    print(f"done: PSNR {res['psnr']:.2f} dB, best loss_mse {res['best_loss']:.6f}, outputs in {res['output_dir']}")


if __name__ == "__main__":
    main()
