#!/usr/bin/env python3
"""Command line of transparency editing, same flags as the reference's trans_edit.py (:62-70): the part of the scene inside
best_results/mask.png rendered as glass over best_results/bg.png.  See materialist_amd/relight.py (`render_trans`)."""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter, description="render a scene with transparency editing")
    ap.add_argument("--save_name", type=str, required=True, help="name of the scene's directory")
    ap.add_argument("--ior", type=float, default=1.2, help="index of refraction")
    ap.add_argument("--keep_albedo_color", action="store_true", help="keep the albedo inside the mask (default: 0.7)")
    ap.add_argument("--specTrans", type=float, default=0.4, help="specular transmission")
    ap.add_argument("--env_path", type=str, default=None, help="environment map (default: the scene's best_results/envmap.hdr)")
    ap.add_argument("--input_path", required=False, default=None, type=str)
    ap.add_argument("--save_path", required=False, default=None, type=str)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10, help="renders averaged (seeds seed, seed + 1, ...)")
    ap.add_argument("--max_depth", type=int, default=4, help="Mitsuba's max_depth")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--refract_distance", type=float, default=100.0, help="thickness scale of the glass in the background lookup")
    ap.add_argument("--denoise", choices=("off", "atrous"), default="off",
                    help="atrous = split every render into two halves of spp/2 and pass their mean through the variance-guided a-trous filter "
                         "(needs an even --spp); off = the plain average")
    a = ap.parse_args(argv)
    if not (a.ior > 0 and math.isfinite(a.ior)):
        ap.error("--ior must be positive")
    if not 0.0 <= a.specTrans <= 1.0:
        ap.error("--specTrans must lie in [0, 1]")
    if not (a.refract_distance >= 0 and math.isfinite(a.refract_distance)):
        ap.error("--refract_distance must be non-negative")
    if a.spp < 1 or a.iters < 1:
        ap.error("--spp and --iters must be at least 1")
    if a.denoise == "atrous" and a.spp % 2:
        ap.error("--denoise atrous splits every render into two halves of spp/2 samples: --spp must be even")
    if not 1 <= a.max_depth <= 16:
        ap.error("--max_depth must lie in 1..16")
    return a


def main(argv=None):
    a = parse_args(argv)
    from materialist_amd import relight

    print("Wrote file to", relight.render_trans(a.save_name, a.ior, a.keep_albedo_color, a.specTrans, a.env_path, a.input_path, a.save_path,
                                                a.spp, a.iters, a.max_depth, a.seed, a.refract_distance, denoise=a.denoise))


if __name__ == "__main__":
    main()
