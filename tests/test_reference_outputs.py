"""Weak pins on the sample outputs the reference ships (`output_imgs/{indoor,jinjya}/`, SURVEY.md section 8c "weak pins").

The pixels and file bytes they need are stored in tests/golden/reference_outputs.npz (tests/golden/gen_reference_outputs.py).  They check
  * the PIZ decoder of `materialist_amd.imageio_exr` against an independent encoding of the same picture: the 8-bit PNG panels
    the reference wrote from the same tensors (`opt_env_img.png` = [gt | Mitsuba render | envmap], gamma 2.2; `gt_image.png`), on a
    PIZ file made of one 32-line chunk of each shipped file (its bytes unchanged);
  * the build's render definition (DESIGN.md section 1, fp32 oracle) against **Mitsuba's own render** of the reference's optimised
    maps (`best_results/rendered_img.exr`), the only image-level evidence of `mi.render` available, on eight bands of rows spread over
    the image.  The residual (occlusion, inter-reflection, MC noise, stretched triangles at depth edges) is documented in DESIGN.md
    section 5; the threshold here only guards against convention regressions (camera, normals from depth, envmap -> SH, gamma).
"""
import os

import numpy as np
import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_outputs.npz")


@pytest.fixture(scope="module")
def ref():
    return np.load(FIXTURE)


def _gamma(x):
    return np.clip(x, 0, 1) ** (1 / 2.2)


def _psnr(a, b):
    return -10 * np.log10(np.mean((_gamma(a) - _gamma(b)) ** 2))


def _exr(ref, key, tmp_path):
    from materialist_amd.imageio_exr import read_exr

    path = tmp_path / f"{key}.exr"
    path.write_bytes(ref[key].tobytes())
    return read_exr(str(path))


@pytest.mark.parametrize("scene", ["indoor", "jinjya"])
def test_piz_decode_matches_the_png_panels(scene, ref, tmp_path):
    rows = int(ref["piz_rows"][1] - ref["piz_rows"][0])
    panel = ref[f"{scene}_panel_u8"].astype(np.float32) / 255
    rough = _exr(ref, f"{scene}_roughness_exr", tmp_path)
    assert rough.shape == (rows, 512, 1) and np.isfinite(rough).all()
    assert rough.min() == np.float32(0.07) and rough.max() == np.float32(1.0)      # the loop's clamp values, bit-exact (:420-423)
    if scene == "indoor":      # (jinjya's rendered_img.exr is not the render of its panel: 19.8 dB even after the best rescale)
        render = _exr(ref, f"{scene}_render_exr", tmp_path)
        assert np.mean((_gamma(render) - panel[:, 512:1024]) ** 2) < 10 ** (-3.3)   # > 33 dB: 8-bit quantisation + last-vs-best epoch
    gt = _exr(ref, f"{scene}_gt_exr", tmp_path)
    assert np.abs(_gamma(gt) - panel[:, :512]).max() < 1.5 / 255


def test_render_definition_against_mitsuba_render_of_the_reference_maps(ref):
    from materialist_amd import sh
    from oracle.oracle import Oracle

    o = Oracle(np.float32)
    H, W = (int(v) for v in ref["indoor_image_hw"])
    rows = ref["render_rows"]
    a, r, m = (ref[f"indoor_render_{k}"] for k in ("albedo", "roughness", "metallic"))
    mitsuba = ref["indoor_render_rendered_img"]
    depth = np.full((H, W), ref["indoor_depth_max"], np.float32)                    # rows no band reads: any value
    depth[ref["indoor_depth_row_index"]] = ref["indoor_depth_rows"]
    depth = 2 * ref["indoor_depth_max"] - depth                                      # inverse_img_w_mi.py:722
    n = o.normals_from_depth(depth)[rows]                                            # config.json: use_mesh_normal = true
    env = ref["indoor_envmap"]
    coef = (sh.envmap_to_sh_matrix(16, 32) @ env.reshape(512, 3).astype(np.float64)).astype(np.float32)
    img = np.empty_like(mitsuba)
    starts = [k for k in range(len(rows)) if k == 0 or rows[k] != rows[k - 1] + 1]
    for k0, k1 in zip(starts, starts[1:] + [len(rows)]):                             # each band with the full image's view directions
        sl = slice(k0, k1)
        img[sl] = o.shade_fwd_win(a[sl], r[sl], m[sl], n[sl], coef, 64, H, W, int(rows[k0]), 0)
    raw = _psnr(img, mitsuba)
    matched = _psnr(img * (mitsuba.mean() / img.mean()), mitsuba)                    # the BRDF loss is scale-free (:388-391)
    print(f"build render vs Mitsuba render, indoor ({len(rows)} rows): {raw:.2f} dB raw, {matched:.2f} dB mean-matched")
    assert raw > 20.5 and matched > 24.5
