"""Forward-only re-rendering of an optimised scene under new lighting: the `render_final.py` side of the reference
(`render_w_mi` :148-203, `render_real` :241-260, `rotate_envmap` :290-298, `render_rolling_envmap` :300-418).  SURVEY.md 8(f4).

The reference re-traces the scene for every light (10 x spp 64 + OptiX denoise, or spp 32 per rolling frame).  The
deterministic render is linear in the light, so the per-pixel transfer is computed once (`matpbr_shade_transfer`) and each
frame is a 75-term dot product per pixel (`matpbr_relight`, HBM-bound).  Rolling the envmap by whole texel columns is the
SH rotation about +y by the same angle (`sh.rotate_y_matrix`), so no envmap is ever re-projected or written to disk.
Material editing inside `best_results/mask.png` (`edit=` of `render_w_mi`, :143-181) is applied to the maps before the
transfer is computed.  Object insertion (`--mode oi`, :100-141,207-237,263-288) is `render_oi`: it always path traces.
`integrator="path"` renders instead with the path tracer (materialist_amd/pathtrace.py), the integrator the
reference's final images come from: the `.ply` mesh, shadows, inter-reflection, the envmap's texels as the light; rolling frames
roll the envmap's texel columns.  `denoise="atrous"` passes a path-traced image through the project's denoiser (DESIGN.md section 1.4,
"Denoiser"): every render of `spp` samples becomes two of `spp / 2` with independent seeds, and one variance-guided a-trous filter
runs over their sums, guided by the first-hit features and the albedo.  The default, "off", leaves every output as it was.
`relight_composite=True` (path only; DESIGN.md section 1.4, "Relighting in the photograph") writes the photograph under the new light
instead of a re-render of the fitted scene: the photograph times the model's radiance under the new envmap over its radiance under the
fitted one, both from one walk (`PathTracer.render_relight`, `composite_relight`).
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional

import numpy as np
import torch

from . import loss as _loss
from . import ops
from . import sh as _sh
from .imageio_exr import read_exr, write_exr
from .imageio_hdr import read_hdr
from .pipeline import OUT_DIR, load_image, write_png


def load_estimated_brdf(root_dir: str, device="cuda") -> Dict[str, torch.Tensor]:
    """myutils/mi_plugin.py:701-739: best_results/{albedo,roughness,metallic,normal}.exr (+ envmap.hdr, mask.png, bg.png); roughness
    is rescaled `r * 0.95 + 0.05` on reload (:716)."""
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)
    mat = {"albedo": t(read_exr(os.path.join(root_dir, "albedo.exr"))),
           "roughness": t(read_exr(os.path.join(root_dir, "roughness.exr"))[..., :1]) * 0.95 + 0.05,
           "metallic": t(read_exr(os.path.join(root_dir, "metallic.exr"))[..., :1]),
           "normal": t(read_exr(os.path.join(root_dir, "normal.exr")))}
    p = os.path.join(root_dir, "envmap.hdr")
    if os.path.exists(p):
        mat["envmap"] = t(read_hdr(p))
    p = os.path.join(root_dir, "mask.png")                            # "load mask for Material editing" (:729-733)
    if os.path.exists(p):
        from PIL import Image

        m = np.asarray(Image.open(p))
        mat["mask"] = torch.from_numpy(np.ascontiguousarray((m[..., 0] if m.ndim == 3 else m) > 0)).to(device)
    p = os.path.join(root_dir, "bg.png")                              # "load background for transparency editing" (:720-728)
    if os.path.exists(p):
        from PIL import Image

        im = Image.open(p)
        if im.mode not in ("RGB", "RGBA", "L"):
            im = im.convert("RGB")
        b = np.asarray(im).astype(np.float32) / 255.0                 # 8-bit values over 255, kept in the file's gamma space
        b = np.repeat(b[..., None], 3, -1) if b.ndim == 2 else b[..., :3]
        bg = t(b)
        H, W = mat["albedo"].shape[0], mat["albedo"].shape[1]
        if bg.shape[0] != H or bg.shape[1] != W:                      # (:723-726)
            bg = torch.nn.functional.interpolate(bg[None].permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=True)[0]
            bg = bg.permute(1, 2, 0).contiguous()
        mat["bg"] = bg
    return mat


def rgb_to_hsv(rgb: np.ndarray) -> np.ndarray:
    """[...,3] in [0,1] -> h, s, v in [0,1] (the convention of skimage.color.rgb2hsv the reference edits with, :143-146)."""
    rgb = np.asarray(rgb, dtype=np.float64)
    v = rgb.max(-1)
    delta = v - rgb.min(-1)
    s = np.where(v > 0, delta / np.where(v > 0, v, 1), 0.0)
    d = np.where(delta > 0, delta, 1.0)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    h = np.where(v == r, (g - b) / d, np.where(v == g, 2.0 + (b - r) / d, 4.0 + (r - g) / d))
    h = np.where(delta > 0, (h / 6.0) % 1.0, 0.0)
    return np.stack([h, s, v], -1)


def hsv_to_rgb(hsv: np.ndarray) -> np.ndarray:
    hsv = np.asarray(hsv, dtype=np.float64)
    h, s, v = hsv[..., 0], hsv[..., 1], hsv[..., 2]
    i = np.floor(h * 6.0)
    f = h * 6.0 - i
    p, q, t = v * (1 - s), v * (1 - f * s), v * (1 - (1 - f) * s)
    i = i.astype(np.int64) % 6
    r = np.choose(i, [v, q, p, p, t, v])
    g = np.choose(i, [t, v, v, q, p, p])
    b = np.choose(i, [p, p, t, v, v, q])
    return np.stack([r, g, b], -1)


def apply_edit(mat: Dict[str, torch.Tensor], edit: Optional[Dict[str, object]]) -> str:
    """render_final.py:143-181: inside the mask, shift the albedo in HSV (`edit['albedo']` = [dh, ds, dv], clipped to [0,1]) and/or
    overwrite roughness / metallic with a constant.  Returns the reference's file-name flag (`_r_0.2`, ...); the albedo flag carries
    the first shift component (the reference's own expression for it, `edit[key].tolist()[0,0]`, raises a TypeError)."""
    flag = ""
    for key in ("albedo", "roughness", "metallic"):
        val = (edit or {}).get(key)
        if val is None:
            continue
        if "mask" not in mat:
            raise FileNotFoundError("Unable to edit img, no mask found")
        mask = mat["mask"]
        if key == "albedo":
            shift = np.asarray(val, dtype=np.float64).reshape(-1)[:3]
            sel = mat[key][mask].cpu().numpy()
            out = hsv_to_rgb(np.clip(rgb_to_hsv(sel) + shift, 0, 1))
            mat[key][mask] = torch.from_numpy(out.astype(np.float32)).to(mat[key].device)
            flag += f"_a_{shift[0]}"
        else:
            mat[key][mask] = float(val)
            flag += f"_{key[:1]}_{val}"
    return flag


def find_envmap(save_name: str, env_path: Optional[str], input_path: Optional[str]) -> str:
    """render_final.py:243-259 / :304-321: explicit path, else <input_path>/<name>/best_results/envmap.hdr, else the default tree."""
    if env_path is not None:
        return env_path
    cands = []
    if input_path is not None:
        cands.append(os.path.join(input_path, save_name, "best_results", "envmap.hdr"))
    cands.append(os.path.join(OUT_DIR, save_name, "best_results", "envmap.hdr"))
    for c in cands:
        if os.path.exists(c):
            return c
    raise ValueError("No envmap found")


def envmap_to_light(env: np.ndarray) -> np.ndarray:
    He, We = env.shape[:2]
    return _sh.envmap_to_sh_matrix(He, We) @ env.reshape(He * We, 3).astype(np.float64)


class Relighter:
    """Transfer of one optimised scene; `frames(lights)` renders any number of lights."""

    def __init__(self, mat: Dict[str, torch.Tensor], shading_normal: torch.Tensor, spp: int = 64, fov_x_deg: float = 35.0,
                 mesh_mask: Optional[torch.Tensor] = None):
        self.H, self.W = mat["albedo"].shape[0], mat["albedo"].shape[1]
        self.T = ops.shade_transfer(mat["albedo"].contiguous(), mat["roughness"].contiguous(), mat["metallic"].contiguous(),
                                    shading_normal.contiguous(), spp, fov_x_deg)
        self.bg = None
        if mesh_mask is not None and bool(mesh_mask.any()):        # pixels without geometry show the environment (mesh_mask.png)
            from .render import Scene

            sc = Scene(self.H, self.W, self.T.device, fov_x_deg=fov_x_deg)
            sc.set_mesh_mask(mesh_mask)
            self.bg = (sc.bg_mask, sc.bg_basis)

    def frames(self, lights) -> torch.Tensor:
        L = torch.as_tensor(np.asarray(lights, dtype=np.float32)).reshape(-1, 25, 3).to(self.T.device)
        out = ops.relight(self.T, L, self.H, self.W)
        if self.bg is not None:
            mask, basis = self.bg
            bg = torch.einsum("pk,fkc->fpc", basis, L).reshape(-1, self.H, self.W, 3)
            out = torch.where(mask[None, :, :, None], bg, out)
        return out


def _mesh_mask(scene_dir: str) -> Optional[torch.Tensor]:
    p = os.path.join(scene_dir, "mesh_mask.png")
    if not os.path.exists(p):
        return None
    from PIL import Image

    mk = np.asarray(Image.open(p))
    return torch.from_numpy(np.ascontiguousarray((mk[..., 0] if mk.ndim == 3 else mk) > 0))


def _scene_normal(scene_dir: str, mat: Dict[str, torch.Tensor], save_name: str, device) -> torch.Tensor:
    if "mn" in save_name:                                            # 'mn' in the name = optimised normals (:155-160)
        return mat["normal"]
    depth = read_exr(os.path.join(scene_dir, "depthPred.exr"))[..., 0]
    depth = 2 * depth.max() - depth                                  # inverse_img_w_mi.py:722
    return ops.normals_from_depth(torch.from_numpy(np.ascontiguousarray(depth, dtype=np.float32)).to(device))


def _path_tracer(scene_dir: str, save_name: str, mat: Dict[str, torch.Tensor], device, objects=None, **movable):
    """PathTracer on the scene's `<save_name>.ply`; without one, the mesh the pipeline would write (depthPred.exr -> 2 max - d,
    mesh_mask.png pixels removed, mesh.reference_mesh: inverse_img_w_mi.py:721-727).  `objects`: PathTracer's inserted meshes;
    `movable`: its `movable` and `reach`."""
    from . import mesh as _mesh
    from .pathtrace import PathTracer
    from .render import DEFAULT_FOV

    H, W = mat["albedo"].shape[0], mat["albedo"].shape[1]
    ply = os.path.join(scene_dir, f"{save_name}.ply")
    if os.path.exists(ply):
        V, T = _mesh.read_ply(ply)
    else:
        depth = read_exr(os.path.join(scene_dir, "depthPred.exr"))[..., 0]
        depth = np.array(2 * depth.max() - depth, dtype=np.float32)
        mm = _mesh_mask(scene_dir)
        if mm is not None:
            depth[mm.numpy()] = 0.0
        rm = _mesh.reference_mesh(depth, DEFAULT_FOV)
        V, T = rm["vertices"], rm["triangles"]
    return PathTracer(V, T, H, W, DEFAULT_FOV, device=device, objects=objects, **movable)


def edit_mask(fitted, edited) -> torch.Tensor:
    """bool [H,W]: the texels where the edited maps (a_e, r_e, m_e) differ from the fitted ones (a, r, m) in the bits of any of their five
    floats: the mask `PathTracer.render_edit_diff` derives when it is given none (`pathtrace.edit_mask`)."""
    from .pathtrace import edit_mask as _edit_mask

    return _edit_mask(fitted, edited)


def _check_integrator(integrator: str, shading_normals: str = "face") -> None:
    if integrator not in ("sh", "path"):
        raise ValueError(f"integrator must be 'sh' or 'path', got {integrator!r}")
    if shading_normals not in ("face", "map"):
        raise ValueError(f"shading_normals must be 'face' or 'map', got {shading_normals!r}")
    if shading_normals == "map" and integrator != "path":
        raise ValueError("shading_normals='map' needs integrator='path' (the 'sh' render takes its normals by the scene's name)")


def _check_denoise(denoise: str, integrator: str, spp: int) -> bool:
    """True when the a-trous denoiser is asked for and can run; ValueError when it cannot."""
    if denoise not in ("off", "atrous"):
        raise ValueError(f"denoise must be 'off' or 'atrous', got {denoise!r}")
    if denoise == "off":
        return False
    if integrator != "path":
        raise ValueError("denoise='atrous' needs integrator='path': the 'sh' render is deterministic quadrature and has no noise to filter")
    if spp < 2 or spp % 2:
        raise ValueError(f"denoise='atrous' splits every render into two halves of spp / 2 samples: spp must be even, got {spp}")
    return True


def _scaled_env(env: np.ndarray, env_scale: float, integrator: str = "path") -> np.ndarray:
    """The envmap times `env_scale`, before its sampling tables are built (1: the array itself, so the same bits; 0: an envmap of
    zero luminance, which has no tables: with an area light, the night shot).  The 'sh' render does not take it."""
    s = float(env_scale)
    if not (np.isfinite(s) and s >= 0):
        raise ValueError(f"env_scale must be finite and >= 0, got {env_scale}")
    if s == 1.0:
        return env
    if integrator != "path":
        raise ValueError("env_scale needs integrator='path' (or render_oi): the 'sh' render projects the envmap as it is")
    return np.asarray(env, dtype=np.float32) * np.float32(s)


_PBR_ALBEDO = 0.8   # pathtrace.PBR_DEFAULTS["albedo"]: what `object_bsdf` gives a "pbr" dict without one


def albedo_guide(geom: torch.Tensor, albedo: torch.Tensor, bsdfs=(), colors: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The denoiser's albedo guide [H,W,3] from the features' ids: the albedo map as rendered where the camera ray hits the depth mesh
    (id 0), a diffuse object's reflectance, a PBR object's albedo, 1 on glass, on rough glass ("roughdielectric": colourless, like
    glass) and on an area light (the fall-through: a light's pixels are its radiance, which the colour term guides alone), 0 where it
    hits nothing.  `bsdfs`: the inserted objects' BSDFs, in order.  `colors` [H,W,3]: `PathTracer.feature_colors()` of a tracer with
    vertex-coloured objects, or `PathTracer.feature_tints()` of one with textured objects; a diffuse or pbr object's constant is
    multiplied by it, so that the guide follows a colour edge inside the object (it is 1 off the coloured and textured objects)."""
    ids = geom[..., 7]
    guide = albedo.to(geom.device, torch.float32).reshape(geom.shape[0], geom.shape[1], 3).clone()
    guide[ids < 0] = 0.0
    for k, b in enumerate(bsdfs):
        value = b["reflectance"] if b["type"] == "diffuse" else b.get("albedo", _PBR_ALBEDO) if b["type"] == "pbr" else (1.0, 1.0, 1.0)
        guide[ids == 1 + k] = torch.tensor([float(x) for x in np.broadcast_to(np.asarray(value, np.float64), (3,))], device=geom.device)
        if colors is not None and b["type"] in ("diffuse", "pbr"):
            guide[ids == 1 + k] *= colors.to(geom.device, torch.float32)[ids == 1 + k]
    return guide


def _denoised(pt, render_half, iters: int, seed: int, geom: torch.Tensor, guide: torch.Tensor) -> torch.Tensor:
    """`iters` pairs of half renders, `render_half(seed)` with seeds seed + 2 i (summed into A) and seed + 2 i + 1 (into B), then one
    filter over the two means."""
    A = torch.zeros_like(guide)
    B = torch.zeros_like(guide)
    for i in range(iters):
        A += render_half(seed + 2 * i)
        B += render_half(seed + 2 * i + 1)
    if iters > 1:
        A /= iters
        B /= iters
    return pt.denoise(A, B, guide, geom)


def _check_relight_composite(integrator: str, edit: Optional[Dict[str, object]], edit_composite: bool, floor: Optional[float]) -> None:
    """ValueError for what relighting in the photograph does not do, before any GPU work."""
    if integrator != "path":
        raise ValueError("relight_composite needs integrator='path': the walk under two envmaps is the path tracer's (the 'sh' render has "
                         "no shadows to transfer)")
    if edit_composite:
        raise ValueError("relight_composite knows no edit composite: one picture takes one transfer, the edit's difference or the light's ratio")
    if any((edit or {}).get(key) is not None for key in ("albedo", "roughness", "metallic")):
        raise ValueError("relight_composite knows no material edit: the photograph shows the materials as they are, and the ratio of two "
                         "lights over edited maps would not put the edit into it")
    if floor is not None and not (np.isfinite(floor) and floor > 0):
        raise ValueError(f"relight_floor must be finite and > 0, got {floor}")


def _relit_photo(pt, mat: Dict[str, torch.Tensor], env_a, tabs_a, env_b, nrm, spp: int, max_depth: int, seed: int, guides, photo: torch.Tensor,
                 floor: Optional[float]) -> torch.Tensor:
    """The photograph under `env_b`: `PathTracer.render_relight` of the fitted maps under the fitted envmap `env_a` and under `env_b`, and
    `composite_relight`.  `guides`: None, or the a-trous filter's (geom, albedo guide): then two walks of spp / 2, seeds `seed` and
    `seed + 1`, and the two radiances pass `PathTracer.denoise` one after the other with the same guides before the composite."""
    from .pathtrace import composite_relight

    maps = (mat["albedo"], mat["roughness"], mat["metallic"])
    tabs_b = pt.tables(env_b)
    if guides is None:
        base, relit = pt.render_relight(*maps, env_a, env_b, spp, max_depth, seed, tables=tabs_a, new_tables=tabs_b, normal=nrm)
    else:
        halves = [pt.render_relight(*maps, env_a, env_b, spp // 2, max_depth, seed + k, tables=tabs_a, new_tables=tabs_b, normal=nrm) for k in (0, 1)]
        base, relit = (pt.denoise(halves[0][k], halves[1][k], guides[1], guides[0]) for k in (0, 1))
    return composite_relight(base, relit, photo, floor=floor)


def render_real(save_name: str, env_path: Optional[str] = None, input_path: Optional[str] = None, save_path: Optional[str] = None,
                spp: int = 64, device="cuda", edit: Optional[Dict[str, object]] = None, integrator: str = "sh", max_depth: int = 4,
                seed: int = 0, shading_normals: str = "face", denoise: str = "off", env_scale: float = 1.0, composite: bool = False,
                photo_path: Optional[str] = None, transfer: str = "additive", relight_composite: bool = False,
                relight_photo: Optional[str] = None, relight_floor: Optional[float] = None) -> str:
    """render_final.py:148-203,241-260: one re-render under `env_path` -> mi_<name>_<env>_<edit flag>.exr / .png.
    integrator "sh": the deterministic render (SH25 light, direct, unshadowed); "path": the path tracer, `max_depth` / `seed`, shading
    with the mesh's face normals or, with `shading_normals="map"`, with best_results/normal.exr whatever the scene is called.
    `denoise="atrous"` (path only, even `spp`): two renders of spp / 2, seeds `seed` and `seed + 1`, through the a-trous filter.
    `env_scale` (path only): the envmap is multiplied by it before its tables are built; 1 gives the same bits as without it.
    `composite=True` ("Material edits in the photograph"; path only, with an edit, env_scale 1, denoise "off"):
    the photograph (`photo_path`, default <scene>/gt_image.exr, as `render_oi` reads it) with what the edit changes, not a re-render of
    the fitted scene: pixels no edited texel reaches keep the photograph's bits -> mi_ec_<name>_<env>_<edit flag>.exr / .png.
    `transfer`: "additive" adds the model's difference; "ratio" dims the photograph, per channel, by the share of light the model
    loses where the edit darkens it, so that the fit's albedo cancels.
    `relight_composite=True` ("Relighting in the photograph"; path only, no edit, not with `composite`): the
    photograph (`relight_photo`, default <scene>/gt_image.exr) under the new light: environment A is the fitted best_results/envmap.hdr,
    B is `env_path` times `env_scale`, and the picture is the photograph times the model's radiance under B over that under A, both from
    one walk -> mi_rc_<name>_<env>_.exr / .png.  Without an `env_path` and with `env_scale` 1 B is A and the picture the photograph: a
    ValueError.  `relight_floor` > 0: `composite_relight`'s floor (default: 0.01 x the frame's mean radiance under A).  With
    `denoise="atrous"`: two walks of spp / 2, seeds `seed` and `seed + 1`, and both radiances pass the a-trous filter before the ratio."""
    _check_integrator(integrator, shading_normals)
    _scaled_env(np.zeros(0, np.float32), env_scale, integrator)
    atrous = _check_denoise(denoise, integrator, spp)
    scene_dir = os.path.join(input_path if input_path is not None else OUT_DIR, save_name)
    if transfer not in ("additive", "ratio"):
        raise ValueError(f"transfer must be 'additive' or 'ratio', got {transfer!r}")
    if not composite and (photo_path is not None or transfer != "additive"):
        raise ValueError("photo_path and transfer need composite=True")
    if not relight_composite and (relight_photo is not None or relight_floor is not None):
        raise ValueError("relight_photo and relight_floor need relight_composite=True")
    if relight_composite:
        _check_relight_composite(integrator, edit, composite, relight_floor)
        if env_path is None and float(env_scale) == 1.0:
            raise ValueError("relight_composite needs a new light, an env_path or an env_scale other than 1: under the fitted envmap the "
                             "picture is the photograph")
        photo = _oi_photo(scene_dir, relight_photo, False, 1.0)
        fitted_env_path = find_envmap(save_name, None, input_path)
    if composite:
        if integrator != "path":
            raise ValueError("composite needs integrator='path': the differential render of edited maps is the path tracer's")
        if not any((edit or {}).get(key) is not None for key in ("albedo", "roughness", "metallic")):
            raise ValueError("composite needs an edit (albedo, roughness or metallic): without one the picture is the photograph")
        photo = _oi_photo(scene_dir, photo_path, atrous, env_scale)
    env_path = find_envmap(save_name, env_path, input_path)
    mat = load_estimated_brdf(os.path.join(scene_dir, "best_results"), device)
    fitted = tuple(mat[key].clone() for key in ("albedo", "roughness", "metallic")) if composite else None
    edit_flag = apply_edit(mat, edit)
    if composite:
        from .pathtrace import composite_edit

        delta, fit, _ = _path_tracer(scene_dir, save_name, mat, device).render_edit_diff(
            *fitted, load_image(env_path), (mat["albedo"], mat["roughness"], mat["metallic"]), None, spp, max_depth, seed,
            normal=mat["normal"] if shading_normals == "map" else None)
        img = composite_edit(delta, torch.from_numpy(photo).to(delta.device), fit if transfer == "ratio" else None)
    elif relight_composite:
        pt = _path_tracer(scene_dir, save_name, mat, device)
        nrm = mat["normal"] if shading_normals == "map" else None
        env_a = load_image(fitted_env_path)
        geom = pt.features(normal=nrm) if atrous else None
        img = _relit_photo(pt, mat, env_a, pt.tables(env_a), _scaled_env(load_image(env_path), env_scale), nrm, spp, max_depth, seed,
                           (geom, albedo_guide(geom, mat["albedo"])) if atrous else None, torch.from_numpy(photo).to(pt.device), relight_floor)
    elif atrous:
        pt = _path_tracer(scene_dir, save_name, mat, device)
        nrm = mat["normal"] if shading_normals == "map" else None
        env = _scaled_env(load_image(env_path), env_scale)
        tabs = pt.tables(env)
        geom = pt.features(normal=nrm)
        half = lambda sd: pt.render(mat["albedo"], mat["roughness"], mat["metallic"], env, spp // 2, max_depth, sd, tables=tabs, normal=nrm)
        img = _denoised(pt, half, 1, seed, geom, albedo_guide(geom, mat["albedo"]))
    elif integrator == "path":
        img = _path_tracer(scene_dir, save_name, mat, device).render(mat["albedo"], mat["roughness"], mat["metallic"],
                                                                     _scaled_env(load_image(env_path), env_scale), spp, max_depth, seed,
                                                                     normal=mat["normal"] if shading_normals == "map" else None)
    else:
        rl = Relighter(mat, _scene_normal(scene_dir, mat, save_name, device), spp, mesh_mask=_mesh_mask(scene_dir))
        img = rl.frames(envmap_to_light(load_image(env_path))[None])[0]
    env_id = os.path.basename(env_path)[:-4]
    out_dir = os.path.join(save_path if save_path else OUT_DIR, save_name)
    os.makedirs(out_dir, exist_ok=True)
    base = os.path.join(out_dir, f"mi_{'ec_' if composite else 'rc_' if relight_composite else ''}{save_name}_{env_id}_{edit_flag}")   # (:199-202)
    write_exr(base + ".exr", img.cpu().numpy())
    write_png(base + ".png", _loss.linear_to_srgb(img.clamp_min(0)).cpu().numpy())
    return base + ".png"


# Mitsuba's named indices of refraction for the reference's inserted glass (render_final.py:126): "acrylic glass" and "air"
OI_INT_IOR, OI_EXT_IOR = 1.49, 1.000277
OI_REFLECTANCE = 0.8                                  # the second inserted mesh: diffuse, reflectance 0.8 (render_final.py:131)


def find_envmap_oi(save_name: str, env_path: Optional[str], input_path: Optional[str]) -> str:
    """render_final.py:263-287: explicit path, else best_results/envmap_opt.hdr before best_results/envmap.hdr, the input tree before
    the default tree."""
    if env_path is not None:
        return env_path
    roots = ([os.path.join(input_path, save_name)] if input_path is not None else []) + [os.path.join(OUT_DIR, save_name)]
    for root in roots:
        for name in ("envmap_opt.hdr", "envmap.hdr"):
            c = os.path.join(root, "best_results", name)
            if os.path.exists(c):
                return c
    raise ValueError("No envmap found")


OI_SCENE_MAX_OBJECTS = 8                              # pathtrace.MAX_OBJECTS


def load_oi_scene(path: str) -> List[dict]:
    """An object list file for `render_oi(objects_file=...)`: JSON that holds only settings,
    {"objects": [{"ply": "chrome_ball.ply", "bsdf": {"type": "pbr", "albedo": [0.95, 0.93, 0.88], "roughness": 0.1, "metallic": 1.0},
    "normals": "vertex", "colors": "vertex"}, ...]}, at most 8 objects.  "ply" is relative to the file; "bsdf" is any of PathTracer's five types
    (dielectric, diffuse, pbr, roughdielectric: {"type": "roughdielectric", "int_ior", "ext_ior", "alpha"} is frosted glass, area:
    {"type": "area", "radiance": [r, g, b]} is a lamp, which takes "normals": "flat" only); "normals" is "flat" (default) or "vertex" (the file's normals if it has them, else
    `mesh.angle_weighted_normals`); "colors" (a diffuse or pbr object only) is "none" (default), "vertex" (the file's `red green blue`,
    display values, decoded to linear as `loss.srgb_to_linear` decodes) or "vertex_linear" (the file's values as written, what Mitsuba's
    `mesh_attribute` does; DESIGN.md section 1.4, "Vertex-coloured inserted objects"); "texture": "wood.png" (a diffuse or pbr object
    only) and "orm_texture": "wood_orm.png" (a pbr object only) name images relative to the file, read over the ply's per-vertex texture
    coordinates ("Textured inserted objects"); "transform": {"scale": 1, "rotate": {"axis": [x, y, z], "deg": a}, "translate": [x, y, z], "pivot": [x, y, z]} places the mesh
    (every part optional, the pivot by default the centre of its bounding box) and "motion": {"spin": {"axis": [x, y, z],
    "deg_per_frame": a}, "slide": [dx, dy, dz]} moves it from frame to frame of `render_oi(frames=N)` (`oi_pose`; DESIGN.md section 1.4,
    "Moving inserted objects"); "medium" (a dielectric or roughdielectric object only) fills the glass with a homogeneous medium
    ("Media inside glass"): {"sigma_a": [r, g, b], "scatter": sigma_s, "g": g}, the coefficients per scene unit, or
    {"color": [r, g, b], "at": d, "scatter", "g"}, the colour in (0, 1] white light has after the distance d > 0 inside the object
    (sigma_a = -ln(color) / d); it travels in the entry's "bsdf" as PathTracer takes it; "photo": true or false (a diffuse, pbr or
    roughdielectric object only; DESIGN.md section 1.4, "Reflected in inserted objects") says whether `render_oi(reflect_photo=True)`
    shows the photograph in what the object reflects (without the key the option decides)
    -> [{"ply": absolute path, "bsdf", "normals", "colors", "texture": absolute path or None, "orm_texture", "transform": the dict or
    None, "motion", "photo": the bool or None}], nothing read yet but the list.  ValueError naming
    the file and the entry: unknown key, missing ply, bad bsdf, too many objects."""
    import json

    from .pathtrace import object_bsdf, object_medium, object_photo

    try:
        with open(path) as f:
            doc = json.load(f)
    except (OSError, ValueError) as e:
        raise ValueError(f"{path}: cannot read the object list: {e}") from None
    if not isinstance(doc, dict) or not isinstance(doc.get("objects"), list):
        raise ValueError(f'{path}: the object list must be {{"objects": [...]}}')
    extra = sorted(set(doc) - {"objects"})
    if extra:
        raise ValueError(f"{path}: unknown key {extra[0]!r} (known: 'objects')")
    if not doc["objects"]:
        raise ValueError(f"{path}: the object list is empty")
    if len(doc["objects"]) > OI_SCENE_MAX_OBJECTS:
        raise ValueError(f"{path}: at most {OI_SCENE_MAX_OBJECTS} objects, got {len(doc['objects'])}")
    out = []
    for k, ob in enumerate(doc["objects"]):
        where = f"{path}: objects[{k}]"
        if not isinstance(ob, dict):
            raise ValueError(f"{where} must be an object with 'ply' and 'bsdf'")
        extra = sorted(set(ob) - {"ply", "bsdf", "normals", "colors", "texture", "orm_texture", "transform", "motion", "medium", "photo"})
        if extra:
            raise ValueError(f"{where}: unknown key {extra[0]!r} (known: 'ply', 'bsdf', 'normals', 'colors', 'texture', 'orm_texture', 'transform', "
                             f"'motion', 'medium', 'photo')")
        if not isinstance(ob.get("ply"), str) or not ob["ply"]:
            raise ValueError(f"{where}: 'ply' must name a mesh file")
        ply = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(path)), ob["ply"]))
        if not os.path.isfile(ply):
            raise ValueError(f"{where}: no such ply: {ply}")
        try:
            object_bsdf(ob.get("bsdf"))
        except (ValueError, TypeError) as e:
            raise ValueError(f"{where}: bad bsdf: {e}") from None
        bsdf = ob["bsdf"]
        if ob.get("medium") is not None:
            if "medium" in bsdf:
                raise ValueError(f"{where}: 'medium' is given twice, as the entry's key and inside its 'bsdf'")
            bsdf = dict(bsdf, medium=ob["medium"])
            try:
                object_medium(bsdf)
            except (ValueError, TypeError) as e:
                raise ValueError(f"{where}: bad medium: {e}") from None
        if "photo" in ob:
            try:
                if ob["photo"] is None:
                    raise ValueError("photo must be true or false, got None")
                object_photo({"bsdf": bsdf, "photo": ob["photo"]})
            except (ValueError, TypeError) as e:
                raise ValueError(f"{where}: bad photo: {e}") from None
        normals = ob.get("normals", "flat")
        if normals not in ("flat", "vertex"):
            raise ValueError(f"{where}: 'normals' must be 'flat' or 'vertex', got {normals!r}")
        if normals == "vertex" and ob["bsdf"].get("type") == "area":
            raise ValueError(f"{where}: 'normals' must be 'flat' for an area light: it emits from its faces")
        colors = ob.get("colors", "none")
        if colors not in OI_COLORS:
            raise ValueError(f"{where}: 'colors' must be 'none', 'vertex' or 'vertex_linear', got {colors!r}")
        if colors != "none" and ob["bsdf"].get("type") not in ("diffuse", "pbr"):
            raise ValueError(f"{where}: 'colors' must be 'none' for a {ob['bsdf'].get('type')!r} object: vertex colours tint a 'diffuse' or a 'pbr' one")
        images = {}
        for key, kinds in (("texture", ("diffuse", "pbr")), ("orm_texture", ("pbr",))):
            images[key] = None
            if ob.get(key) is None:
                continue
            if not isinstance(ob[key], str) or not ob[key]:
                raise ValueError(f"{where}: {key!r} must name an image file")
            if ob["bsdf"].get("type") not in kinds:
                raise ValueError(f"{where}: {key!r} belongs to a {' or a '.join(repr(x) for x in kinds)} object, not to a {ob['bsdf'].get('type')!r} one")
            images[key] = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(path)), ob[key]))
            if not os.path.isfile(images[key]):
                raise ValueError(f"{where}: no such {key}: {images[key]}")
        transform, motion = ob.get("transform"), ob.get("motion")
        try:
            oi_pose(transform, motion, 1)
        except ValueError as e:
            raise ValueError(f"{where}: {e}") from None
        out.append({"ply": ply, "bsdf": bsdf, "normals": normals, "colors": colors, **images, "transform": transform, "motion": motion,
                    "photo": ob.get("photo")})
    return out


def oi_pose(transform: Optional[dict], motion: Optional[dict], frame: int, pivot=None) -> tuple:
    """An object list entry's pose at frame `frame` -> `pathtrace.similarity`'s (R, s, t, c) in float64.  "transform": {"scale",
    "rotate": {"axis", "deg"}, "translate", "pivot"} places the object (every part optional; the pivot by default `pivot`, the centre of
    the mesh's bounding box); "motion": {"spin": {"axis", "deg_per_frame"}, "slide": [dx, dy, dz]} turns and slides it per frame: the
    rotation is spin(frame deg_per_frame) o rotate, the translation translate + frame slide, about the same pivot.  ValueError for an
    unknown sub-key, a zero axis, a scale that is not positive or a value that is not finite."""
    from .pathtrace import rotation, similarity

    if transform is not None and not isinstance(transform, dict):
        raise ValueError(f"'transform' must be an object with keys of 'scale', 'rotate', 'translate', 'pivot', got {transform!r}")
    if transform is not None and not isinstance(transform.get("rotate", {}), dict):
        raise ValueError(f"'transform': 'rotate' must be {{\"axis\": [x, y, z], \"deg\": a}}, got {transform['rotate']!r}")
    R, s, t, c = similarity(transform, pivot)
    if motion is None:
        return R, s, t, c
    if not isinstance(motion, dict):
        raise ValueError(f"'motion' must be an object with keys of 'spin', 'slide', got {motion!r}")
    extra = sorted(set(motion) - {"spin", "slide"})
    if extra:
        raise ValueError(f"'motion': unknown key {extra[0]!r} (known: 'spin', 'slide')")
    spin = motion.get("spin")
    if spin is not None:
        if not isinstance(spin, dict) or set(spin) != {"axis", "deg_per_frame"}:
            raise ValueError(f"'motion': 'spin' must be {{\"axis\": [x, y, z], \"deg_per_frame\": a}}, got {spin!r}")
        try:
            R = rotation(spin["axis"], frame * float(spin["deg_per_frame"])) @ R
        except TypeError:
            raise ValueError(f"'motion': 'spin' needs a number of degrees per frame, got {spin['deg_per_frame']!r}") from None
    if motion.get("slide") is not None:
        try:
            slide = np.array(motion["slide"], dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"'motion': 'slide' must be 3 numbers, got {motion['slide']!r}") from None
        if slide.shape != (3,) or not np.isfinite(slide).all():
            raise ValueError(f"'motion': 'slide' must be 3 finite numbers, got {motion['slide']!r}")
        t = t + frame * slide
    return R, s, t, c


def _oi_moves(motion: Optional[dict]) -> bool:
    """Whether an entry's "motion" changes its pose from frame to frame."""
    if not motion:
        return False
    spin, slide = motion.get("spin"), motion.get("slide")
    return bool(spin is not None and float(spin["deg_per_frame"]) != 0.0) or bool(slide is not None and np.any(np.asarray(slide, np.float64) != 0))


OI_COLORS = ("none", "vertex", "vertex_linear")
OI_SHADOWS = ("additive", "ratio")   # render_oi's `shadows`: how the differential composite transfers what the objects darken


def _object_colors(path: str, C: Optional[np.ndarray], colors: str) -> np.ndarray:
    """The vertex colours `mesh.read_ply_any` found in `path`, as linear RGB: "vertex" decodes them as display values, "vertex_linear"
    takes them as written.  ValueError naming the file when it has none."""
    if C is None:
        raise ValueError(f"{path}: colors={colors!r} needs vertex colours ('red green blue' or 'r g b' properties), the file has none")
    return np.clip(C, 0.0, 1.0) ** 2.2 if colors == "vertex" else C


def _object_image(path: str, decode: bool) -> np.ndarray:
    """An inserted object's image as linear values [h,w,3] float64 in [0, 1], row 0 the top row.  An integer image (a PNG) is divided
    by its type's maximum and, with `decode` (a base colour: display values), decoded with the project's 2.2 power; an orm image is
    never decoded.  `.exr` / `.hdr` are taken as written and must lie in [0, 1].  ValueError naming the file."""
    try:
        img = np.asarray(load_image(path))
    except Exception as e:
        raise ValueError(f"{path}: cannot read the image: {e}") from None
    if img.ndim == 2:
        img = np.repeat(img[..., None], 3, -1)
    if img.ndim != 3 or img.shape[2] < 3:
        raise ValueError(f"{path}: an image of three channels is needed, got an array of shape {img.shape}")
    img = img[..., :3]
    if img.dtype.kind in "iu":
        out = img.astype(np.float64) / float(np.iinfo(img.dtype).max)
        return out ** 2.2 if decode else out
    out = img.astype(np.float64)
    if not (np.isfinite(out).all() and out.min() >= 0.0 and out.max() <= 1.0):
        raise ValueError(f"{path}: a floating-point texture is taken as written and must be finite and lie in [0, 1]")
    return out


def _object_uv(path: str, Uv: Optional[np.ndarray]) -> np.ndarray:
    """The per-vertex texture coordinates `mesh.read_ply_any` found in `path`; ValueError naming the file when it has none."""
    if Uv is None:
        raise ValueError(f"{path}: a texture needs per-vertex texture coordinates ('s t', 'u v' or 'texture_u texture_v' properties), "
                         f"the file has none")
    return Uv


def _oi_photo(scene_dir: str, photo_path: Optional[str], atrous: bool, env_scale: float) -> np.ndarray:
    """The photograph `render_oi(composite=True)` composites into, linear float32 [H,W,3] of the maps' size; ValueError for what the
    composite does not do or cannot read, before any GPU work."""
    if atrous:
        raise ValueError("composite knows no denoise='atrous': the filter takes a radiance image, and the composite adds a signed difference "
                         "(composite_denoise=True runs the differential render's own filter)")
    if float(env_scale) != 1.0:
        raise ValueError(f"composite needs env_scale 1, got {env_scale}: the photograph was taken under the envmap as it is and is not dimmed")
    path = photo_path if photo_path is not None else os.path.join(scene_dir, "gt_image.exr")
    if not os.path.exists(path):
        raise ValueError(f"composite needs the photograph: {path} does not exist (photo_path, or the gt_image.exr the pipeline writes)")
    try:
        img = np.asarray(load_image(path))
    except Exception as e:
        raise ValueError(f"{path}: cannot read the photograph: {e}") from None
    if img.dtype.kind in "iu":
        img = img.astype(np.float32) / float(np.iinfo(img.dtype).max)
    img = np.asarray(img, dtype=np.float32)
    if not path.endswith((".exr", ".hdr")):                                  # display values, as the pipeline reads its input
        img = _loss.srgb_to_linear(torch.from_numpy(np.ascontiguousarray(img))).numpy()
    H, W = read_exr(os.path.join(scene_dir, "best_results", "albedo.exr")).shape[:2]
    if img.ndim != 3 or img.shape[2] < 3 or img.shape[:2] != (H, W):
        raise ValueError(f"{path}: the photograph must be [{H},{W},3], the maps' size, got an array of shape {img.shape}")
    img = np.ascontiguousarray(img[..., :3], dtype=np.float32)
    if not (np.isfinite(img).all() and (img >= 0).all()):
        raise ValueError(f"{path}: the photograph must be finite and >= 0")
    return img


def render_oi(save_name: str, env_path: Optional[str] = None, input_path: Optional[str] = None, save_path: Optional[str] = None,
              spp: int = 64, n_iter: int = 10, max_depth: int = 16, seed: int = 0, device="cuda", object_normals: str = "flat",
              denoise: str = "off", objects_file: Optional[str] = None, env_scale: float = 1.0, object_colors: str = "none",
              object_texture: Optional[str] = None, composite: bool = False, photo_path: Optional[str] = None,
              composite_denoise: bool = False, see_through: bool = False, shadows: str = "additive", frames: int = 1, tint=None,
              tint_at: Optional[float] = None, reflect_photo: bool = False):
    """render_final.py:100-141,207-237,263-288: the scene with `<scene_dir>/oi.ply` inserted as acrylic glass (smooth dielectric,
    1.49 / 1.000277) and `<scene_dir>/oi2.ply` as a diffuse object of reflectance 0.8, path traced with `max_depth` 16 ->
    mi_oi_<name>_<env>.exr / .png.  Either mesh may be missing (the reference needs both); both missing is a FileNotFoundError.
    The meshes are in the renderer's frame, read by `mesh.read_ply_any`.  `object_normals`: "flat" (default) shades them with their
    face normals; "vertex" shades each smooth, with its file's vertex normals where it has them, else with
    `mesh.angle_weighted_normals` ("Smooth inserted objects").  `n_iter` renders with seeds seed + i are
    averaged.  The reference renders spp 32 x 10 and denoises each with OptiX, which stays out: by default the
    samples do the denoiser's work (spp 64 x 10).  `denoise="atrous"` (even `spp`) runs the project's own filter instead: each of
    the `n_iter` renders becomes two of spp / 2, seeds seed + 2 i and seed + 2 i + 1, summed into two half buffers, and one a-trous
    pass runs over them ("Denoiser"); behind glass only its colour term guides.  `objects_file`: an object
    list (`load_oi_scene`) whose meshes are inserted instead, each with its own BSDF (dielectric, diffuse, pbr, roughdielectric: frosted glass, or area: a lamp) and
    its own normals; with it oi.ply and oi2.ply are not looked for and `object_normals` is ignored.  The output names are the same.
    `env_scale`: the envmap is multiplied by it before its tables are built (1: the same bits as without it; 0 with an area light in
    the list: the night shot, lit by the lamp alone).  `object_colors`: "none" (default), "vertex" or "vertex_linear" (`load_oi_scene`'s
    "colors") tints oi2.ply, the diffuse object, with its file's vertex colours; with `objects_file` it is ignored and each entry's
    "colors" holds.  A file without colours is a ValueError naming it.  `object_texture`: an image (a PNG of display values, or an
    .exr / .hdr of linear ones in [0, 1]) that textures oi2.ply over its file's per-vertex texture coordinates (DESIGN.md section 1.4,
    "Textured inserted objects"); with `objects_file` it is ignored and each entry's "texture" and "orm_texture" hold.  A file without
    coordinates is a ValueError naming it.  `composite`: differential rendering ("Differential render"): the
    objects, their shadows, bounce light and reflections are put into the photograph `photo_path` (default <scene_dir>/gt_image.exr,
    linear, as `pipeline.py` writes it; a .png is decoded with `loss.srgb_to_linear`; [H,W,3] of the maps' size, finite and >= 0)
    instead of re-rendering the fitted scene: the `n_iter` frames of `PathTracer.render_diff` are summed and composited once, into
    mi_oic_<name>_<env>.exr / .png.  A pixel no sample of which met an object keeps the photograph's bits; through glass the
    re-rendered scene shows, not the photograph.  With it `denoise="atrous"`, an `env_scale` other than 1 and a missing or wrongly
    sized photograph are a ValueError before any GPU work.  `composite_denoise` (with `composite`, even `spp`): the differential
    render's own a-trous filter ("Denoiser for the differential render"): each of the `n_iter` frames becomes
    two `render_diff` calls of spp / 2, seeds seed + 2 i (summed into one half) and seed + 2 i + 1 (into the other), and
    `PathTracer.denoise_diff` filters each pixel's own layer before the composite; a pixel farther than 63 pixels (5 levels) from
    every touched one still keeps the photograph's bits.  The output names are `composite`'s.  `see_through` (with `composite`; DESIGN.md
    section 1.4, "Seen through glass"): behind clear glass the photograph shows, refracted, instead of the re-rendered scene: the
    frames are `PathTracer.render_diff_through`'s, and fg + through (one fp32 addition) takes fg's place in the composite.  With
    `composite_denoise` the halves' (fg, delta, alpha) pass the filter as they are and the mean of the halves' `through`,
    (through_A + through_B) * (0.5 / n_iter), is added to the filtered fg: the filter's guides are the glass surface's and would blur
    the refracted photograph.  Rough glass stays re-rendered.  Without `composite` it is a ValueError before any other work; with
    `see_through=False` the code path, and so the bytes, are the ones without it.  `shadows` (with `composite`; DESIGN.md section 1.4,
    "Ratio shadow transfer"): "additive" (default) adds the model's difference to the photograph; "ratio" dims the photograph by the
    share of light the model loses, per channel, where the objects darken it, and stays additive where they brighten it: the frames
    are `PathTracer.render_diff_ratio`'s (with the photograph when `see_through`), `base` is summed with the others, and the picture
    is `composite_ratio`.  With `composite_denoise`, `base` passes `PathTracer.denoise_diff` a second time in delta's place beside a
    zero fg, which gives it delta's coverage weighting.  The output names are `composite`'s.  "ratio" without `composite`, or another
    value, is a ValueError before any other work; with "additive" the code path, and so the bytes, are the ones without it.  An entry of
    `objects_file` may carry "transform" and "motion" (`load_oi_scene`, `oi_pose`; DESIGN.md section 1.4, "Moving inserted objects").
    `frames` 1 (default): a still; a "transform" is baked into the vertices and normals on the host in fp64 before the meshes are merged
    (the identity leaves the file's bytes), and "motion" is ignored with a printed line.  `frames` > 1: a video: one movable tracer, per
    frame `PathTracer.move_objects` to the frame's poses and then the very branch a still runs for the options given, the feature guides
    computed anew -> <out>/oi_animation/frame_%04d.png, mi_oi[c]_<name>_<env>.mp4 and .gif, and the dict of paths
    `render_rolling_envmap` returns.  `frames` > 1 without an `objects_file` in which an object moves is a ValueError.  `tint` (r, g, b in
    (0, 1]; without `objects_file`): oi.ply, the glass, holds an absorbing medium ("Media inside glass") that gives
    white light this colour after the distance `tint_at` (default: the largest side of the mesh's bounding box); an entry of
    `objects_file` says "medium" itself, and with one `tint` is a ValueError, as is `tint_at` without `tint`.  `reflect_photo` (with
    `composite`; it implies `see_through`; DESIGN.md section 1.4, "Reflected in inserted objects"): what a diffuse, pbr or roughdielectric
    object reflects of the depth mesh is the photograph, not the re-rendered scene: every such object whose entry of `objects_file` does
    not say "photo" itself carries "photo": True (of the default pair, oi2.ply), and `PathTracer.render_diff_through` /
    `render_diff_ratio` follow the camera chain through its vertices.  With `composite_denoise` `through` by-passes the filter as it
    does behind glass, so on a rough flagged object it carries its unfiltered noise.  Without `composite` it is a ValueError before any
    other work; with `reflect_photo=False` and no entry that says "photo": true the code path, and so the bytes, are the ones without it."""
    if reflect_photo and not composite:
        raise ValueError("reflect_photo needs composite=True: it shows the photograph in what inserted objects reflect, in the differential composite")
    see_through = see_through or reflect_photo
    if shadows not in OI_SHADOWS:
        raise ValueError(f"shadows must be 'additive' or 'ratio', got {shadows!r}")
    if shadows == "ratio" and not composite:
        raise ValueError("shadows='ratio' needs composite=True: it transfers the differential render's shadows into the photograph as a ratio")
    if see_through and not composite:
        raise ValueError("see_through needs composite=True: it shows the photograph behind inserted glass in the differential composite")
    from . import mesh as _mesh
    from . import pathtrace as _pathtrace

    scene_dir = os.path.join(input_path if input_path is not None else OUT_DIR, save_name)
    if frames < 1:
        raise ValueError(f"frames must be at least 1, got {frames}")
    placed = None                                       # per object (its "transform", its "motion"), with an object list
    if objects_file is not None:
        entries = load_oi_scene(objects_file)
        have = [(e["ply"], e["bsdf"], e["normals"], e["colors"], e["texture"], e["orm_texture"], e["photo"]) for e in entries]
        placed = [(e["transform"], e["motion"]) for e in entries]
    if frames > 1 and not (placed and any(_oi_moves(mo) for _, mo in placed)):
        raise ValueError(f"frames={frames} would render {frames} equal frames: give an objects_file in which an object has a \"motion\" "
                         f"(\"spin\" with a deg_per_frame other than 0, or a \"slide\" other than 0)")
    if tint is None and tint_at is not None:
        raise ValueError("tint_at needs tint: it is the distance at which the glass has the tint's colour")
    if tint is not None and objects_file is not None:
        raise ValueError("tint colours oi.ply, the default glass: an entry of objects_file says \"medium\" itself")
    if objects_file is None:
        plys = [os.path.join(scene_dir, "oi.ply"), os.path.join(scene_dir, "oi2.ply")]
        bsdfs = [{"type": "dielectric", "int_ior": OI_INT_IOR, "ext_ior": OI_EXT_IOR}, {"type": "diffuse", "reflectance": (OI_REFLECTANCE,) * 3}]
        if tint is not None:
            if not os.path.exists(plys[0]):
                raise FileNotFoundError(f"tint colours the glass object, {plys[0]}, which does not exist")
            at = tint_at
            if at is None:                                # the largest side of the mesh's bounding box
                Vg = np.asarray(_mesh.read_ply_any(plys[0], normals=True, colors=True, uv=True)[0], np.float64)
                at = float((Vg.max(0) - Vg.min(0)).max())
            bsdfs[0]["medium"] = {"color": [float(x) for x in tint], "at": at}
            _pathtrace.object_medium(bsdfs[0])           # ValueError now, before any other work
        have = [(p, b, object_normals, c, t, None, None) for p, b, c, t in zip(plys, bsdfs, ("none", object_colors), (None, object_texture))
                if os.path.exists(p)]
        if not have:
            raise FileNotFoundError(f"object insertion needs {plys[0]} (glass) or {plys[1]} (diffuse); neither exists")
    if n_iter < 1:
        raise ValueError(f"n_iter must be at least 1, got {n_iter}")
    if object_normals not in ("flat", "vertex"):
        raise ValueError(f"object_normals must be 'flat' or 'vertex', got {object_normals!r}")
    if object_colors not in OI_COLORS:
        raise ValueError(f"object_colors must be 'none', 'vertex' or 'vertex_linear', got {object_colors!r}")
    atrous = _check_denoise(denoise, "path", spp)
    if composite_denoise and not composite:
        raise ValueError("composite_denoise needs composite=True: it filters the differential render (denoise='atrous' filters the plain one)")
    if composite_denoise and (spp < 2 or spp % 2):
        raise ValueError(f"composite_denoise splits every frame into two halves of spp / 2 samples: spp must be even, got {spp}")
    _scaled_env(np.zeros(0, np.float32), env_scale)
    photo = _oi_photo(scene_dir, photo_path, atrous, env_scale) if composite else None
    env_path = find_envmap_oi(save_name, env_path, input_path)
    objects = []
    for k, (p, b, normals, colors, texture, orm_texture, flagged) in enumerate(have):
        V, T, Nn, Cc, Uv = _mesh.read_ply_any(p, normals=True, colors=True, uv=True)
        if normals == "vertex" and Nn is None:
            Nn = _mesh.angle_weighted_normals(V, T)
        transform, motion = placed[k] if placed else (None, None)
        if frames == 1 and motion is not None:
            print(f"{p}: \"motion\" is ignored for a still (frames=1)")
        if frames == 1 and transform is not None:     # the static route: the placement baked into the vertices and normals, fp64
            sim = oi_pose(transform, None, 0, pivot=0.5 * (np.asarray(V, np.float64).min(0) + np.asarray(V, np.float64).max(0)))
            if not (np.array_equal(sim[0], np.eye(3)) and sim[1] == 1.0 and not sim[2].any()):   # the identity leaves the file's bytes
                V = _pathtrace.apply_similarity(sim, V)
                Nn = None if Nn is None else _pathtrace.apply_similarity(sim, Nn, vectors=True)
        objects.append({"vertices": V, "triangles": T, "bsdf": b})
        if flagged if flagged is not None else (reflect_photo and b.get("type") in _pathtrace.PHOTO_TYPES):
            objects[-1]["photo"] = True
        if texture is not None or orm_texture is not None:
            objects[-1]["uv"] = _object_uv(p, Uv)
        if texture is not None:
            objects[-1]["texture"] = _object_image(texture, decode=True)
        if orm_texture is not None:
            objects[-1]["orm_texture"] = _object_image(orm_texture, decode=False)
        if colors != "none":
            objects[-1]["colors"] = _object_colors(p, Cc, colors)
        if normals == "vertex":
            objects[-1]["normals"] = Nn
    mat = load_estimated_brdf(os.path.join(scene_dir, "best_results"), device)
    env = _scaled_env(load_image(env_path), env_scale)
    env_id = os.path.basename(env_path)[:-4]
    out_dir = os.path.join(save_path if save_path else OUT_DIR, save_name)
    base = os.path.join(out_dir, f"mi_oi{'c' if composite else ''}_{save_name}_{env_id}")   # (:233-236)
    image = lambda pt, tabs: _oi_image(pt, tabs, mat, env, photo, [h[1] for h in have], spp, n_iter, max_depth, seed, device, atrous, composite,
                                       composite_denoise, see_through, shadows == "ratio")
    if frames > 1:
        return _oi_animation(scene_dir, save_name, mat, device, objects, placed, frames, env, image, out_dir, base)
    pt = _path_tracer(scene_dir, save_name, mat, device, objects)
    img = image(pt, pt.tables(env))
    os.makedirs(out_dir, exist_ok=True)
    write_exr(base + ".exr", img.cpu().numpy())
    write_png(base + ".png", _loss.linear_to_srgb(img.clamp_min(0)).cpu().numpy())
    return base + ".png"


def _oi_animation(scene_dir: str, save_name: str, mat, device, objects, placed, frames: int, env, image, out_dir: str, base: str) -> Dict[str, object]:
    """`render_oi(frames > 1)`: one movable tracer over the files' meshes as they are (the rest pose), `reach` the farthest any frame's pose
    carries a corner of a rest bounding box; per frame `move_objects` to the frame's poses and then `image(pt, tabs)`, the branch a still
    runs -> <out>/oi_animation/frame_%04d.png, `base`.mp4 and .gif, as `render_rolling_envmap` writes its own."""
    from . import pathtrace as _pathtrace

    boxes = [(np.asarray(ob["vertices"], np.float64).min(0), np.asarray(ob["vertices"], np.float64).max(0)) for ob in objects]
    sims = [[oi_pose(tr, mo, f, pivot=0.5 * (lo + hi)) for (tr, mo), (lo, hi) in zip(placed, boxes)] for f in range(frames)]
    reach = max(_pathtrace.pose_extent(sim, lo, hi) for per_frame in sims for sim, (lo, hi) in zip(per_frame, boxes))
    pt = _path_tracer(scene_dir, save_name, mat, device, objects, movable=True, reach=reach * (1 + 1e-6))   # the poses are rounded to fp32 on their way
    tabs = pt.tables(env)
    anim_dir = os.path.join(out_dir, "oi_animation")
    os.makedirs(anim_dir, exist_ok=True)
    paths, imgs = [], []
    for f in range(frames):
        pt.move_objects([{"rotate": R, "scale": s, "translate": t, "pivot": c} for R, s, t, c in sims[f]])
        srgb = _loss.linear_to_srgb(image(pt, tabs).clamp_min(0)).clamp(0, 1).cpu().numpy()
        paths.append(os.path.join(anim_dir, f"frame_{f:04d}.png"))
        write_png(paths[-1], srgb)
        imgs.append((srgb * 255 + 0.5).astype(np.uint8))
    from PIL import Image

    from .video_mp4 import write_mp4

    pil = [Image.fromarray(i) for i in imgs]
    pil[0].save(base + ".gif", save_all=True, append_images=pil[1:], duration=100, loop=0)
    return {"animation_dir": anim_dir, "frames": paths, "gif": base + ".gif", "mp4": write_mp4(base + ".mp4", imgs, fps=10)}


def _oi_image(pt, tabs, mat, env, photo, bsdfs, spp: int, n_iter: int, max_depth: int, seed: int, device, atrous: bool, composite: bool,
              composite_denoise: bool, see_through: bool, ratio: bool) -> torch.Tensor:
    """One picture of `render_oi` from the tracer as it stands: the branch its options select (plain, denoise="atrous", composite,
    composite_denoise, see_through, shadows="ratio"), the feature guides computed now."""
    from . import pathtrace as _pathtrace

    diff = (lambda n, sd: pt.render_diff_through(mat["albedo"], mat["roughness"], mat["metallic"], env, photo, n, max_depth, sd, tables=tabs)[:4]) if see_through else \
           (lambda n, sd: pt.render_diff(mat["albedo"], mat["roughness"], mat["metallic"], env, n, max_depth, sd, tables=tabs)[:3])
    if ratio:   # (fg, delta, alpha[, through], base): the additive frame's order, base last
        def diff(n, sd):
            fg, delta, base, alpha, *through, _ = pt.render_diff_ratio(mat["albedo"], mat["roughness"], mat["metallic"], env, n, max_depth, sd, tables=tabs,
                                                                       photo=photo if see_through else None)
            return (fg, delta, alpha, *through, base)
    if composite and composite_denoise:
        halves = [None, None]
        for i in range(n_iter):
            for k in (0, 1):
                frame = diff(spp // 2, seed + 2 * i + k)
                halves[k] = frame if halves[k] is None else tuple(x + y for x, y in zip(halves[k], frame))
        geom = pt.features()
        tint = pt.feature_tints() if pt.stats["n_textured_objects"] else pt.feature_colors() if pt.stats["n_colored_objects"] else None
        guide = albedo_guide(geom, mat["albedo"], bsdfs, tint)
        fg, delta, alpha = pt.denoise_diff(halves[0][:3], halves[1][:3], guide, geom, 1.0 / n_iter)
        if ratio:   # base in delta's place beside a zero fg: delta's coverage weighting
            zero = torch.zeros_like(halves[0][0])
            base = pt.denoise_diff((zero, halves[0][-1], halves[0][2]), (zero, halves[1][-1], halves[1][2]), guide, geom, 1.0 / n_iter)[1]
        if see_through:   # the refracted photograph does not pass the filter
            fg = fg + (halves[0][3] + halves[1][3]) * (0.5 / n_iter)
        img = _pathtrace.composite_ratio(fg, delta, base, alpha, torch.from_numpy(photo).to(device), 1.0) if ratio else \
            _pathtrace.composite(fg, delta, alpha, torch.from_numpy(photo).to(device), 1.0)
    elif composite:
        sums = None
        for i in range(n_iter):
            frame = diff(spp, seed + i)
            sums = frame if sums is None else tuple(x + y for x, y in zip(sums, frame))
        if see_through:
            sums = (sums[0] + sums[3], sums[1], sums[2], *sums[4:])
        img = _pathtrace.composite_ratio(sums[0], sums[1], sums[3], sums[2], torch.from_numpy(photo).to(device), 1.0 / n_iter) if ratio else \
            _pathtrace.composite(*sums, torch.from_numpy(photo).to(device), 1.0 / n_iter)
    elif atrous:
        geom = pt.features()
        half = lambda sd: pt.render(mat["albedo"], mat["roughness"], mat["metallic"], env, spp // 2, max_depth, sd, tables=tabs)
        tint = pt.feature_tints() if pt.stats["n_textured_objects"] else pt.feature_colors() if pt.stats["n_colored_objects"] else None
        img = _denoised(pt, half, n_iter, seed, geom, albedo_guide(geom, mat["albedo"], bsdfs, tint))
    else:
        img = torch.zeros_like(mat["albedo"])
        for i in range(n_iter):
            img += pt.render(mat["albedo"], mat["roughness"], mat["metallic"], env, spp, max_depth, seed + i, tables=tabs)
        img /= n_iter
    return img


TRANS_ALBEDO, TRANS_ROUGHNESS, TRANS_METALLIC = 0.7, 0.3, 0.0   # the maps inside the mask (trans_edit.py:25-28)


def render_trans(save_name: str, ior: float = 1.2, keep_albedo_color: bool = False, spec_trans: float = 0.4, env_path: Optional[str] = None,
                 input_path: Optional[str] = None, save_path: Optional[str] = None, spp: int = 64, iters: int = 10, max_depth: int = 4,
                 seed: int = 0, refract_distance: float = 100.0, device="cuda", denoise: str = "off") -> str:
    """trans_edit.py:16-60: the masked part of the scene as glass (TransBSDF; DESIGN.md section 1.4, "Transparency editing") ->
    mi_trans_<ior>_<wA|woA>_<specTrans>_<name>_<env>.exr / .png.  Needs best_results/mask.png and best_results/bg.png.  Inside the
    mask the albedo becomes 0.7 unless `keep_albedo_color`, roughness 0.3 and metallic 0.  The light is `env_path`, else
    best_results/envmap.hdr.  `iters` renders with seeds seed + i are averaged.  `denoise="atrous"` (even `spp`): each of them becomes
    two of spp / 2, seeds seed + 2 i and seed + 2 i + 1, and one a-trous pass runs over the two sums; the masked pixels are an id of
    their own, so nothing filters across the mask's edge, and inside it the guide is the edited albedo."""
    scene_dir = os.path.join(input_path if input_path is not None else OUT_DIR, save_name)
    mat_dir = os.path.join(scene_dir, "best_results")
    for name in ("mask.png", "bg.png"):
        if not os.path.exists(os.path.join(mat_dir, name)):
            raise FileNotFoundError(f"transparency editing needs {os.path.join(mat_dir, name)}")
    if iters < 1:
        raise ValueError(f"iters must be at least 1, got {iters}")
    atrous = _check_denoise(denoise, "path", spp)
    env_path = find_envmap(save_name, env_path, input_path)
    mat = load_estimated_brdf(mat_dir, device)
    mask = mat["mask"]
    if not keep_albedo_color:
        mat["albedo"][mask] = TRANS_ALBEDO
    mat["roughness"][mask] = TRANS_ROUGHNESS
    mat["metallic"][mask] = TRANS_METALLIC
    pt = _path_tracer(scene_dir, save_name, mat, device)
    env = load_image(env_path)
    tabs = pt.tables(env)
    if atrous:
        geom = pt.features()
        guide = albedo_guide(geom, mat["albedo"])                   # the maps are edited above: inside the mask, the edited albedo
        geom = geom.clone()
        geom[..., 7][mask] = 1.0                                    # the glass is an id of its own
        half = lambda sd: pt.render_trans(mat["albedo"], mat["roughness"], mat["metallic"], env, mask, mat["bg"], ior, spec_trans,
                                          refract_distance, spp // 2, max_depth, sd, tables=tabs)
        img = _denoised(pt, half, iters, seed, geom, guide)
    else:
        img = torch.zeros_like(mat["albedo"])
        for i in range(iters):
            img += pt.render_trans(mat["albedo"], mat["roughness"], mat["metallic"], env, mask, mat["bg"], ior, spec_trans, refract_distance, spp,
                                   max_depth, seed + i, tables=tabs)
        img /= iters
    env_id = os.path.basename(env_path)[:-4]
    out_dir = os.path.join(save_path if save_path else OUT_DIR, save_name)
    os.makedirs(out_dir, exist_ok=True)
    flag = "wA" if keep_albedo_color else "woA"
    base = os.path.join(out_dir, f"mi_trans_{ior}_{flag}_{spec_trans}_{save_name}_{env_id}")   # (trans_edit.py:45-48)
    write_exr(base + ".exr", img.cpu().numpy())
    write_png(base + ".png", _loss.linear_to_srgb(img.clamp_min(0)).cpu().numpy())
    return base + ".png"


def render_rolling_envmap(save_name: str, env_path: Optional[str], frames: int = 36, rotation_step: float = 10.0,
                          input_path: Optional[str] = None, save_path: Optional[str] = None, spp: int = 64, device="cuda",
                          write_frames: bool = True, edit: Optional[Dict[str, object]] = None, integrator: str = "sh",
                          max_depth: int = 4, seed: int = 0, shading_normals: str = "face", denoise: str = "off",
                          env_scale: float = 1.0, relight_composite: bool = False, relight_photo: Optional[str] = None,
                          relight_floor: Optional[float] = None) -> Dict[str, object]:
    """render_final.py:300-418: `frames` renders, the envmap rolled by int(angle/360*W) columns per frame.  integrator "sh": the
    rolled light is the SH rotation of the projected envmap; "path": the path tracer renders the rolled texels themselves (`shading_normals` as in `render_real`).
    `denoise="atrous"` (path only, even `spp`): every frame is two renders of spp / 2, seeds `seed` and `seed + 1`, through the a-trous
    filter; the features are computed once for all frames.  `env_scale` (path only): the envmap is multiplied by it first.
    `relight_composite=True` ("Relighting in the photograph"; path only, no edit): every frame is the photograph
    (`relight_photo`, default <scene>/gt_image.exr) under the rolled envmap: environment A is the fitted best_results/envmap.hdr, B the
    frame's rolled envmap, as in `render_real` -> <out>/rolling_rc_animation/frame_%04d.png and rolling_rc_<name>_<env>.mp4 / .gif.  Without
    an `env_path` (and with `env_scale` 1) frame 0 is the photograph, bit for bit."""
    _check_integrator(integrator, shading_normals)
    _scaled_env(np.zeros(0, np.float32), env_scale, integrator)
    atrous = _check_denoise(denoise, integrator, spp)
    scene_dir = os.path.join(input_path if input_path is not None else OUT_DIR, save_name)
    if not relight_composite and (relight_photo is not None or relight_floor is not None):
        raise ValueError("relight_photo and relight_floor need relight_composite=True")
    if relight_composite:
        _check_relight_composite(integrator, edit, False, relight_floor)
        photo = _oi_photo(scene_dir, relight_photo, False, 1.0)
        fitted_env_path = find_envmap(save_name, None, input_path)
    env_path = find_envmap(save_name, env_path, input_path)
    env = _scaled_env(load_image(env_path), env_scale, integrator)
    We = env.shape[1]
    light0 = envmap_to_light(env)
    shifts = [int((f * rotation_step / 360.0) * We) for f in range(frames)]   # rotate_envmap (:290-298)
    mat = load_estimated_brdf(os.path.join(scene_dir, "best_results"), device)
    apply_edit(mat, edit)
    if integrator == "path":
        pt = _path_tracer(scene_dir, save_name, mat, device)
        nrm = mat["normal"] if shading_normals == "map" else None
        if relight_composite:
            env_a = load_image(fitted_env_path)
            tabs_a = pt.tables(env_a)                                # A does not roll: one set for all frames, as the features are
            geom = pt.features(normal=nrm) if atrous else None
            guides = (geom, albedo_guide(geom, mat["albedo"])) if atrous else None
            photo_t = torch.from_numpy(photo).to(pt.device)
            render_frame = lambda f: _relit_photo(pt, mat, env_a, tabs_a, np.roll(env, shifts[f], axis=1), nrm, spp, max_depth, seed, guides,
                                                  photo_t, relight_floor)
        elif atrous:
            geom = pt.features(normal=nrm)                           # the camera and the mesh do not move: one set for all frames
            guide = albedo_guide(geom, mat["albedo"])

            def render_frame(f):
                rolled = np.roll(env, shifts[f], axis=1)
                tabs = pt.tables(rolled)
                half = lambda sd: pt.render(mat["albedo"], mat["roughness"], mat["metallic"], rolled, spp // 2, max_depth, sd, tables=tabs,
                                            normal=nrm)
                return _denoised(pt, half, 1, seed, geom, guide)
        else:
            render_frame = lambda f: pt.render(mat["albedo"], mat["roughness"], mat["metallic"], np.roll(env, shifts[f], axis=1), spp, max_depth,
                                               seed, normal=nrm)
        render_frames = lambda f0, f1: torch.stack([render_frame(f) for f in range(f0, f1)])
    else:
        lights = [_sh.rotate_y_matrix(2 * np.pi * s / We) @ light0 for s in shifts]
        rl = Relighter(mat, _scene_normal(scene_dir, mat, save_name, device), spp, mesh_mask=_mesh_mask(scene_dir))
        render_frames = lambda f0, f1: rl.frames(np.stack(lights[f0:f1]))
    out_dir = os.path.join(save_path if save_path else OUT_DIR, save_name)
    tag = "rolling_rc" if relight_composite else "rolling_envmap"
    anim_dir = os.path.join(out_dir, f"{tag}_animation")
    os.makedirs(anim_dir, exist_ok=True)
    env_id = os.path.basename(env_path)[:-4]
    paths: List[str] = []
    imgs = []
    for f0 in range(0, frames, 24):                                  # matpbr_relight's chunk: the transfer is read once per 24 frames
        batch = render_frames(f0, min(f0 + 24, frames))
        if write_frames:
            srgb = _loss.linear_to_srgb(batch.clamp_min(0)).clamp(0, 1).cpu().numpy()
            for k in range(srgb.shape[0]):
                path = os.path.join(anim_dir, f"frame_{f0 + k:04d}.png")
                write_png(path, srgb[k])
                paths.append(path)
                imgs.append((srgb[k] * 255 + 0.5).astype(np.uint8))
    gif_path = None
    if imgs:
        from PIL import Image

        from .video_mp4 import write_mp4

        gif_path = os.path.join(out_dir, f"{tag}_{save_name}_{env_id}.gif")     # render_final.py:405-414 writes both
        pil = [Image.fromarray(i) for i in imgs]
        pil[0].save(gif_path, save_all=True, append_images=pil[1:], duration=100, loop=0)
        mp4_path = write_mp4(os.path.join(out_dir, f"{tag}_{save_name}_{env_id}.mp4"), imgs, fps=10)
    return {"animation_dir": anim_dir, "frames": paths, "gif": gif_path, "mp4": mp4_path if imgs else None}
