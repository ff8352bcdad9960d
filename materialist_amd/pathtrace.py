"""Path-traced re-render of the depth mesh: `PathTracer` over libmatpbr_path.so (include/matpbr_path.h), and every name of the binding.
The binding lies in four modules, which this one re-exports: path_abi (the ctypes ABI, `load`, `symbol`), path_scene (the objects,
the merged mesh, the BVH, the tables), path_host (the CPU twins the tests call) and path_filters (the denoisers and the composite).

The deterministic render is direct light, unshadowed, under SH25.  The reference's *final* images come from
Mitsuba's `path` integrator, `max_depth` 4, on the `.ply` mesh under the texel envmap (render_final.py:35-96, inverse_img_w_mi.py:
49-52).  `PathTracer` is that render on the GPU: shadows, inter-reflection, the envmap's texels as the light.
`PathTracer.render_bwd` is its backward pass (the fixed-seed estimator's derivative with the sampling detached) and `PathRenderFn`
puts both behind autograd.  `PathTracer.features` and `PathTracer.denoise` are the opt-in denoiser (DESIGN.md section 1.4,
"Denoiser"): first-hit features and a variance-guided a-trous filter over two half renders, forward only.  `PathTracer.render_diff`
and `composite` are the differential render ("Differential render"): what inserted objects add to and take
from a photograph of the scene, forward only; `PathTracer.denoise_diff` is its own a-trous filter over two halves of it ("Denoiser
for the differential render"); `PathTracer.render_diff_through` is the differential render with the photograph shown, refracted,
behind inserted clear glass ("Seen through glass"); `PathTracer.render_diff_ratio` and `composite_ratio` transfer the shadows as a
ratio of the model's radiance with and without the objects ("Ratio shadow transfer").  A glass object may hold a homogeneous medium
("Media inside glass"): `render` and the three differential renders then take the entries that know it.  A diffuse, pbr or
roughdielectric object may carry "photo": True ("Reflected in inserted objects"): `render_diff_through` and `render_diff_ratio` with a
photograph then show the photograph in what the object reflects.  `PathTracer.render_edit_diff`, `edit_mask` and `composite_edit`
put a material edit into the photograph ("Material edits in the photograph"): the differential render of edited maps on a tracer
without objects.  `PathTracer.render_relight` and `composite_relight` put a new light into the photograph ("Relighting in the
photograph"): one walk under the fitted and the new envmap, and the quotient image.  There is no fallback: a missing or failing
library raises.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from .path_abi import *      # noqa: F401,F403
from .path_abi import _FEATURE, _P, _aligned_texels, _ptr, _ref, _rows, _same_rows, _table_ptrs, _tex_ptrs, _uncolored, _unflagged  # noqa: F401
from .path_filters import *  # noqa: F401,F403
from .path_host import *     # noqa: F401,F403
from .path_host import _host_image  # noqa: F401
from .path_scene import *    # noqa: F401,F403

def _dptr(t):
    return t.data_ptr() if t is not None else None


def edit_mask(fitted, edited) -> torch.Tensor:
    """bool [H,W]: the texels where the maps `edited` = (a_e, r_e, m_e) differ from `fitted` = (a, r, m) in the bits of any of their five
    float32 values (albedo [H,W,3], roughness and metallic [H,W] or [H,W,1]; tensors or arrays), on the device of `fitted`'s albedo.
    Bitwise, so -0.0 differs from 0.0 and a NaN equals itself: a texel is masked exactly where a walk could read another value."""
    a = torch.as_tensor(fitted[0])
    if a.dim() != 3 or a.shape[2] != 3:
        raise ValueError(f"albedo must be [H,W,3], got {tuple(a.shape)}")
    H, W = int(a.shape[0]), int(a.shape[1])
    out = torch.zeros(H, W, dtype=torch.bool, device=a.device)
    for x, y, c in zip(fitted, edited, (3, 1, 1)):
        x, y = (torch.as_tensor(t).to(a.device, torch.float32).reshape(H, W, c).contiguous().view(torch.int32) for t in (x, y))
        out |= (x != y).any(-1)
    return out


class PathTracer:
    """One mesh in the renderer's frame (camera at the origin looking down -z, `fov_x_deg` horizontal field of view, H x W pixels).
    The BVH is built once on the host and kept on the device; `render` takes the maps and the envmap of each frame.
    `objects`: meshes inserted into the scene ("Inserted objects"), in the same frame, outward winding, a list
    of {"vertices" [Nv,3], "triangles" [Nt,3], "bsdf": {"type": "dielectric", "int_ior": 1.49, "ext_ior": 1.000277} or
    {"type": "diffuse", "reflectance": (r, g, b)} or {"type": "pbr", "albedo": (r, g, b), "roughness": r, "metallic": m} (the depth
    mesh's own BSDF on constants; DESIGN.md section 1.4, "PBR inserted objects")} and optionally "normals" [Nv,3] (per vertex,
    outward): with them the object shades smooth, with the normals interpolated at each hit; without them flat.  An object with
    {"type": "area", "radiance": (r, g, b)} is an area light ("Emissive inserted objects"): it emits its
    radiance from its outward faces, reflects nothing, takes no "normals", and is sampled as an emitter beside the envmap at every
    vertex (`stats["n_lights"]` counts them; an envmap of zero luminance leaves the lights as the only emitters).  An object with
    {"type": "roughdielectric", "int_ior": 1.49, "ext_ior": 1.000277, "alpha": 0.1} is rough (frosted) glass (DESIGN.md section 1.4,
    "Rough dielectric objects"; `stats["n_rough_objects"]` counts them): it shades from both sides, takes "normals", and, unlike
    clear glass, takes an emitter sample at every vertex.  A diffuse or pbr object may carry "colors" [Nv,3] (per vertex, linear RGB in
    [0, 1]; DESIGN.md section 1.4, "Vertex-coloured inserted objects"; `stats["n_colored_objects"]` counts them): its reflectance or
    albedo is multiplied by the colour interpolated at each hit.  A diffuse or pbr object may carry "uv" [Nv,2] with "texture" [h,w,3]
    (base colour, linear, in [0, 1], row 0 the top row) and, a pbr one, "orm_texture" [h,w,3] ("Textured inserted
    objects"; `stats["n_textured_objects"]` counts them): the reflectance or the albedo is multiplied by the base colour, the roughness
    and the metallic by the orm image's g and b, each read with bilinear filtering and repeat wrapping at the coordinate interpolated
    at the hit.  A dielectric or roughdielectric bsdf may carry "medium": {"sigma_a": (r, g, b), "scatter": sigma_s, "g": g} or {"color":
    (r, g, b), "at": d, ...} ("Media inside glass"; `stats["n_medium_objects"]` counts them): a homogeneous medium
    behind the interface, chromatic absorption and grey scattering with a Henyey-Greenstein phase function, the coefficients per scene
    unit.  `move_objects` leaves them per scene unit, so an object scaled by s is optically s times thicker.  A dense medium of high
    albedo loses the energy of the paths that max_depth (16 at the most) cuts, as Mitsuba does at the same max_depth.
    An object of bsdf type diffuse, pbr or roughdielectric may carry "photo": True ("Reflected in inserted
    objects"; `stats["n_photo_objects"]` counts them): the camera chain of `render_diff_through` (and of `render_diff_ratio` with a
    photograph) passes its vertices, so that the depth mesh it reflects is the photograph.  Every other method renders it as without the key.
    A tracer with objects renders forward only.  `movable=True` (with objects; DESIGN.md section 1.4, "Moving inserted
    objects"; `stats["movable"]`): the BVH is grafted, the depth mesh's subtree and the objects' under one root, and the objects' rest
    pose stays on the device, so that `move_objects` places them anew without a rebuild (two launches; well under a millisecond for a small mesh); `reach`: the largest coordinate magnitude any
    later pose will have (default, and at least: the rest scene's; `stats["reach"]`), for which the boxes are padded.  `movable=False`
    is the merged BVH and the static route."""

    def __init__(self, vertices: np.ndarray, triangles: np.ndarray, H: int, W: int, fov_x_deg: float = 35.0, device="cuda",
                 objects: Optional[Sequence[dict]] = None, movable: bool = False, reach: Optional[float] = None):
        if movable and not objects:
            raise ValueError("movable=True moves inserted objects: build the PathTracer with `objects`")
        self.H, self.W, self.fov = int(H), int(W), float(fov_x_deg)
        self.device = torch.device(device)
        self._move: Optional[dict] = None             # what `move_objects` needs of a movable tracer: the rest pose on the device, the refit's tables
        n_scene = int(np.asarray(triangles).reshape(-1, 3).shape[0])
        n_scene_vert = int(np.asarray(vertices).reshape(-1, 3).shape[0])
        self.objects = None
        self.obj_nrm: Optional[torch.Tensor] = None   # corner normals of the inserted triangles, when some object is smooth
        self.n_scene_tris = n_scene
        self.pbr = None                               # the PathObjectPbr records, when some object is of kind BSDF_PBR
        self.lights = None                            # (PathLights, tris, cdf on the device), when some object is of kind BSDF_AREA
        self.rough = False                            # some object is of kind BSDF_ROUGH_DIELECTRIC: `render` takes the rough entry point
        self.obj_col: Optional[torch.Tensor] = None   # corner colours of the inserted triangles, when some object is coloured
        self.textures = None                          # (obj_uv, PathObjectTex records, texels on the device), when some object is textured
        self.media = None                             # the PathObjectMedium records, when some glass object holds a medium
        self.reflect = False                          # some object carries OBJECT_PHOTO: the see-through renders take the entry that knows it
        counts = dict.fromkeys(COUNT_KEYS, 0)
        if objects:
            scene = merge_scene(vertices, triangles, objects, lights=True, symbol=symbol)
            vertices, triangles, counts = scene.V, scene.T, scene.counts
            self.objects = (PathObject * len(scene.table))(*scene.table)
            for have, level in ((scene.lights, "lights"), (counts["n_rough_objects"], "rough"), (counts["n_pbr_objects"], "pbr"),
                                (counts["n_smooth_objects"], "normals"), (counts["n_colored_objects"], "colors"), (scene.textures, "textures")):
                if have:                              # a library built before the feature: PathError now, not at the first render
                    symbol("matpbr_path_render_objects_" + level)
            if scene.media is not None:
                for name in ("matpbr_path_render_objects_media", "matpbr_path_render_objects_diff_media"):
                    symbol(name)
                self.media = (PathObjectMedium * len(scene.media))(*scene.media)
            if any(t.kind & OBJECT_PHOTO for t in scene.table):
                symbol("matpbr_path_render_objects_reflect")
                self.reflect = True
            if scene.obj_col is not None:
                symbol("matpbr_path_feature_colors")
                self.obj_col = torch.from_numpy(scene.obj_col).to(self.device)
            if scene.textures is not None:
                symbol("matpbr_path_feature_tints")
                uv, records, texels = scene.textures
                self.textures = (torch.from_numpy(uv).to(self.device), (PathObjectTex * len(records))(*records), torch.from_numpy(texels).to(self.device))
            if scene.lights is not None:
                lt = scene.lights
                self.lights = (lt["header"], torch.from_numpy(lt["tris"]).to(self.device), torch.from_numpy(lt["cdf"]).to(self.device))
            self.rough = counts["n_rough_objects"] > 0
            if any(counts[key] for key in COUNT_KEYS if key != "n_smooth_objects") or self.media is not None:
                self.pbr = (PathObjectPbr * len(scene.records))(*scene.records)   # the entry points from the lights' on take the records beside the table as well
            if scene.obj_nrm is not None:
                self.obj_nrm = torch.from_numpy(scene.obj_nrm).to(self.device)
            if movable:
                symbol("matpbr_path_objects_move")    # a library built before the feature: PathError now, not at the first move
                bvh = build_bvh_grafted(vertices, triangles, n_scene, reach, n_scene_vert)
            else:
                bvh = build_bvh(vertices, triangles, n_scene)
        else:
            bvh = build_bvh(vertices, triangles)
        self.stats = {k: bvh[k] for k in ("n_nodes", "depth", "n_leaves", "build_s")}
        if movable:
            dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(self.device)
            boxes = [(np.asarray(ob["vertices"], np.float64).min(0), np.asarray(ob["vertices"], np.float64).max(0)) for ob in objects]
            self._move = {"rest_tris": dev(bvh["rest_tris"]), "node_level": dev(bvh["node_level"]), "first_object_node": bvh["first_object_node"],
                          "n_object_nodes": bvh["n_object_nodes"], "object_depth": bvh["object_depth"], "pad": bvh["pad"], "boxes": boxes,
                          "rest_nrm": None if self.obj_nrm is None else self.obj_nrm.clone(),
                          "rest_light_tris": None if self.lights is None else self.lights[1].clone(),
                          "rest_lights": None if self.lights is None else scene.lights}
            self.reach = bvh["reach"]                 # the largest coordinate magnitude a pose may have: the boxes' padding was sized for it
            self.stats["movable"] = True
            self.stats["reach"] = self.reach
        self.stats["n_tris"] = int(np.asarray(triangles).reshape(-1, 3).shape[0])
        self.stats["n_objects"] = len(self.objects) if self.objects is not None else 0
        self.stats["n_object_tris"] = self.stats["n_tris"] - n_scene
        self.stats.update(counts)
        self.stats["n_medium_objects"] = sum(1 for t in self.objects if t.kind & OBJECT_MEDIUM) if self.objects is not None else 0
        self.stats["n_photo_objects"] = sum(1 for t in self.objects if t.kind & OBJECT_PHOTO) if self.objects is not None else 0
        self.stats["bytes"] = int(bvh["nodes"].nbytes + bvh["tris"].nbytes)
        self.nodes = torch.from_numpy(bvh["nodes"]).to(self.device)
        self.tris = torch.from_numpy(bvh["tris"]).to(self.device)
        self._ws: Optional[torch.Tensor] = None      # render_bwd's workspace, kept between calls
        self._dn_ws: Optional[torch.Tensor] = None   # denoise's

    def _tables(self, env: torch.Tensor):
        tab = env_tables(env.cpu().numpy())          # host, fp64 -> fp32: microseconds for the 16 x 32 maps of the pipeline
        return (env.contiguous(), *(torch.from_numpy(np.ascontiguousarray(tab[k])).to(self.device) for k in ("row_cdf", "col_cdf", "pdf")))

    def tables(self, envmap) -> tuple:
        """(env, row_cdf, col_cdf, pdf) on the device for `render` / `render_bwd`'s `tables=`: hold them fixed across calls."""
        env = torch.as_tensor(envmap).to(self.device, torch.float32)
        if env.dim() != 3 or env.shape[2] != 3:
            raise ValueError(f"envmap must be [He,We,3], got {tuple(env.shape)}")
        return self._tables(env)

    def _inputs(self, albedo, roughness, metallic, envmap, tables):
        H, W, dev = self.H, self.W, self.device
        f = lambda x, c: torch.as_tensor(x).to(dev, torch.float32).reshape(H, W, c).contiguous()
        a, r, m = f(albedo, 3), f(roughness, 1), f(metallic, 1)
        if tables is None:
            env, row, col, pdf = self.tables(envmap)
        else:
            _, row, col, pdf = tables
            env = torch.as_tensor(envmap).to(dev, torch.float32).contiguous()
            if tuple(env.shape) != tuple(pdf.shape) + (3,):
                raise ValueError(f"envmap {tuple(env.shape)} does not match its tables {tuple(pdf.shape)}")
        return a, r, m, env, row, col, pdf

    def _frame(self, a, r, m, env, row, col, pdf, spp, max_depth, seed, spp_per_launch) -> tuple:
        """The 18 common arguments of a render or a backward pass (SIGNATURES' _FRAME) over what `_inputs` returned."""
        return (self.nodes.data_ptr(), self.tris.data_ptr(), a.data_ptr(), r.data_ptr(), m.data_ptr(), self.H, self.W, self.fov,
                env.data_ptr(), row.data_ptr(), col.data_ptr(), pdf.data_ptr(), int(env.shape[0]), int(env.shape[1]),
                int(spp), int(max_depth), int(seed) & 0xFFFFFFFF, int(spp_per_launch))

    def _normal(self, normal, what: str) -> torch.Tensor:
        """The shading-normal map [H,W,3] on the device, used as given; `what` names the caller in the refusals."""
        if self.objects is not None:
            raise ValueError(f"{what} knows no shading normals on a tracer with inserted objects: build the PathTracer without `objects`")
        nrm = torch.as_tensor(normal)
        if tuple(nrm.shape) != (self.H, self.W, 3):
            raise ValueError(f"normal must be [{self.H},{self.W},3], got {tuple(nrm.shape)}")
        return nrm.to(self.device, torch.float32).contiguous()

    def object_args(self, photo_flag: bool = False) -> tuple:
        """(table, n_objects, obj_nrm, n_scene_tri, records, lights header, light_tris, light_cdf, obj_col, obj_uv, texture records, texels,
        n_texels): the object arguments of a forward entry point after `stream`, as the C ABI takes them, None where the tracer has
        none.  An entry takes the first OBJECT_ENTRIES[its name] of them.  The last four are there on a tracer with a textured object
        only, the one whose `render` takes the entry that reads them: a tracer without one returns the nine values it always has.
        `photo_flag`: the table with OBJECT_PHOTO where an object carries it, for matpbr_path_render_objects_reflect alone; every other
        entry takes the table without it."""
        table, records = _table_ptrs(self.objects if photo_flag else _unflagged(self.objects), self.pbr)
        head, ltris, lcdf = self.lights if self.lights is not None else (None, None, None)
        return (table, len(self.objects) if self.objects is not None else 0, _dptr(self.obj_nrm), self.n_scene_tris, records,
                _ref(head) if head is not None else None, _dptr(ltris), _dptr(lcdf), _dptr(self.obj_col),
                *(self._texture_args() if self.textures is not None else ()))

    def _texture_args(self) -> tuple:
        """(obj_uv, texture records, texels, n_texels) as the C ABI takes them; (None, None, None, 0) without a textured object."""
        if self.textures is None:
            return None, None, None, 0
        uv, rec, texels = self.textures
        return (uv.data_ptr(), *_tex_ptrs(self.objects, rec, texels))

    def media_arg(self):
        """The PathObjectMedium records as the two entries with media take them, after the thirteen object arguments (and, in the
        differential family, the outputs); None on a tracer without a medium."""
        return ctypes.cast(self.media, _P) if self.media is not None else None

    def _render_entry(self, nrm) -> tuple:
        """(the entry point `render` takes, its own arguments after `stream`) ("The object entries").  A tracer with
        objects takes level 8 where a medium exists, else the entry of the first attribute it holds (not None, not False), from the
        textures down, else matpbr_path_render_objects; OBJECT_ENTRIES says how many of `object_args()` that entry takes."""
        if nrm is not None:
            return "matpbr_path_render_normals", (nrm.data_ptr(),)
        if self.objects is None:
            return "matpbr_path_render", ()
        if self.media is not None:
            return MEDIA_ENTRY, (*self.object_args()[:9], *self._texture_args(), self.media_arg())
        for attr, level in (("textures", "textures"), ("obj_col", "colors"), ("rough", "rough"), ("lights", "lights"), ("pbr", "pbr"), ("obj_nrm", "normals")):
            if getattr(self, attr) is not None and getattr(self, attr) is not False:
                entry = "matpbr_path_render_objects_" + level
                return entry, self.object_args()[:OBJECT_ENTRIES[entry]]
        return "matpbr_path_render_objects", self.object_args()[:2]

    def poses(self, transforms: Sequence[Optional[dict]]):
        """`move_objects`' argument checked, before any device work -> the PathXform records: one entry per object, each None or a
        placement `similarity` takes (the default pivot is the centre of the object's rest bounding box); every record one the library
        takes (`check_xforms`); every pose within `reach`.  ValueError otherwise, also on a tracer that is not movable."""
        if self._move is None:
            raise ValueError("move_objects needs a movable tracer: build the PathTracer with `objects` and movable=True")
        n = len(self.objects)
        if transforms is None or len(transforms) != n:
            raise ValueError(f"transforms must hold one entry per object ({n}), each a dict or None, got {None if transforms is None else len(transforms)}")
        boxes = self._move["boxes"]
        records = xform_records([similarity(tr, pivot=0.5 * (lo + hi)) for tr, (lo, hi) in zip(transforms, boxes)])
        check_xforms(records)
        for k, (x, (lo, hi)) in enumerate(zip(records, boxes)):
            sim = (np.array(x.R, np.float64).reshape(3, 3), float(x.s), np.array(x.t, np.float64), np.array(x.c, np.float64))
            far = pose_extent(sim, lo, hi)
            if not far <= self.reach:
                raise ValueError(f"the pose of object {k} reaches a coordinate of magnitude {far:.6g}, beyond this tracer's reach {self.reach:.6g}: "
                                 f"the boxes' padding was sized for it; build the PathTracer with reach={far:.6g} or more")
        return records

    @torch.no_grad()
    def move_objects(self, transforms: Sequence[Optional[dict]]) -> None:
        """Moves the inserted objects of a movable tracer ("Moving inserted objects"): `transforms` holds one entry
        per object, None for an object left at rest or {"scale": s, "rotate": 3 x 3 or {"axis": (x, y, z), "deg": a}, "translate": (x, y, z),
        "pivot": (x, y, z)}, every part optional: p' = R (s (p - pivot)) + pivot + translate, the pivot by default the centre of the
        object's rest bounding box.  Always from the rest pose the tracer was built with, never from the last pose.  Everything is
        checked first (`poses`); then the move and the refit of the object nodes are enqueued on the current stream and a light's area
        becomes (float)((double) area_rest s s).  A medium's coefficients stay per scene unit: an object scaled by s is optically s times
        thicker.  Every other method sees the moved scene from then on."""
        records = self.poses(transforms)
        mv, dev = self._move, self.device
        head, ltris = (None, None) if self.lights is None else self.lights[:2]
        n_obj = self.stats["n_object_tris"]
        if head is not None:
            rest = mv["rest_lights"]["header"]
            moved = PathLights.from_buffer_copy(rest)
            for l, area in enumerate(moved_light_areas(mv["rest_lights"], records)):
                moved.area[l] = area
            head = moved
        check(symbol("matpbr_path_objects_move")(
            self.nodes.data_ptr(), self.tris.data_ptr(), mv["rest_tris"].data_ptr(), self.n_scene_tris, n_obj, mv["first_object_node"],
            mv["n_object_nodes"], mv["node_level"].data_ptr(), mv["object_depth"], _table_ptrs(_uncolored(self.objects, 0))[0], len(self.objects),
            ctypes.cast(records, ctypes.c_void_p), mv["pad"], _dptr(mv["rest_nrm"]), _dptr(self.obj_nrm), _dptr(mv["rest_light_tris"]), _dptr(ltris),
            0 if ltris is None else int(ltris.shape[0]), None if head is None else _ref(head), torch.cuda.current_stream(dev).cuda_stream),
            "matpbr_path_objects_move")
        if head is not None:
            self.lights = (head, *self.lights[1:])

    @torch.no_grad()
    def render(self, albedo: torch.Tensor, roughness: torch.Tensor, metallic: torch.Tensor, envmap, spp: int = 64, max_depth: int = 4,
               seed: int = 0, spp_per_launch: int = 8, out: Optional[torch.Tensor] = None, rays: Optional[torch.Tensor] = None,
               tables: Optional[tuple] = None, normal=None) -> torch.Tensor:
        """-> linear radiance [H,W,3] on the current torch stream.  albedo [H,W,3], roughness / metallic [H,W] or [H,W,1], envmap
        [He,We,3] (tensor or array, the `sh.py` equirectangular convention).  Every split into launches of `spp_per_launch` samples gives
        the same bits.  `rays` (optional int32 [H,W] on the device): the rays each pixel traced are added to it.  `tables`: what
        `tables(envmap)` returned (default: built from `envmap` now).  `normal` [H,W,3] (unit length, used as given): the shading-normal
        map ("Shading normals"); None shades with the face normals.  A tracer with objects refuses it."""
        H, W, dev = self.H, self.W, self.device
        nrm = self._normal(normal, "render") if normal is not None else None
        inputs = self._inputs(albedo, roughness, metallic, envmap, tables)
        if out is None:
            out = torch.empty(H, W, 3, device=dev, dtype=torch.float32)
        lib = load()
        args = (*self._frame(*inputs, spp, max_depth, seed, spp_per_launch), out.data_ptr(), rays.data_ptr() if rays is not None else None,
                torch.cuda.current_stream(dev).cuda_stream)
        entry, own = self._render_entry(nrm)
        check(symbol(entry, lib)(*args, *own), entry)
        return out

    @torch.no_grad()
    def render_diff(self, albedo: torch.Tensor, roughness: torch.Tensor, metallic: torch.Tensor, envmap, spp: int = 64, max_depth: int = 4,
                    seed: int = 0, spp_per_launch: int = 8, tables: Optional[tuple] = None, rays: Optional[torch.Tensor] = None) -> tuple:
        """The differential render ("Differential render") with `render`'s arguments and random numbers ->
        (fg [H,W,3], delta [H,W,3], alpha [H,W], rewalked [H,W] int32) on the device, the first three means over `spp`.  fg: the radiance
        of the samples whose camera ray lands on an inserted object; alpha: their share; delta: what the objects add to and take from
        the other samples, the sample's radiance minus the same sample's walked again without the objects, over the samples whose first
        walk met an object (`rewalked` counts them; every sample that misses the objects, where the table holds a light).  Where
        rewalked is 0, delta is exactly 0.  `composite` puts them into a photograph.  Every split into launches gives the same bits.  A
        tracer without objects raises ValueError."""
        return self._render_diff("matpbr_path_render_objects_diff", (albedo, roughness, metallic, envmap), spp, max_depth, seed, spp_per_launch, tables, rays)

    def _render_diff(self, entry: str, maps, spp, max_depth, seed, spp_per_launch, tables, rays, photo=None, ratio=False) -> tuple:
        """`render_diff` through the library's `entry`; with `photo`, `render_diff_through`: the photograph and `through` follow the four
        outputs in the call, and `through` comes back before `rewalked`.  `ratio`: `render_diff_ratio`: the entry takes photo and
        through (NULL without `photo`) and then `base`, which comes back after `delta`."""
        if self.objects is None:
            raise ValueError(f"render_diff{'_ratio' if ratio else '' if photo is None else '_through'} renders what inserted objects change: "
                             f"build the PathTracer with `objects`")
        if photo is not None and tuple(torch.as_tensor(photo).shape) != (self.H, self.W, 3):
            raise ValueError(f"photo must be [{self.H},{self.W},3], got {tuple(torch.as_tensor(photo).shape)}")
        symbol(entry)                                 # a library built before the method's own feature: PathError naming it
        reflect = self.reflect and photo is not None  # a flagged object and a photograph: the one entry that sees the flag
        if reflect:
            entry = "matpbr_path_render_objects_reflect"
        elif self.media is not None:                  # the superset entry, only where a medium exists
            entry = "matpbr_path_render_objects_diff_media"
        fn = symbol(entry)
        H, W, dev = self.H, self.W, self.device
        own = () if photo is None else (torch.as_tensor(photo).to(dev, torch.float32).contiguous(), torch.empty(H, W, 3, device=dev, dtype=torch.float32))
        base = (torch.empty(H, W, 3, device=dev, dtype=torch.float32),) if ratio else ()
        inputs = self._inputs(*maps, tables)
        fg, delta = torch.empty(H, W, 3, device=dev, dtype=torch.float32), torch.empty(H, W, 3, device=dev, dtype=torch.float32)
        alpha, rewalked = torch.empty(H, W, device=dev, dtype=torch.float32), torch.zeros(H, W, device=dev, dtype=torch.int32)
        # the four outputs, then as many of (photo, through, base, media) as the entry takes, None where this call has none
        tail = (*map(_dptr, (fg, delta, alpha, rewalked, *(own or (None, None)), *(base or (None,)))), self.media_arg())[:4 + DIFF_ENTRIES[entry]]
        check(fn(*self._frame(*inputs, spp, max_depth, seed, spp_per_launch), _dptr(rays), torch.cuda.current_stream(dev).cuda_stream,
                 *self.object_args(reflect)[:9], *self._texture_args(), *tail), entry)
        return (fg, delta, *base, alpha, *own[1:], rewalked)

    @torch.no_grad()
    def render_diff_through(self, albedo: torch.Tensor, roughness: torch.Tensor, metallic: torch.Tensor, envmap, photo, spp: int = 64,
                            max_depth: int = 4, seed: int = 0, spp_per_launch: int = 8, tables: Optional[tuple] = None,
                            rays: Optional[torch.Tensor] = None) -> tuple:
        """`render_diff` with the photograph seen through inserted glass ("Seen through glass") ->
        (fg [H,W,3], delta [H,W,3], alpha [H,W], through [H,W,3], rewalked [H,W] int32).  `photo` [H,W,3]: the photograph, linear, finite
        and >= 0.  A sample whose camera ray lands on an object and leaves it through clear glass alone (smooth or flat dielectric
        vertices) onto the depth mesh's front adds throughput x photo at the landing point's texel to `through`; its fg is then what
        the objects change in the landing point's light (the sample minus its tail walked again without the objects, where that walk
        met one; nothing where it met none), and may be negative.  Rough glass, chains that end on another object, on a light, on the
        envmap or inside the glass at max_depth keep `render_diff`'s rule.  delta and alpha are `render_diff`'s bits; `rewalked`
        counts both kinds of second walk.  The picture is `composite(fg + through, delta, alpha, photo)`.  Every split into launches
        gives the same bits.  A tracer without objects, or a photograph of another shape, raises ValueError.  Where an object carries
        "photo": True ("Reflected in inserted objects") the chain also passes its vertices, which are not delta:
        fg then holds the light the chain itself gathered (emitter samples, the envmap, lights) besides the tail's difference, and
        `through` the photograph weighted by the chain's BSDF weights, noisy where the object is rough."""
        return self._render_diff("matpbr_path_render_objects_through", (albedo, roughness, metallic, envmap), spp, max_depth, seed, spp_per_launch,
                                 tables, rays, photo)

    @torch.no_grad()
    def render_diff_ratio(self, albedo: torch.Tensor, roughness: torch.Tensor, metallic: torch.Tensor, envmap, spp: int = 64, max_depth: int = 4,
                          seed: int = 0, spp_per_launch: int = 8, tables: Optional[tuple] = None, rays: Optional[torch.Tensor] = None,
                          photo=None) -> tuple:
        """`render_diff` that also keeps the radiance without the objects ("Ratio shadow transfer") ->
        (fg, delta, base [H,W,3], alpha, rewalked); with `photo` [H,W,3], `render_diff_through` with it -> (fg, delta, base, alpha,
        through, rewalked).  base: the mean over `spp` of the radiance without the objects of the samples whose camera ray misses
        them: the second walk's where a sample was walked twice, else its only walk's, which met no object (no further walk runs).
        base >= 0, exactly 0 where alpha = 1, and base + delta is the radiance with the objects of those samples.  The other outputs
        are `render_diff`'s (`render_diff_through`'s) bits.  `composite_ratio` puts them into a photograph.  Every split into launches
        gives the same bits.  A tracer without objects, or a photograph of another shape, raises ValueError."""
        return self._render_diff("matpbr_path_render_objects_ratio", (albedo, roughness, metallic, envmap), spp, max_depth, seed, spp_per_launch,
                                 tables, rays, photo, ratio=True)

    @torch.no_grad()
    def render_edit_diff(self, albedo: torch.Tensor, roughness: torch.Tensor, metallic: torch.Tensor, envmap, edited, mask=None, spp: int = 64,
                         max_depth: int = 4, seed: int = 0, spp_per_launch: int = 8, tables: Optional[tuple] = None,
                         rays: Optional[torch.Tensor] = None, normal=None) -> tuple:
        """The differential render of edited maps ("Material edits in the photograph") with `render`'s arguments
        and random numbers -> (delta [H,W,3], base [H,W,3], rewalked [H,W] int32) on the device, the first two means over `spp`.
        albedo, roughness, metallic: the fitted maps; `edited` = (a_e, r_e, m_e): the edited ones; `mask` [H,W] (non-zero = edited):
        where a vertex reads the edited maps, by default `edit_mask` of the two, the texels any of whose five floats differs.  A sample
        is walked on the edited maps inside the mask; where it read a masked texel it is walked again on the fitted maps alone, and
        delta takes the difference (`rewalked` counts those samples).  base: the fitted scene's radiance of every sample; base + delta:
        the edited scene's.  Where rewalked is 0, delta is exactly 0.  `composite_edit` puts them into a photograph.  `normal`: the
        shading-normal map of `render`, which is not edited.  Every split into launches gives the same bits.  A tracer with objects
        raises ValueError."""
        if self.objects is not None:
            raise ValueError("render_edit_diff knows no inserted objects: build the PathTracer without `objects`")
        if edited is None or len(edited) != 3:
            raise ValueError("edited must be the three edited maps (albedo, roughness, metallic)")
        H, W, dev = self.H, self.W, self.device
        if mask is not None and tuple(torch.as_tensor(mask).shape) != (H, W):
            raise ValueError(f"mask must be [{H},{W}], got {tuple(torch.as_tensor(mask).shape)}")
        fn = symbol("matpbr_path_render_edit_diff")
        nrm = self._normal(normal, "render_edit_diff") if normal is not None else None
        inputs = self._inputs(albedo, roughness, metallic, envmap, tables)
        ae, re, me = (torch.as_tensor(x).to(dev, torch.float32).reshape(H, W, c).contiguous() for x, c in zip(edited, (3, 1, 1)))
        mk = edit_mask(inputs[:3], (ae, re, me)) if mask is None else torch.as_tensor(mask) != 0
        mk = mk.to(dev, torch.uint8).contiguous()
        delta, base = torch.empty(H, W, 3, device=dev, dtype=torch.float32), torch.empty(H, W, 3, device=dev, dtype=torch.float32)
        rewalked = torch.zeros(H, W, device=dev, dtype=torch.int32)
        check(fn(*self._frame(*inputs, spp, max_depth, seed, spp_per_launch), _dptr(rays), torch.cuda.current_stream(dev).cuda_stream,
                 ae.data_ptr(), re.data_ptr(), me.data_ptr(), mk.data_ptr(), _dptr(nrm), delta.data_ptr(), base.data_ptr(), rewalked.data_ptr()),
              "matpbr_path_render_edit_diff")
        return delta, base, rewalked

    @torch.no_grad()
    def render_relight(self, albedo: torch.Tensor, roughness: torch.Tensor, metallic: torch.Tensor, envmap, new_envmap, spp: int = 64,
                       max_depth: int = 4, seed: int = 0, spp_per_launch: int = 8, tables: Optional[tuple] = None,
                       new_tables: Optional[tuple] = None, rays: Optional[torch.Tensor] = None, normal=None) -> tuple:
        """One walk under two environments ("Relighting in the photograph") with `render`'s arguments and random
        numbers -> (base [H,W,3], relit [H,W,3]) on the device, the means over `spp` of the radiance under `envmap` (the fitted light)
        and under `new_envmap` [He_b,We_b,3], which may have another size.  Each is what `render` gives under that envmap up to the
        rounding of its sums; the closest hits, the texels and the BSDF samples are computed once, and both estimators run on the same
        paths.  Where `new_envmap` has `envmap`'s values relit has base's bits.  `composite_relight` puts them into a photograph.
        `tables`, `new_tables`: what `tables(envmap)`, `tables(new_envmap)` returned (default: built now).  `rays`: the closest-hit
        rays once and each environment's shadow rays.  `normal`: the shading-normal map of `render`.  Every split into launches gives
        the same bits.  A tracer with objects raises ValueError."""
        if self.objects is not None:
            raise ValueError("render_relight knows no inserted objects: build the PathTracer without `objects`")
        H, W, dev = self.H, self.W, self.device
        fn = symbol("matpbr_path_render_relight")
        nrm = self._normal(normal, "render_relight") if normal is not None else None
        inputs = self._inputs(albedo, roughness, metallic, envmap, tables)
        env_b, row_b, col_b, pdf_b = self._inputs(*inputs[:3], new_envmap, new_tables)[3:]
        base, relit = torch.empty(H, W, 3, device=dev, dtype=torch.float32), torch.empty(H, W, 3, device=dev, dtype=torch.float32)
        check(fn(*self._frame(*inputs, spp, max_depth, seed, spp_per_launch), _dptr(rays), torch.cuda.current_stream(dev).cuda_stream,
                 env_b.data_ptr(), row_b.data_ptr(), col_b.data_ptr(), pdf_b.data_ptr(), int(env_b.shape[0]), int(env_b.shape[1]), _dptr(nrm),
                 base.data_ptr(), relit.data_ptr()), "matpbr_path_render_relight")
        return base, relit

    def _first_hit(self, entry: str, channels: int, hidden: int, *own) -> torch.Tensor:
        """[H,W,channels] on the device from the first-hit entry `entry`: it takes the BVH, the camera, the table without the flags
        `hidden` (`_uncolored`) and its count, its `own` arguments, the output and the stream."""
        out = torch.empty(self.H, self.W, channels, device=self.device, dtype=torch.float32)
        check(symbol(entry)(self.nodes.data_ptr(), self.tris.data_ptr(), self.H, self.W, self.fov, _table_ptrs(_uncolored(self.objects, hidden))[0],
                            len(self.objects) if self.objects is not None else 0, *own, out.data_ptr(),
                            torch.cuda.current_stream(self.device).cuda_stream), entry)
        return out

    @torch.no_grad()
    def features(self, normal=None) -> torch.Tensor:
        """geom [H,W,8] on the device: per pixel (p, rho) and (n, id) of the camera ray through the pixel centre, the denoiser's guides
        ("Denoiser").  n is the normal `render` shades that camera vertex with: `normal` [H,W,3] is the
        shading-normal map of `render` (a tracer with objects refuses it); id -1 = no hit, 0 = the depth mesh, 1 + k = object k."""
        nrm = self._normal(normal, "features") if normal is not None else None
        return self._first_hit("matpbr_path_features", 8, OBJECT_COLORED | OBJECT_TEXTURED, _dptr(self.obj_nrm), self.n_scene_tris, _dptr(nrm))

    @torch.no_grad()
    def feature_colors(self) -> torch.Tensor:
        """[H,W,3] on the device: the interpolated colour where the camera ray through the pixel centre (`features`' ray) first hits a
        vertex-coloured object, (1, 1, 1) elsewhere: what `relight.albedo_guide` multiplies a coloured object's constant by."""
        return self._first_hit("matpbr_path_feature_colors", 3, OBJECT_TEXTURED, self.n_scene_tris, _dptr(self.obj_col))

    @torch.no_grad()
    def feature_tints(self) -> torch.Tensor:
        """[H,W,3] on the device: the interpolated colour times the base-colour fetch where the camera ray through the pixel centre
        (`features`' ray) first hits a coloured or textured object, (1, 1, 1) elsewhere: `feature_colors` with the textures, what
        `relight.albedo_guide` multiplies a textured object's constant by."""
        return self._first_hit("matpbr_path_feature_tints", 3, 0, self.n_scene_tris, _dptr(self.obj_col), *self._texture_args())

    @torch.no_grad()
    def denoise(self, A, B, alb, geom, **params) -> torch.Tensor:
        """The a-trous filter over two half renders A, B [H,W,3] of this tracer (independent seeds, the same sample count), guided by
        the albedo alb [H,W,3] and `features()` -> the denoised mean [H,W,3].  `params`: levels, sigma_n, sigma_x, sigma_a, sigma_c
        (default DENOISE_DEFAULTS).  Forward only."""
        ws, to = self._filter_workspace(geom, "matpbr_path_denoise_workspace_bytes")
        return denoise(to(A), to(B), to(alb), to(geom), workspace=ws, **params)

    def _filter_workspace(self, geom, size: str) -> tuple:
        """(the filters' workspace, kept between calls and grown to what the library's `size` asks for this frame; the function that puts
        an image on this tracer's device) once `geom` is this frame's [H,W,8]."""
        if tuple(torch.as_tensor(geom).shape) != (self.H, self.W, 8):
            raise ValueError(f"geom must be [{self.H},{self.W},8], got {list(torch.as_tensor(geom).shape)}")
        nbytes = int(symbol(size)(self.H, self.W))
        if self._dn_ws is None or self._dn_ws.numel() < nbytes:
            self._dn_ws = torch.empty(nbytes, device=self.device, dtype=torch.uint8)
        return self._dn_ws, lambda x: x.to(self.device) if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x)).to(self.device)

    @torch.no_grad()
    def denoise_diff(self, A, B, alb, geom, scale: float = 1.0, **params) -> tuple:
        """The a-trous filter over two halves of `render_diff` ("Denoiser for the differential render"): A and B
        are (fg, delta, alpha) triples, each a sum over the same number of frames with independent seeds and equal spp, `scale` 1 / (the
        frames summed per half) -> (fg', delta', alpha'), which `composite(fg', delta', alpha', photo, 1.0)` puts into the photograph.
        Each pixel's own layer is filtered (fg where the camera ray through its centre lands on an object, delta elsewhere); the other
        layer and alpha pass through as their means.  `params`: `denoise`'s.  Forward only."""
        ws, to = self._filter_workspace(geom, "matpbr_path_denoise_diff_workspace_bytes")
        return denoise_diff(tuple(map(to, A)), tuple(map(to, B)), to(alb), to(geom), scale, workspace=ws, **params)

    @torch.no_grad()
    def render_trans(self, albedo: torch.Tensor, roughness: torch.Tensor, metallic: torch.Tensor, envmap, mask, bg, ior: float = 1.2,
                     spec_trans: float = 0.4, refract_distance: float = 100.0, spp: int = 64, max_depth: int = 4, seed: int = 0,
                     spp_per_launch: int = 8, tables: Optional[tuple] = None, rays: Optional[torch.Tensor] = None, normal=None) -> torch.Tensor:
        """`render` with the depth mesh shading as the reference's TransBSDF ("Transparency editing"): where
        `mask` [H,W] (bool) is set the surface is glass of index `ior` and transmission `spec_trans` over the picture `bg` [H,W,3].
        The maps are used as given (`relight.render_trans` edits them inside the mask first).  Forward only: there is no backward
        pass through it, a tracer with inserted objects refuses it, and it refuses a shading-normal map (`normal`)."""
        if normal is not None:
            raise ValueError("render_trans knows no shading normals: the transparency edit shades with the face normals")
        if self.objects is not None:
            raise ValueError("render_trans knows no inserted objects: build the PathTracer without `objects`")
        H, W, dev = self.H, self.W, self.device
        mk, bgt = torch.as_tensor(mask), torch.as_tensor(bg)
        if tuple(mk.shape) != (H, W):
            raise ValueError(f"mask must be [{H},{W}], got {tuple(mk.shape)}")
        if tuple(bgt.shape) != (H, W, 3):
            raise ValueError(f"bg must be [{H},{W},3], got {tuple(bgt.shape)}")
        ed = trans_edit(ior, spec_trans, refract_distance)
        mk = (mk != 0).to(dev, torch.uint8).contiguous()
        bgt = bgt.to(dev, torch.float32).contiguous()
        inputs = self._inputs(albedo, roughness, metallic, envmap, tables)
        out = torch.empty(H, W, 3, device=dev, dtype=torch.float32)
        check(load().matpbr_path_render_trans(*self._frame(*inputs, spp, max_depth, seed, spp_per_launch), out.data_ptr(),
                                              rays.data_ptr() if rays is not None else None, torch.cuda.current_stream(dev).cuda_stream,
                                              mk.data_ptr(), bgt.data_ptr(), _ref(ed)), "matpbr_path_render_trans")
        return out

    @torch.no_grad()
    def render_bwd(self, albedo: torch.Tensor, roughness: torch.Tensor, metallic: torch.Tensor, envmap, d_out: torch.Tensor, spp: int = 64,
                   max_depth: int = 4, seed: int = 0, spp_per_launch: int = 8, want=("a", "r", "m", "env"), grads: Optional[dict] = None,
                   tables: Optional[tuple] = None, rays: Optional[torch.Tensor] = None, normal=None) -> Dict[str, torch.Tensor]:
        """The backward pass of `render` with the same arguments: d loss / d {"a" [H,W,3], "r" [H,W,1], "m" [H,W,1], "env" [He,We,3]}
        for d_out = d loss / d render [H,W,3], for the keys in `want`.  The derivative of the fixed-seed estimator with the sampling
        detached; bit-identical for every `spp_per_launch`.  `grads`: device buffers to ADD to (by key; the
        missing ones start from zero).  `rays` (optional int32 [H,W]): the rays both replays traced are added to it.  `normal`: the
        shading-normal map of `render`; with it `want` may hold "n", d loss / d normal [H,W,3] with respect to the map's components as
        free variables (normalising is the caller's)."""
        if self.objects is not None:
            raise ValueError("render_bwd knows no inserted objects: build the PathTracer without `objects` for gradients")
        if "n" in want and normal is None:
            raise ValueError("want 'n' needs the shading-normal map it is the gradient of: pass `normal`")
        nrm = self._normal(normal, "render_bwd") if normal is not None else None
        H, W, dev = self.H, self.W, self.device
        inputs = self._inputs(albedo, roughness, metallic, envmap, tables)
        He, We = int(inputs[3].shape[0]), int(inputs[3].shape[1])
        d_out = torch.as_tensor(d_out).to(dev, torch.float32).reshape(H, W, 3).contiguous()
        shapes = {"a": (H, W, 3), "r": (H, W, 1), "m": (H, W, 1), "env": (He, We, 3), "n": (H, W, 3)}
        grads = dict(grads or {})
        for k in want:
            if k not in shapes:
                raise ValueError(f"want: keys of {tuple(shapes)}, got {k!r}")
            if k not in grads:
                grads[k] = torch.zeros(shapes[k], device=dev, dtype=torch.float32)
            g = grads[k]
            if tuple(g.shape) != shapes[k] or g.dtype != torch.float32 or not g.is_contiguous() or g.device.type != dev.type:
                raise ValueError(f"grads[{k!r}] must be contiguous float32 {shapes[k]} on {dev}")
        if "env" in want and He * We > MAX_BWD_ENV_TEXELS:
            raise ValueError(f"the envmap gradient needs He * We <= {MAX_BWD_ENV_TEXELS}, got {He} x {We}")
        lib = load()
        size = lib.matpbr_path_render_bwd_workspace_bytes if nrm is None else lib.matpbr_path_render_bwd_normals_workspace_bytes
        nbytes = int(size(H, W, He, We))
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, device=dev, dtype=torch.uint8)
        ptr = lambda k: grads[k].data_ptr() if k in want else None
        args = (*self._frame(*inputs, spp, max_depth, seed, spp_per_launch), d_out.data_ptr(), ptr("a"), ptr("r"), ptr("m"), ptr("env"),
                self._ws.data_ptr(), nbytes, rays.data_ptr() if rays is not None else None, torch.cuda.current_stream(dev).cuda_stream)
        if nrm is None:
            check(lib.matpbr_path_render_bwd(*args), "matpbr_path_render_bwd")
        else:
            check(lib.matpbr_path_render_bwd_normals(*args, nrm.data_ptr(), ptr("n")), "matpbr_path_render_bwd_normals")
        return {k: grads[k] for k in want}


class PathRenderFn(torch.autograd.Function):
    """out = PathTracer.render(a, r, m, env[, normal=nrm]) (bit for bit), differentiable in a [H,W,3], r [H,W,1], m [H,W,1], env
    [He,We,3] and the shading-normal map nrm [H,W,3] (None: face normals) by `render_bwd` with the forward's seed.  `ctx_in`:
    {"tracer", "spp", "max_depth", "seed", "spp_per_launch"} and the envmap-table cache `PathTables`."""

    @staticmethod
    def forward(ctx, a, r, m, env, ctx_in, nrm=None):
        tracer = ctx_in["tracer"]
        tabs = ctx_in["tables"].get(tracer, env)
        kw = {k: ctx_in[k] for k in ("spp", "max_depth", "seed", "spp_per_launch")}
        out = tracer.render(a.detach(), r.detach(), m.detach(), env.detach(), tables=tabs, normal=None if nrm is None else nrm.detach(), **kw)
        ctx.save_for_backward(a, r, m, env, *(() if nrm is None else (nrm,)))
        ctx.tracer, ctx.tabs, ctx.kw = tracer, tabs, kw
        return out

    @staticmethod
    def backward(ctx, d_out):
        a, r, m, env, *rest = ctx.saved_tensors
        nrm = rest[0] if rest else None
        need = ctx.needs_input_grad
        need = need[:4] + (bool(nrm is not None and need[5]),)
        want = [k for k, n in zip(("a", "r", "m", "env", "n"), need) if n]
        g = ctx.tracer.render_bwd(a.detach(), r.detach(), m.detach(), env.detach(), d_out, want=want, tables=ctx.tabs,
                                  normal=None if nrm is None else nrm.detach(), **ctx.kw) if want else {}
        return (g["a"].reshape(a.shape) if need[0] else None, g["r"].reshape(r.shape) if need[1] else None,
                g["m"].reshape(m.shape) if need[2] else None, g["env"].reshape(env.shape) if need[3] else None, None,
                g["n"].reshape(nrm.shape) if need[4] else None)


class PathTables:
    """The envmap's sampling tables, rebuilt only when the envmap tensor is another object or its version counter moved (an in-place
    optimiser step)."""

    def __init__(self):
        self._key, self._tabs = None, None

    def get(self, tracer: PathTracer, env: torch.Tensor) -> tuple:
        key = (env, env._version, tuple(env.shape))
        if self._key is None or self._key[0] is not env or self._key[1:] != key[1:]:
            self._tabs = tracer.tables(env.detach())
            self._key = key
        return self._tabs
