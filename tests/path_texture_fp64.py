"""The texture rule of the fp64 restatement of the path render ("Textured inserted objects"); the walk that
applies it, and the order of the rules, is `path_objects_fp64.replay_objects`.

  * An object of type "diffuse" or "pbr" may carry "uv" [Nv,2] with "texture" [h,w,3] (base colour, linear, in [0, 1], row 0 the top
    row) and, a pbr one, "orm_texture" [h,w,3]; the table entry holds the coordinates as the library does, one pair per triangle
    corner, rounded to fp32 ("corner_uv"), and the images rounded to fp32.
  * At a hit on such an object u, v are Moller-Trumbore's (`path_oi_smooth_fp64.barycentrics`), (s, t) = st0 + u (st1 - st0) +
    v (st2 - st0), and an image of W x H texels is read with bilinear filtering and repeat wrapping: fs = s - floor(s),
    x = fs W - 1/2, x0 = floor(x), fx = x - x0, columns x0 and x0 + 1 wrapped into [0, W); t = 0 is the image's bottom,
    y = (1 - ft) H - 1/2, the rows likewise; c = clip(top + fy (bot - top), 0, 1) with top, bot the two rows blended by fx.  A
    coordinate that is not finite reads (0, 0, 0).
  * diffuse: reflectance = p (.) c_vertex (.) c_base; pbr: albedo = a (.) c_vertex (.) c_base and, with an orm image whose fetch is
    (o, g, b), roughness = clip(r g, 0.07, 1), metallic = clip(m b, 0, 1).  A base-colour image changes no path; an orm image does.

With every image (1, 1, 1) the walk returns the bits of the table without textures.  No library code.

The record gains `textured_camera` [N,8] (the camera ray's first hit lies on textured object k), `textured_indirect` (a later vertex
ray lands on a textured object, whether max_depth lets it shade there or not), `fetch_wraps_columns` / `fetch_wraps_rows` (a fetch at a
shaded vertex paired column W - 1 with column 0, or row H - 1 with row 0) and `orm_roughness_floor` (a pbr vertex whose r g lies at or
below the 0.07 floor)."""
import numpy as np

import path_color_fp64 as pc
import path_light_fp64 as pl
import path_oi_fp64 as po
import path_oi_smooth_fp64 as ps

ROUGHNESS_FLOOR = 0.07


def texture_st(cs, u, v, dtype=np.float64):
    """(s, t) = st0 + u (st1 - st0) + v (st2 - st0) for corner coordinates cs [N,3,2] and barycentrics u, v [N] -> s [N], t [N]."""
    cs, u, v = np.asarray(cs, dtype), np.asarray(u, dtype), np.asarray(v, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        st = cs[:, 0] + u[:, None] * (cs[:, 1] - cs[:, 0]) + v[:, None] * (cs[:, 2] - cs[:, 0])
    return st[:, 0], st[:, 1]


def _axis(f, n, dtype):
    """One axis of the fetch: position f in [0, 1] among n texel centres -> (i0, i1 wrapped into [0, n), the weight of i1, wrapped)."""
    x = f * dtype(n) - dtype(0.5)
    x0 = np.floor(x)
    k = np.clip(x0.astype(np.int64), -1, n - 1)
    return k % n, (k + 1) % n, x - x0, (k < 0) | (k + 1 >= n)


def texture_fetch(img, s, t, dtype=np.float64):
    """The bilinear, repeat-wrapped read of img [h,w,3] (row 0 the top row) at (s, t) [N] -> (c [N,3] in [0, 1], the fetch paired
    column w - 1 with column 0 [N], row h - 1 with row 0 [N]).  `dtype=np.float32`: the same statements in fp32, each rounded once
    (the transcription the library's error is measured against)."""
    img = np.asarray(img, dtype)
    h, w = img.shape[:2]
    s, t = np.asarray(s, dtype), np.asarray(t, dtype)
    ok = np.isfinite(s) & np.isfinite(t)
    s, t = np.where(ok, s, dtype(0)), np.where(ok, t, dtype(0))
    fs, ft = s - np.floor(s), t - np.floor(t)
    fs, ft = np.where(fs < 1, fs, dtype(0)), np.where(ft < 1, ft, dtype(0))
    x0, x1, fx, wx = _axis(fs, w, dtype)
    y0, y1, fy, wy = _axis(dtype(1) - ft, h, dtype)
    fx, fy = fx[:, None], fy[:, None]
    top = img[y0, x0] + fx * (img[y0, x1] - img[y0, x0])
    bot = img[y1, x0] + fx * (img[y1, x1] - img[y1, x0])
    c = np.clip(top + fy * (bot - top), 0, 1)
    return np.where(ok[:, None], c, dtype(0)).astype(dtype), wx & ok, wy & ok


# ---- the shared test scenes ----------------------------------------------------------------------------------------------------------
TEX_SPHERE = pc.COLOR_SPHERE                                        # `path_color_fp64`'s coloured sphere's place
TEX_CUBE = pc.COLOR_CUBE                                            # its coloured cube's
BOTH_CUBE = ((0.27, 0.07, -1.25), 0.1, (0.3, 0.2, 0.0))            # a vertex-coloured and textured diffuse cube, right of the sphere
PLAIN_CUBE = pc.PLAIN_CUBE
CLEAR_SPHERE = pc.CLEAR_SPHERE
PBR_BASE = {"type": "pbr", "albedo": (0.9, 0.8, 0.7), "roughness": 0.5, "metallic": 0.6}
DIFFUSE_BASE = pc.DIFFUSE_BASE


def image(h, w, seed, lo=0.0):
    """A random image [h,w,3] of fp32 values in [lo, 1], with a texel at lo and one at 1 among them."""
    A = lo + (1 - lo) * np.random.default_rng(seed).random((h, w, 3))
    A[0, 0], A[-1, -1] = lo, 1.0
    return A.astype(np.float32).astype(np.float64)


def orm_image():
    """3 x 2 (w x h) texels: g drives the roughness of PBR_BASE (0.5) to the 0.07 floor in four of them, b scales the metallic."""
    A = image(2, 3, 33, 0.2)
    A[0, :, 1] = (0.0, 0.1, 0.05)
    A[1, 1, 1] = 0.0
    return A.astype(np.float32).astype(np.float64)


def sphere_uv(V, centre):
    """Latitude-longitude coordinates of a sphere's vertices scaled by 2.5 and shifted by -1.3: both seams and negative values occur."""
    n = (V - np.asarray(centre)) / np.linalg.norm(V - np.asarray(centre), axis=-1, keepdims=True)
    st = np.stack([np.arctan2(n[:, 0], n[:, 2]) / (2 * np.pi) + 0.5, np.arccos(np.clip(n[:, 1], -1, 1)) / np.pi], -1)
    return (2.5 * st - 1.3).astype(np.float32).astype(np.float64)


def cube_uv(V, seed, scale=1.7):
    """Per-vertex coordinates of a cube that cross the seams: random in [-scale, scale]."""
    return ((np.random.default_rng(seed).random((len(V), 2)) * 2 - 1) * scale).astype(np.float32).astype(np.float64)


def table_scene(uniform=False, flagged=True):
    """The GPU parity scene's table, in front of a depth mesh at z <= -1.6: a smooth diffuse icosphere with a 5 x 4 texture, a flat PBR
    cube with a 2 x 3 base image and a 3 x 2 orm image, a vertex-coloured and textured diffuse cube, an untextured diffuse cube and a
    clear-glass icosphere.  `uniform`: every image (1, 1, 1); `flagged=False`: the same table without textures (the colours stay)."""
    Vs, Ts, Ns = ps.icosphere(*TEX_SPHERE, 1)
    Vc, Tc = po.cube(*TEX_CUBE)
    Vb, Tb = po.cube(*BOTH_CUBE)
    Vd, Td = po.cube(*PLAIN_CUBE)
    Vg, Tg, Ng = ps.icosphere(*CLEAR_SPHERE, 1)
    out = [{"vertices": Vs, "triangles": Ts, "bsdf": DIFFUSE_BASE, "normals": Ns},
           {"vertices": Vc, "triangles": Tc, "bsdf": PBR_BASE},
           {"vertices": Vb, "triangles": Tb, "bsdf": po.DIFFUSE_08, "colors": pc.vertex_colors(Vb, 23)},
           {"vertices": Vd, "triangles": Td, "bsdf": po.DIFFUSE_08},
           {"vertices": Vg, "triangles": Tg, "bsdf": po.GLASS, "normals": Ng}]
    if flagged:
        one = lambda h, w: np.ones((h, w, 3))
        out[0].update(uv=sphere_uv(Vs, TEX_SPHERE[0]), texture=one(4, 5) if uniform else image(4, 5, 31))
        out[1].update(uv=cube_uv(Vc, 41), texture=one(3, 2) if uniform else image(3, 2, 32), orm_texture=one(2, 3) if uniform else orm_image())
        out[2].update(uv=cube_uv(Vb, 42), texture=one(2, 2) if uniform else image(2, 2, 34))
    return out


def corner_uv(ob):
    """The object's "uv" as the library stores it: one pair per triangle corner, rounded to fp32; None without coordinates."""
    if ob.get("uv") is None:
        return None
    return np.asarray(ob["uv"], np.float64)[np.asarray(ob["triangles"], np.int64)].astype(np.float32).astype(np.float64)


# the closed form in expectation: `path_light_fp64.furnace_scene`'s box around a camera-facing diffuse quad at constant depth whose
# (s, t) are affine in position and stay inside the texel centres' hull, and whose 5 x 4 texels are affine in their indices: there the
# bilinear fetch is the affine function itself
FURNACE_QUAD = ((0.0, 0.0, -1.2), 0.25)                             # centre, half side
FURNACE_P = (0.9, 0.8, 0.7)
FURNACE_WH = (5, 4)


def furnace_st(x):
    """(s, t) [..., 2] of a point of the quad: affine in x, y, inside [0.5 / w, 1 - 0.5 / w] x [0.5 / h, 1 - 0.5 / h] on the quad."""
    w, h = FURNACE_WH
    c, half = np.asarray(FURNACE_QUAD[0]), FURNACE_QUAD[1]
    q = (np.asarray(x, np.float64)[..., :2] - c[:2]) / (2 * half) + 0.5      # [0, 1]^2 over the quad
    return np.stack([0.5 / w + q[..., 0] * (1 - 1.0 / w), 0.5 / h + q[..., 1] * (1 - 1.0 / h)], -1)


def furnace_texels():
    """[h,w,3], affine in the column i and in the row j counted from the bottom: T = A + B i + C j per channel, inside [0, 1]."""
    w, h = FURNACE_WH
    i, j = np.meshgrid(np.arange(w), (h - 1) - np.arange(h))       # row 0 is the top row
    A, B, C = np.array([0.1, 0.8, 0.3]), np.array([0.2, -0.15, 0.05]), np.array([0.02, -0.05, 0.15])
    return (A + B * i[..., None] + C * j[..., None]).astype(np.float32).astype(np.float64)


def furnace_value(s, t):
    """T(s, t) [..., 3]: the affine function the texels sample, x = s w - 1/2 columns from the left, y = t h - 1/2 rows from the bottom."""
    w, h = FURNACE_WH
    tx = furnace_texels()
    A, B, C = tx[h - 1, 0], tx[h - 1, 1] - tx[h - 1, 0], tx[h - 2, 0] - tx[h - 1, 0]
    return A + B * (np.asarray(s)[..., None] * w - 0.5) + C * (np.asarray(t)[..., None] * h - 0.5)


def furnace_scene():
    """-> the objects: the emitting box and the textured diffuse quad facing the camera."""
    Vb, Tb = pl.box(*pl.FURNACE_BOX, inward=True)
    (cx, cy, cz), half = FURNACE_QUAD
    Vq = np.array([[cx - half, cy - half, cz], [cx + half, cy - half, cz], [cx + half, cy + half, cz], [cx - half, cy + half, cz]])
    Vq = Vq.astype(np.float32).astype(np.float64)
    Tq = np.array([[0, 1, 2], [0, 2, 3]], np.int32)                # outward normal +z: towards the camera
    quad = {"vertices": Vq, "triangles": Tq, "bsdf": {"type": "diffuse", "reflectance": FURNACE_P}, "uv": furnace_st(Vq),
            "texture": furnace_texels()}
    return [{"vertices": Vb, "triangles": Tb, "bsdf": {"type": "area", "radiance": pl.FURNACE_L}}, quad]
