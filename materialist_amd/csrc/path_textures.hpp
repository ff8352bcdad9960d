// path_textures.hpp -- UV-textured inserted objects ("Textured inserted objects"; matpbr_path.hip includes it):
// the table the kernel takes by value, the texture coordinate at a hit, the bilinear fetch with repeat wrapping and the check of the
// caller's records.  The coordinate and the fetch are __host__ __device__, uncontracted apart from their explicit fmaf: the CPU entry
// points run what the kernel runs and give the same bits for the same u, v.
#pragma once
#include "path_lights.hpp"

namespace {
constexpr int kTexMaxSide = 8192;   // w, h of an image: first + w h stays far inside an int64, row * w + col inside an int32

// the table of a scene with a textured object: the superset table, the corner coordinates, the texels and one record per object
struct TexObjects : ColorObjects {
    const float* uv;        // [n_tri - n_scene_tri, 3, 2]: (s, t) per corner of every inserted triangle
    const float4* texels;   // all images one after another: linear (r, g, b, 0), row-major, row 0 the top row
    MatpbrPathObjectTex tex[MATPBR_PATH_MAX_OBJECTS];
};

// the record of the object whose range holds triangle `id` (all zero: none), by object_match's selects
__host__ __device__ inline MatpbrPathObjectTex tex_lookup(const ObjTable& ot, const MatpbrPathObjectTex* tex, int id) {
    MatpbrPathObjectTex r{};
    object_match(ot, id, [&](int k, const MatpbrPathObject&) { r = tex[k]; });
    return r;
}

// (s, t) = st0 + u (st1 - st0) + v (st2 - st0) for the corner coordinates cs = (s0, t0, s1, t1, s2, t2) and tri_uv's u, v:
// object_color's form without the clamp
__host__ __device__ inline void object_st(const float cs[6], float u, float v, float& s, float& t) {
    s = fmaf(v, cs[4] - cs[0], fmaf(u, cs[2] - cs[0], cs[0]));
    t = fmaf(v, cs[5] - cs[1], fmaf(u, cs[3] - cs[1], cs[1]));
}

// the fractional part of a finite coordinate in [0, 1): where s - floor(s) rounds to 1 (a tiny negative s), 0
__host__ __device__ inline float tex_frac(float s) {
    const float f = s - floorf(s);
    return f < 1.0f ? f : 0.0f;
}
// One axis of the fetch: the position x = f n - 0.5 among n texel centres -> the two texels i0, i1 wrapped into [0, n) (-1 becomes
// n - 1, n becomes 0) and the weight of i1.  f n <= n for every f in [0, 1] and n <= 8192, so floor(x) lies in {-1 .. n - 1}; the
// integer clamp keeps a fetch inside its image whatever x is.
__host__ __device__ inline void tex_axis(float f, int n, int& i0, int& i1, float& w) {
#pragma clang fp contract(off)
    const float x = f * (float)n - 0.5f, x0 = floorf(x);
    w = x - x0;
    int k = (int)x0;
    k = k < -1 ? -1 : k > n - 1 ? n - 1 : k;
    i0 = k < 0 ? n - 1 : k;
    i1 = k + 1 >= n ? 0 : k + 1;
}
// Bilinear filtering with `repeat` wrapping of the image of W x H texels that starts at img (Mitsuba's `bitmap` texture in outline; ours
// in detail): t = 0 is the image's bottom, texel centres lie at ((i + 0.5) / W, 1 - (j + 0.5) / H).  Four 16-byte loads issued together,
// then three explicit fmaf per channel and the clamp to [0, 1]: four equal texels give exactly their value.  A coordinate that is not
// finite gives (0, 0, 0).
__host__ __device__ inline void texture_fetch(const float4* img, int W, int H, float s, float t, float c[3]) {
#pragma clang fp contract(off)
    c[0] = c[1] = c[2] = 0.0f;
    if (!(fabsf(s) <= FLT_MAX) || !(fabsf(t) <= FLT_MAX)) return;
    int x0, x1, y0, y1;
    float fx, fy;
    tex_axis(tex_frac(s), W, x0, x1, fx);
    tex_axis(1.0f - tex_frac(t), H, y0, y1, fy);
    const float4 c00 = img[y0 * W + x0], c10 = img[y0 * W + x1], c01 = img[y1 * W + x0], c11 = img[y1 * W + x1];
    const float a00[3] = {c00.x, c00.y, c00.z}, a10[3] = {c10.x, c10.y, c10.z}, a01[3] = {c01.x, c01.y, c01.z}, a11[3] = {c11.x, c11.y, c11.z};
    for (int k = 0; k < 3; ++k) {
        const float top = fmaf(fx, a10[k] - a00[k], a00[k]), bot = fmaf(fx, a11[k] - a01[k], a01[k]);
        c[k] = fminf(fmaxf(fmaf(fy, bot - top, top), 0.0f), 1.0f);
    }
}
// both fetches of a record at (s, t): (1, 1, 1) for an image it does not have; the orm fetch follows the base fetch
__host__ __device__ inline void texture_fetch_record(const MatpbrPathObjectTex& r, const float4* texels, float s, float t, float base[3],
                                                     float orm[3]) {
    base[0] = base[1] = base[2] = 1.0f;
    orm[0] = orm[1] = orm[2] = 1.0f;
    if (r.base_w > 0) texture_fetch(texels + (long)r.base_first, r.base_w, r.base_h, s, t, base);
    if (r.orm_w > 0) texture_fetch(texels + (long)r.orm_first, r.orm_w, r.orm_h, s, t, orm);
}
// the roughness and the metallic of a PBR vertex under an orm fetch: glTF's factor times texture, with the project's roughness floor
__host__ __device__ inline void orm_apply(const float orm[3], float& r, float& m) {
    r = fminf(fmaxf(r * orm[1], 0.07f), 1.0f);
    m = fminf(fmaxf(m * orm[2], 0.0f), 1.0f);
}

// one image of a record against the texel buffer's length: w == 0 is "no such image"
bool tex_image_valid(int32_t first, int32_t w, int32_t h, long n_texels) {
    if (w == 0) return true;
    return w >= 1 && w <= kTexMaxSide && h >= 1 && h <= kTexMaxSide && first >= 0 && (long)first + (long)w * (long)h <= n_texels;
}
// the record of a flagged object: at least one image, orm on kind 3 only, every image inside the buffer, reserved zero
bool tex_valid(const MatpbrPathObjectTex& r, bool pbr, long n_texels) {
    if (r.reserved[0] != 0 || r.reserved[1] != 0 || (r.base_w == 0 && r.orm_w == 0) || (r.orm_w != 0 && !pbr)) return false;
    return tex_image_valid(r.base_first, r.base_w, r.base_h, n_texels) && tex_image_valid(r.orm_first, r.orm_w, r.orm_h, n_texels);
}
}  // namespace
