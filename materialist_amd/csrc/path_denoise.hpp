// path_denoise.hpp -- the denoiser of libmatpbr_path.so (matpbr_path.hip includes it; DESIGN.md section 1.4, "Denoiser"): first-hit
// features and a variance-guided edge-avoiding a-trous filter.
// The spatial part of SVGF (Schied et al. 2017) over the a-trous wavelet of Dammertz et al. 2010, the variance from two half
// buffers (Rousselle et al. 2012), the guides noise-free features of the camera ray through the pixel centre.  Forward only, no
// atomics: the bits are the same from run to run.  The per-pixel bodies are __host__ __device__: the *_host entry points run what
// the kernels run (the device takes its exponentials and reciprocals from the hardware's approximations, the CPU from libm).
#pragma once
#include "path_textures.hpp"

namespace {
constexpr int kDnTileX = 32, kDnTileY = 8;   // the filter's workgroup: 256 lanes, a wave = two rows of 32 pixels (512 B of cv each)
constexpr int kDnMaxLevels = 8;

__host__ __device__ inline float dn_lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }   // matpbr_path_env_tables' weights
__host__ __device__ inline float dn_exp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __expf(x);
#else
    return expf(x);
#endif
}
__host__ __device__ inline float dn_rcp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(x);
#else
    return 1.0f / x;
#endif
}
// max(0, c)^sigma as exp2(sigma log2 c), 0 where c <= 0 (or is not a number)
__host__ __device__ inline float dn_pow(float c, float sigma) {
    if (!(c > 0.0f)) return 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_exp2f(sigma * __log2f(c));
#else
    return exp2f(sigma * log2f(c));
#endif
}

struct FeatArgs {
    const float4* nodes;
    const float4* tris;
    const float* obj_nrm;   // nullable: corner normals of the inserted triangles (smooth objects)
    const float* nrm_map;   // nullable: the shading-normal map of the depth mesh
    float4* geom;           // [H,W,2]
    int H, W;
    int32_t n_scene_tri;
    float f_pix, cx, cy, f_ndc, aspect;
    float rho_scale;        // 2 tan(fov_x / 2) / W: the footprint of a pixel at distance 1
};

// The features of the camera ray through the centre of pixel (i, j): g0 = (p, rho), g1 = (n, id).  n is the normal the forward
// kernel shades that camera vertex with: the depth mesh's camera-side face normal or its map's texel, an object's face normal or,
// where it is smooth, smooth_normal + smooth_side.
template <class Stack>
__host__ __device__ inline void features_pixel(const FeatArgs& q, const ObjTable& ot, int i, int j, Stack& stk, float4& g0, float4& g1) {
    const float o[3] = {0.0f, 0.0f, 0.0f};
    float d[3] = {((float)j - q.cx) / q.f_pix, -((float)i - q.cy) / q.f_pix, -1.0f};
    {
        const float il = 1.0f / sqrtf(dot3s(d, d));   // the same bits on the device and on the CPU: see trace_strict
        for (int c = 0; c < 3; ++c) d[c] *= il;
    }
    float t = FLT_MAX;
    const int k = trace_strict(q.nodes, q.tris, o, d, 0.0f, t, stk);
    if (k < 0) {
        g0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        g1 = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
        return;
    }
    const float4 A = q.tris[3 * k], B = q.tris[3 * k + 1], C = q.tris[3 * k + 2];
    const float v0[3] = {A.x, A.y, A.z}, e1[3] = {B.x, B.y, B.z}, e2[3] = {C.x, C.y, C.z};
    float n[3];
    cross3(e1, e2, n);
    {
        const float il = 1.0f / sqrtf(dot3h(n, n));
        for (int c = 0; c < 3; ++c) n[c] *= il;
    }
    int32_t id;
    __builtin_memcpy(&id, &A.w, 4);
    // the hit point on the winning triangle's plane, (n . v0) / (n . d) along the ray from the origin: without the cancellation of
    // Moller-Trumbore's t, which the traversal only needs for ordering (n . d != 0: the triangle test refuses det == 0)
    t = dot3h(n, v0) / dot3h(n, d);
    const float p[3] = {t * d[0], t * d[1], t * d[2]};
    const int obj = object_index(ot, id);
    if (obj < 0) {
        if (q.nrm_map) {
            const long tp = screen_texel(p, q.f_ndc, q.aspect, q.H, q.W);
            for (int c = 0; c < 3; ++c) n[c] = q.nrm_map[3 * tp + c];
        }
    } else if (ot.o[obj].kind & MATPBR_PATH_OBJECT_SMOOTH) {
        const float* cp = q.obj_nrm + 9 * (long)(id - q.n_scene_tri);
        const float wo[3] = {-d[0], -d[1], -d[2]};
        float cn[9], bu, bv, ns[3];
        for (int c = 0; c < 9; ++c) cn[c] = cp[c];
        tri_uv(v0, e1, e2, o, d, bu, bv);
        smooth_normal(cn, bu, bv, n, ns);
        smooth_side(n, wo, ns);
        for (int c = 0; c < 3; ++c) n[c] = ns[c];
    }
    g0 = make_float4(p[0], p[1], p[2], sqrtf(dot3h(p, p)) * q.rho_scale);
    g1 = make_float4(n[0], n[1], n[2], (float)(obj + 1));
}

__global__ __launch_bounds__(kBlock) void features_kernel(const FeatArgs q, const ObjTable ot) {
    __shared__ int s_stack[kStack * kBlock];
    const int tid = threadIdx.y * kTileX + threadIdx.x;
    const int j = blockIdx.x * kTileX + threadIdx.x, i = blockIdx.y * kTileY + threadIdx.y;
    if (i >= q.H || j >= q.W) return;   // no barriers below: each lane's stack column is its own
    LdsStack stk{s_stack + tid};
    float4 g0, g1;
    features_pixel(q, ot, i, j, stk, g0, g1);
    float4* gp = q.geom + 2 * ((long)i * q.W + j);
    gp[0] = g0;
    gp[1] = g1;
}

// ---- the colour guide ("Vertex-coloured inserted objects") -------------------------------------------------
struct FeatColorArgs {
    const float4* nodes;
    const float4* tris;
    const float* obj_col;   // nullable: corner colours of the inserted triangles (coloured objects)
    float* out;             // [H,W,3]
    int H, W;
    int32_t n_scene_tri;
    float f_pix, cx, cy;
};
// the tint guide's textures ("Textured inserted objects"): a trailing argument that the colour guide does not have
struct FeatTextures {
    const float* uv;        // nullable: corner coordinates of the inserted triangles (textured objects)
    const float4* texels;
    MatpbrPathObjectTex tex[MATPBR_PATH_MAX_OBJECTS];
};
// c *= the base-colour fetch of the textured object that holds triangle `id` (slot = id - n_scene_tri) at the hit u, v
__host__ __device__ inline void feature_texture(const FeatTextures& tx, const ObjTable& ot, int id, int slot, float u, float v, float c[3]) {
    const MatpbrPathObjectTex r = tex_lookup(ot, tx.tex, id);
    const float* up = tx.uv + 6 * (long)slot;
    float cs[6], s, t, base[3];
    for (int n = 0; n < 6; ++n) cs[n] = up[n];
    object_st(cs, u, v, s, t);
    base[0] = base[1] = base[2] = 1.0f;
    if (r.base_w > 0) texture_fetch(tx.texels + (long)r.base_first, r.base_w, r.base_h, s, t, base);
    for (int n = 0; n < 3; ++n) c[n] *= base[n];
}
// features_pixel's ray and traversal: c = the interpolated colour where the first hit lies on a coloured object, (1, 1, 1) elsewhere.
// With FeatTextures the colour is multiplied by the base-colour fetch where the object is textured; without, every `if (TEX ...)` folds
// away.
template <class Stack, class... Tex>
__host__ __device__ inline void feature_colors_pixel(const FeatColorArgs& q, const ObjTable& ot, int i, int j, Stack& stk, float c[3],
                                                     const Tex&... tx) {
    constexpr bool TEX = sizeof...(Tex) != 0;
    const float o[3] = {0.0f, 0.0f, 0.0f};
    float d[3] = {((float)j - q.cx) / q.f_pix, -((float)i - q.cy) / q.f_pix, -1.0f};
    {
        const float il = 1.0f / sqrtf(dot3s(d, d));
        for (int k = 0; k < 3; ++k) d[k] *= il;
    }
    c[0] = c[1] = c[2] = 1.0f;
    float t = FLT_MAX;
    const int k = trace_strict(q.nodes, q.tris, o, d, 0.0f, t, stk);
    if (k < 0) return;
    const float4 A = q.tris[3 * k], B = q.tris[3 * k + 1], C = q.tris[3 * k + 2];
    int32_t id;
    __builtin_memcpy(&id, &A.w, 4);
    const int obj = object_index(ot, id);
    if (obj < 0 || !(ot.o[obj].kind & (TEX ? MATPBR_PATH_OBJECT_COLORED | MATPBR_PATH_OBJECT_TEXTURED : MATPBR_PATH_OBJECT_COLORED))) return;
    const float v0[3] = {A.x, A.y, A.z}, e1[3] = {B.x, B.y, B.z}, e2[3] = {C.x, C.y, C.z};
    float bu, bv;
    tri_uv_strict(v0, e1, e2, o, d, bu, bv);
    if (!TEX || (ot.o[obj].kind & MATPBR_PATH_OBJECT_COLORED)) {
        const float* cp = q.obj_col + 9 * (long)(id - q.n_scene_tri);
        float cc[9];
        for (int n = 0; n < 9; ++n) cc[n] = cp[n];
        object_color(cc, bu, bv, c);
    }
    if constexpr (TEX) {
        if (ot.o[obj].kind & MATPBR_PATH_OBJECT_TEXTURED) feature_texture(tx..., ot, id, id - q.n_scene_tri, bu, bv, c);
    }
}

__global__ __launch_bounds__(kBlock) void feature_colors_kernel(const FeatColorArgs q, const ObjTable ot) {
    __shared__ int s_stack[kStack * kBlock];
    const int tid = threadIdx.y * kTileX + threadIdx.x;
    const int j = blockIdx.x * kTileX + threadIdx.x, i = blockIdx.y * kTileY + threadIdx.y;
    if (i >= q.H || j >= q.W) return;   // no barriers below: each lane's stack column is its own
    LdsStack stk{s_stack + tid};
    float c[3];
    feature_colors_pixel(q, ot, i, j, stk, c);
    float* op = q.out + 3 * ((long)i * q.W + j);
    op[0] = c[0]; op[1] = c[1]; op[2] = c[2];
}

// the tint guide: feature_colors_kernel with the textures
__global__ __launch_bounds__(kBlock) void feature_tints_kernel(const FeatColorArgs q, const ObjTable ot, const FeatTextures tx) {
    __shared__ int s_stack[kStack * kBlock];
    const int tid = threadIdx.y * kTileX + threadIdx.x;
    const int j = blockIdx.x * kTileX + threadIdx.x, i = blockIdx.y * kTileY + threadIdx.y;
    if (i >= q.H || j >= q.W) return;   // no barriers below: each lane's stack column is its own
    LdsStack stk{s_stack + tid};
    float c[3];
    feature_colors_pixel(q, ot, i, j, stk, c, tx);
    float* op = q.out + 3 * ((long)i * q.W + j);
    op[0] = c[0]; op[1] = c[1]; op[2] = c[2];
}

// prepare: cv0 = ((A + B) / 2, v0), v0 the 3 x 3 binomial average of (lum(A) - lum(B))^2 / 4 over the taps inside the image that
// carry the pixel's id, normalised by the weights used
__host__ __device__ inline float4 dn_prepare_pixel(const float* __restrict__ A, const float* __restrict__ B, const float4* __restrict__ geom, int H,
                                                   int W, int i, int j) {
    const long p = (long)i * W + j;
    const float idp = geom[2 * p + 1].w;
    float sv = 0.0f, sw = 0.0f;
    for (int di = -1; di <= 1; ++di) {
        for (int dj = -1; dj <= 1; ++dj) {
            const int qi = i + di, qj = j + dj;
            const bool in = qi >= 0 && qi < H && qj >= 0 && qj < W;
            const long q = in ? (long)qi * W + qj : p;   // a tap outside reads the centre and weighs nothing
            const float dl = dn_lum(A[3 * q], A[3 * q + 1], A[3 * q + 2]) - dn_lum(B[3 * q], B[3 * q + 1], B[3 * q + 2]);
            const float w = in && geom[2 * q + 1].w == idp ? (float)((2 - (di < 0 ? -di : di)) * (2 - (dj < 0 ? -dj : dj))) : 0.0f;
            sv += w * (dl * dl * 0.25f);
            sw += w;
        }
    }
    return make_float4(0.5f * (A[3 * p] + B[3 * p]), 0.5f * (A[3 * p + 1] + B[3 * p + 1]), 0.5f * (A[3 * p + 2] + B[3 * p + 2]), sv / sw);
}

// one a-trous level at stride s: the 5 x 5 taps p + s (di, dj), the centre with weight 9/64, every other tap with
// h h [id_q == id_p] w_n w_x w_a w_c.  The centre's guides stay in registers; a tap outside the image reads
// the centre's records and weighs nothing (no branch).  -> (sum w c / sum w, sum w^2 v / (sum w)^2)
//
// COV (the differential render's filter, "Denoiser for the differential render"): every tap weight, the centre's included, is
// multiplied by the tap's coverage cov[q], the colour term's relative part takes |lum(c_p)|, and a pixel without coverage is
// (0, 0, 0, 0).  Off, every `if constexpr (COV)` folds away and `cov` is not read.
template <bool COV = false>
__host__ __device__ inline float4 dn_level_pixel(const float4* __restrict__ cv, const float4* __restrict__ geom, const float* __restrict__ alb, int H,
                                                 int W, int i, int j, int s, const MatpbrPathDenoise& prm, const float* __restrict__ cov = nullptr) {
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const long p = (long)i * W + j;
    const float4 cp = cv[p], xp = geom[2 * p], np_ = geom[2 * p + 1];
    const float ap[3] = {alb[3 * p], alb[3 * p + 1], alb[3 * p + 2]};
    const float lp = dn_lum(cp.x, cp.y, cp.z);
    const bool geo = np_.w != -1.0f;   // a pixel that hit nothing has no normal and no position to compare
    float kp = 1.0f;
    if constexpr (COV) {
        kp = cov[p];
        if (!(kp > 0.0f)) return make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    const float inv_c = 1.0f / (prm.sigma_c * sqrtf(fmaxf(cp.w, 0.0f)) + 1e-3f * (COV ? fabsf(lp) : lp) + 1e-30f);
    const float inv_a = 1.0f / (prm.sigma_a * prm.sigma_a);
    const float xs = prm.sigma_x * xp.w * (float)s;
    const float w0 = COV ? (h[2] * h[2]) * kp : h[2] * h[2];
    float sw = w0, sc[3] = {w0 * cp.x, w0 * cp.y, w0 * cp.z}, sv = (w0 * w0) * cp.w;
#pragma unroll
    for (int di = -2; di <= 2; ++di) {
#pragma unroll
        for (int dj = -2; dj <= 2; ++dj) {
            if (di == 0 && dj == 0) continue;
            const int qi = i + s * di, qj = j + s * dj;
            const bool in = qi >= 0 && qi < H && qj >= 0 && qj < W;
            const long q = in ? (long)qi * W + qj : p;
            const float4 cq = cv[q], xq = geom[2 * q], nq = geom[2 * q + 1];
            const float da[3] = {ap[0] - alb[3 * q], ap[1] - alb[3 * q + 1], ap[2] - alb[3 * q + 2]};
            float e = (da[0] * da[0] + da[1] * da[1] + da[2] * da[2]) * inv_a + fabsf(lp - dn_lum(cq.x, cq.y, cq.z)) * inv_c;
            float wn = 1.0f;
            if (geo) {
                wn = dn_pow(np_.x * nq.x + np_.y * nq.y + np_.z * nq.z, prm.sigma_n);
                const float dist = fabsf(np_.x * (xq.x - xp.x) + np_.y * (xq.y - xp.y) + np_.z * (xq.z - xp.z));
                e += dist * dn_rcp(xs * sqrtf((float)(di * di + dj * dj)) + 1e-30f);
            }
            float w = in && nq.w == np_.w ? (h[di + 2] * h[dj + 2]) * wn * dn_exp(-e) : 0.0f;
            if constexpr (COV) w *= cov[q];
            sw += w;
            sc[0] += w * cq.x; sc[1] += w * cq.y; sc[2] += w * cq.z;
            sv += (w * w) * cq.w;
        }
    }
    const float iw = 1.0f / sw;
    return make_float4(sc[0] * iw, sc[1] * iw, sc[2] * iw, sv * (iw * iw));
}

__global__ __launch_bounds__(kDnTileX * kDnTileY) void denoise_prepare_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                                             const float4* __restrict__ geom, int H, int W, float4* __restrict__ cv0) {
    const int j = blockIdx.x * kDnTileX + threadIdx.x, i = blockIdx.y * kDnTileY + threadIdx.y;
    if (i >= H || j >= W) return;
    cv0[(long)i * W + j] = dn_prepare_pixel(A, B, geom, H, W, i, j);
}

// `rgb`: 0 writes (c, v) to cv_out[H,W,4]; 1 writes c to rgb_out[H,W,3] (the last level of the chain).  One kernel for both, so the
// chain's last level runs the instructions the separate call runs.
__global__ __launch_bounds__(kDnTileX * kDnTileY) void denoise_level_kernel(const float4* __restrict__ cv, const float4* __restrict__ geom,
                                                                           const float* __restrict__ alb, int H, int W, int s,
                                                                           const MatpbrPathDenoise prm, float4* __restrict__ cv_out,
                                                                           float* __restrict__ rgb_out, int rgb) {
    const int j = blockIdx.x * kDnTileX + threadIdx.x, i = blockIdx.y * kDnTileY + threadIdx.y;
    if (i >= H || j >= W) return;
    const float4 r = dn_level_pixel(cv, geom, alb, H, W, i, j, s, prm);
    const long p = (long)i * W + j;
    if (rgb) {
        rgb_out[3 * p] = r.x; rgb_out[3 * p + 1] = r.y; rgb_out[3 * p + 2] = r.z;
    } else {
        cv_out[p] = r;
    }
}

// ---- the differential render's filter ("Denoiser for the differential render") ---------------------------------
// Two halves of matpbr_path_render_objects_diff's sums.  A pixel's own layer is the object layer (id >= 1: signal fg, coverage the mean
// alpha) or the scene layer (id 0 or -1: signal delta, coverage 1 - the mean alpha); the filter runs over the own layer's signal divided
// by its coverage, with the coverage as every tap's confidence, and `finish` multiplies the coverage back.
struct DiffHalves {
    const float* fgA; const float* deltaA; const float* alphaA;
    const float* fgB; const float* deltaB; const float* alphaB;
};
// the mean alpha of a pixel, (0.5 (alphaA + alphaB)) scale, and from it the own layer's coverage; each operation rounded on its own, so
// the device and the CPU agree on which pixels have none
__host__ __device__ inline float dd_alpha(const DiffHalves& x, long p, float scale) {
#pragma clang fp contract(off)
    return (0.5f * (x.alphaA[p] + x.alphaB[p])) * scale;
}
__host__ __device__ inline float dd_coverage(float abar, bool object) {
#pragma clang fp contract(off)
    return object ? abar : fmaxf(0.0f, 1.0f - abar);
}

// prepare: cv0 = ((X_A + X_B) / 2 g, v0) with g = scale / coverage, v0 dn_prepare_pixel's average of (lum(X_A) - lum(X_B))^2 / 4 g_q^2
// over the taps that also have coverage; a pixel without coverage is (0, 0, 0, 0) and no quotient is formed for it.  -> its coverage
__host__ __device__ inline float dd_prepare_pixel(const DiffHalves& x, const float4* __restrict__ geom, int H, int W, int i, int j, float scale,
                                                  float4& cv0) {
    const long p = (long)i * W + j;
    const float idp = geom[2 * p + 1].w;
    const bool object = idp >= 1.0f;
    const float* __restrict__ A = object ? x.fgA : x.deltaA;
    const float* __restrict__ B = object ? x.fgB : x.deltaB;
    const float kp = dd_coverage(dd_alpha(x, p, scale), object);
    cv0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!(kp > 0.0f)) return 0.0f;
    float sv = 0.0f, sw = 0.0f;
    for (int di = -1; di <= 1; ++di) {
        for (int dj = -1; dj <= 1; ++dj) {
            const int qi = i + di, qj = j + dj;
            const bool in = qi >= 0 && qi < H && qj >= 0 && qj < W;
            const long q = in ? (long)qi * W + qj : p;   // a tap outside reads the centre and weighs nothing
            const float kq = dd_coverage(dd_alpha(x, q, scale), object);
            const bool use = in && geom[2 * q + 1].w == idp && kq > 0.0f;
            const float g = use ? scale / kq : 0.0f;
            const float dl = dn_lum(A[3 * q], A[3 * q + 1], A[3 * q + 2]) - dn_lum(B[3 * q], B[3 * q + 1], B[3 * q + 2]);
            const float w = use ? (float)((2 - (di < 0 ? -di : di)) * (2 - (dj < 0 ? -dj : dj))) : 0.0f;
            sv += w * ((dl * dl * 0.25f) * (g * g));
            sw += w;
        }
    }
    const float gp = scale / kp;
    cv0 = make_float4((0.5f * (A[3 * p] + B[3 * p])) * gp, (0.5f * (A[3 * p + 1] + B[3 * p + 1])) * gp, (0.5f * (A[3 * p + 2] + B[3 * p + 2])) * gp,
                      sv / sw);
    return kp;
}

// finish: the own layer's filtered colour times its coverage; the other layer's mean and the mean alpha pass through
__host__ __device__ inline void dd_finish_pixel(const float4* cv, const float* cov, const DiffHalves& x, const float4* geom, long p, float scale,
                                                float* fg, float* delta, float* alpha) {
    const bool object = geom[2 * p + 1].w >= 1.0f;
    const float4 c = cv[p];
    const float k = cov[p];
    const float own[3] = {k * c.x, k * c.y, k * c.z};
    for (int n = 0; n < 3; ++n) {
        const float mf = (0.5f * (x.fgA[3 * p + n] + x.fgB[3 * p + n])) * scale, md = (0.5f * (x.deltaA[3 * p + n] + x.deltaB[3 * p + n])) * scale;
        fg[3 * p + n] = object ? own[n] : mf;
        delta[3 * p + n] = object ? md : own[n];
    }
    alpha[p] = dd_alpha(x, p, scale);
}

__global__ __launch_bounds__(kDnTileX * kDnTileY) void denoise_diff_prepare_kernel(const DiffHalves x, const float4* __restrict__ geom, int H, int W,
                                                                                  float scale, float4* __restrict__ cv0, float* __restrict__ cov) {
    const int j = blockIdx.x * kDnTileX + threadIdx.x, i = blockIdx.y * kDnTileY + threadIdx.y;
    if (i >= H || j >= W) return;
    float4 r;
    const float k = dd_prepare_pixel(x, geom, H, W, i, j, scale, r);
    cv0[(long)i * W + j] = r;
    cov[(long)i * W + j] = k;
}

// denoise_level_kernel's second instantiation of dn_level_pixel
__global__ __launch_bounds__(kDnTileX * kDnTileY) void denoise_diff_level_kernel(const float4* __restrict__ cv, const float* __restrict__ cov,
                                                                                const float4* __restrict__ geom, const float* __restrict__ alb, int H,
                                                                                int W, int s, const MatpbrPathDenoise prm, float4* __restrict__ cv_out) {
    const int j = blockIdx.x * kDnTileX + threadIdx.x, i = blockIdx.y * kDnTileY + threadIdx.y;
    if (i >= H || j >= W) return;
    cv_out[(long)i * W + j] = dn_level_pixel<true>(cv, geom, alb, H, W, i, j, s, prm, cov);
}

__global__ __launch_bounds__(kDnTileX * kDnTileY) void denoise_diff_finish_kernel(const float4* cv, const float* cov, const DiffHalves x,
                                                                                 const float4* geom, int H, int W, float scale, float* fg, float* delta,
                                                                                 float* alpha) {
    const int j = blockIdx.x * kDnTileX + threadIdx.x, i = blockIdx.y * kDnTileY + threadIdx.y;
    if (i >= H || j >= W) return;
    dd_finish_pixel(cv, cov, x, geom, (long)i * W + j, scale, fg, delta, alpha);
}

inline bool diff_halves_valid(const DiffHalves& x) { return x.fgA && x.deltaA && x.alphaA && x.fgB && x.deltaB && x.alphaB; }
inline bool diff_scale_valid(float scale) { return std::isfinite(scale) && scale > 0.0f; }

bool denoise_params_valid(const MatpbrPathDenoise* prm) {
    if (!prm || prm->levels < 1 || prm->levels > kDnMaxLevels) return false;
    for (float s : {prm->sigma_n, prm->sigma_x, prm->sigma_a, prm->sigma_c})
        if (!(s > 0.0f && std::isfinite(s))) return false;
    return true;
}
bool denoise_size_valid(int H, int W) { return H > 0 && W > 0 && (long)H * W <= INT32_MAX / 8; }
dim3 denoise_grid(int H, int W) { return dim3((unsigned)((W + kDnTileX - 1) / kDnTileX), (unsigned)((H + kDnTileY - 1) / kDnTileY)); }
}  // namespace
