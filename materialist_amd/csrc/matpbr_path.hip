// matpbr_path.hip -- libmatpbr_path.so: the path-traced re-render of the depth mesh (include/matpbr_path.h).
//
//   * host: a binned-SAH BVH2 over the mesh's triangles (every node holds both children's boxes, so one 64-byte node read tests
//     two boxes), triangles stored in leaf order as precomputed (v0, e1, e2); the envmap's importance-sampling tables (fp64 -> fp32);
//   * device: one thread per pixel loops over its samples in order and accumulates them in a fixed order (no atomics: the image is
//     bit-reproducible, and so is every split of a frame into launches); the traversal stack lives in LDS, one column per lane;
//   * the closest-hit routine and the emitter sampler are __host__ __device__: the CPU entry points run the same code as the kernel;
//   * backward (matpbr_path_render_bwd): path replay with the sampling detached, 64-bit fixed-point sums (see "backward pass" below).
// The BRDF arithmetic is matpbr_device.hpp's (pixel_const, brdf_core, ggx_den_stable, frame, to_world), unchanged.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/matpbr_path.h"
#include "matpbr_device.hpp"

using namespace matpbr;

namespace {

constexpr int kMaxBvhDepth = MATPBR_PATH_MAX_BVH_DEPTH;
constexpr int kStack = kMaxBvhDepth;   // at most one pushed sibling per inner level of the path from the root
constexpr int kLeafMax = 4;            // triangles per leaf the builder aims for
constexpr int kBins = 16;              // SAH bins per axis
constexpr int kTileX = 16, kTileY = 8; // one workgroup = a 16 x 8 pixel tile (a wave = 16 x 4): neighbouring rays share nodes
constexpr int kBlock = kTileX * kTileY;
constexpr int kDims = 16;              // random dimensions reserved per path vertex (RNG counter layout below)

// ---- node / triangle layout ------------------------------------------------------------------------------------------------
// node = 4 x float4: box0 lo, box0 hi, box1 lo, box1 hi (12 floats), then child[2], count[2] as int.  count < 0: the child is the
// inner node `child`; count >= 0: a leaf of triangles [child, child + count) (count 0 = an empty slot, only a root's).
struct BNode {
    float b[12];
    int32_t child[2];
    int32_t count[2];
};
static_assert(sizeof(BNode) == MATPBR_PATH_NODE_BYTES, "node layout");
static_assert(3 * sizeof(float4) == MATPBR_PATH_TRI_BYTES, "triangle layout");

__host__ __device__ inline float dot3h(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__host__ __device__ inline void cross3(const float a[3], const float b[3], float c[3]) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// slab test of one box: entry distance in `tn`; the exit distance is widened by 2 ulp-ish so that rounding never culls a box
// the triangle test would hit
__host__ __device__ inline bool box_hit(float lx, float ly, float lz, float hx, float hy, float hz, const float inv[3], const float oi[3],
                                        float tmin, float tmax, float& tn) {
    const float ax = lx * inv[0] - oi[0], bx = hx * inv[0] - oi[0];
    const float ay = ly * inv[1] - oi[1], by = hy * inv[1] - oi[1];
    const float az = lz * inv[2] - oi[2], bz = hz * inv[2] - oi[2];
    const float t0 = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), tmin));
    const float t1 = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fminf(fmaxf(az, bz), tmax)) * 1.0000004f;
    tn = t0;
    return t0 <= t1;
}

// Moller-Trumbore on (v0, e1, e2); updates t / k where tmin < t' < t
__host__ __device__ inline void tri_test(const float4* tris, int k, const float o[3], const float d[3], float tmin, float& t, int& hit) {
    const float4 A = tris[3 * k], B = tris[3 * k + 1], C = tris[3 * k + 2];
    const float e1[3] = {B.x, B.y, B.z}, e2[3] = {C.x, C.y, C.z};
    float pv[3];
    cross3(d, e2, pv);
    const float det = dot3h(e1, pv);
    if (det == 0.0f) return;
    const float idet = 1.0f / det;
    const float tv[3] = {o[0] - A.x, o[1] - A.y, o[2] - A.z};
    const float u = dot3h(tv, pv) * idet;
    if (!(u >= 0.0f && u <= 1.0f)) return;
    float qv[3];
    cross3(tv, e1, qv);
    const float v = dot3h(d, qv) * idet;
    if (!(v >= 0.0f && u + v <= 1.0f)) return;
    const float tt = dot3h(e2, qv) * idet;
    if (tt > tmin && tt < t) { t = tt; hit = k; }
}

// Closest hit (ANY = false) or any hit (ANY = true, shadow rays) of the ray o + t d, tmin < t < t_in.  Returns the leaf-order index
// of the triangle hit (-1: none) and its distance in t.  `stk` is the traversal stack (kStack entries): LDS on the device, an
// array on the host.  Pushes beyond kStack are dropped: only a BVH deeper than the builder makes could reach that.
template <bool ANY, class Stack>
__host__ __device__ inline int trace(const float4* __restrict__ nodes, const float4* __restrict__ tris, const float o[3], const float d[3],
                                     float tmin, float& t, Stack& stk) {
    float inv[3], oi[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float dc = fabsf(d[c]) < 1e-30f ? copysignf(1e-30f, d[c]) : d[c];
        inv[c] = 1.0f / dc;
        oi[c] = o[c] * inv[c];
    }
    int hit = -1, node = 0, sp = 0;
    while (true) {
        const float4* np = nodes + 4 * node;
        const float4 q0 = np[0], q1 = np[1], q2 = np[2], q3f = np[3];
        const int4 q3 = *reinterpret_cast<const int4*>(&q3f);
        float tn0, tn1;
        bool h0 = box_hit(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, inv, oi, tmin, t, tn0);
        bool h1 = box_hit(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, inv, oi, tmin, t, tn1);
        if (h0 && q3.z >= 0) {
            for (int k = q3.x, e = q3.x + q3.z; k < e; ++k) tri_test(tris, k, o, d, tmin, t, hit);
            h0 = false;
            if (ANY && hit >= 0) return hit;
        }
        if (h1 && q3.w >= 0) {
            for (int k = q3.y, e = q3.y + q3.w; k < e; ++k) tri_test(tris, k, o, d, tmin, t, hit);
            h1 = false;
            if (ANY && hit >= 0) return hit;
        }
        if (h0 && h1) {
            const bool first0 = tn0 <= tn1;
            node = first0 ? q3.x : q3.y;
            if (sp < kStack) stk[sp++] = first0 ? q3.y : q3.x;
        } else if (h0) {
            node = q3.x;
        } else if (h1) {
            node = q3.y;
        } else {
            if (sp == 0) break;
            node = stk[--sp];
        }
    }
    return hit;
}

struct HostStack {
    int s[kStack];
    int& operator[](int i) { return s[i]; }
};
struct LdsStack {  // entry i of this lane at p[i * kBlock]: the 64 lanes of a wave hit 64 consecutive words (no bank conflicts)
    int* p;
    __device__ int& operator[](int i) { return p[i * kBlock]; }
};

// ---- RNG: the PCG hash (Jarzynski & Olano 2020, "Hash Functions for GPU Rendering"), chained over the counter ---------------
// u(seed, pixel, sample, vertex, dim) = (h >> 8) * 2^-24,  h = pcg(pcg(pcg(pcg(seed) + pixel) + sample) + vertex * 16 + dim)
// (uint32 arithmetic throughout; tests/path_fp64.py restates it in numpy)
__host__ __device__ inline uint32_t pcg_hash(uint32_t v) {
    const uint32_t s = v * 747796405u + 2891336453u;
    const uint32_t w = ((s >> ((s >> 28u) + 4u)) ^ s) * 277803737u;
    return (w >> 22u) ^ w;
}
__host__ __device__ inline float rng_u(uint32_t base, int vertex, int dim) {
    return (float)(pcg_hash(base + (uint32_t)(vertex * kDims + dim)) >> 8) * 5.9604644775390625e-8f;
}
// dims of a vertex: 0-1 pixel jitter (vertex 0), 2-5 emitter sample (row, column, cos theta, phi), 6-8 BSDF sample (lobe, u0, u1)

// ---- envmap: equirectangular, theta = acos(y), phi = atan2(x, -z) in [0, 2 pi) (materialist_amd/sh.py) --------------------
__host__ __device__ inline int env_texel(const float d[3], int He, int We) {
    const float kPiF = 3.14159265358979323846f;
    const float th = acosf(fminf(fmaxf(d[1], -1.0f), 1.0f));
    float ph = atan2f(d[0], -d[2]);
    if (ph < 0.0f) ph += 2.0f * kPiF;
    const int row = std::min(std::max((int)(th * ((float)He / kPiF)), 0), He - 1);
    const int col = std::min(std::max((int)(ph * ((float)We / (2.0f * kPiF))), 0), We - 1);
    return row * We + col;
}
// largest i in [0, n) with cdf[i] <= u (cdf[0] = 0, cdf[n] = 1): zero-weight entries are never returned
__host__ __device__ inline int cdf_find(const float* cdf, int n, float u) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] <= u) lo = mid; else hi = mid;
    }
    return lo;
}
// emitter sample: texel by luminance x solid angle (row from the marginal, column from the row's conditional), then uniform in
// cos theta and phi inside the texel's cell.  Returns the texel; dir / pdf (solid angle) written.
__host__ __device__ inline int env_sample(const float* row_cdf, const float* col_cdf, const float* pdf_tab, int He, int We, float u0, float u1,
                                          float u2, float u3, float dir[3], float& pdf) {
    const float kPiF = 3.14159265358979323846f;
    const int row = cdf_find(row_cdf, He, u0);
    const int col = cdf_find(col_cdf + (long)row * (We + 1), We, u1);
    const float c0 = cosf((float)row * (kPiF / (float)He)), c1 = cosf((float)(row + 1) * (kPiF / (float)He));
    const float ct = c0 + (c1 - c0) * u2;
    const float st = sqrtf(fmaxf(1.0f - ct * ct, 0.0f));
    const float ph = ((float)col + u3) * (2.0f * kPiF / (float)We);
    const float sp = sinf(ph), cp = cosf(ph);
    dir[0] = st * sp; dir[1] = ct; dir[2] = -st * cp;
    pdf = pdf_tab[row * We + col];
    return row * We + col;
}

// ---- BSDF: MatDiffBSDF.eval_brdf / sample_brdf (myutils/mi_plugin.py:1296-1341,1372-1427) ------------------------------------
// These restate matpbr_kernels.hip's lane_setup and the sampler inside sample_brdf_kernel (the same formulas, the same
// matpbr_device.hpp helpers).  They are copied rather than shared because moving them into a header would change the sources
// build.sources_digest() hashes (and with it the traffic profile bench.py checks); tests/test_gpu_path.py pins them against the
// fp64 oracle's sample_brdf / eval_brdf.
struct PLane {
    PixelConst<float> pc;
    float NoL_raw, NoH, VoH, den;
};
__device__ __forceinline__ void path_lane(PLane& ln, const float wi[3], const float wo[3], const float n[3], const float a[3], float r, float m) {
    float h[3] = {wi[0] + wo[0], wi[1] + wo[1], wi[2] + wo[2]};
    const float il = rsq(dot3(h, h));
#pragma unroll
    for (int c = 0; c < 3; ++c) h[c] *= il;
    pixel_const<float>(ln.pc, a, r, m, dot3(n, wo));
    ln.NoL_raw = dot3(n, wi);
    ln.VoH = fmaxf(dot3(wo, h), 0.0f);
    const float nh_raw = dot3(n, h);
    ln.NoH = fmaxf(nh_raw, 0.0f);
    const float nn = dot3(n, n);
    if (fabsf(nn - 1.0f) < 1e-5f && nh_raw > 0.0f) {
        const float cx = n[1] * h[2] - n[2] * h[1], cy = n[2] * h[0] - n[0] * h[2], cz = n[0] * h[1] - n[1] * h[0];
        ln.den = ggx_den_stable(ln.pc, fmaf(cx, cx, fmaf(cy, cy, cz * cz)));
    } else {
        ln.den = ggx_den_literal(ln.pc, ln.NoH);
    }
}
// path_lane's h and n . h before its clamp (the same operations): the normal's gradient reads them (shading normals, backward)
__device__ __forceinline__ float half_vector(const float wi[3], const float wo[3], const float n[3], float h[3]) {
    h[0] = wi[0] + wo[0]; h[1] = wi[1] + wo[1]; h[2] = wi[2] + wo[2];
    const float il = rsq(dot3(h, h));
#pragma unroll
    for (int c = 0; c < 3; ++c) h[c] *= il;
    return dot3(n, h);
}
// eval_brdf(wi, wo) -> f (RGB, with the trailing cosine) and the mixture pdf
__device__ __forceinline__ void path_eval(const float wi[3], const float wo[3], const float n[3], const float a[3], float r, float m, float f[3],
                                          float& pdf) {
    PLane ln;
    path_lane(ln, wi, wo, n, a, r, m);
    BrdfState<float> st;
    brdf_core(ln.pc, ln.NoL_raw, ln.NoH, ln.VoH, ln.den, st, f, pdf);
}
// path_eval keeping what the backward pass needs (brdf_core_grad reads the lane constants and the state)
__device__ __forceinline__ void path_eval_st(const float wi[3], const float wo[3], const float n[3], const float a[3], float r, float m, PLane& ln,
                                             BrdfState<float>& st, float f[3], float& pdf) {
    path_lane(ln, wi, wo, n, a, r, m);
    brdf_core(ln.pc, ln.NoL_raw, ln.NoH, ln.VoH, ln.den, st, f, pdf);
}
// sample_brdf's direction and the BSDF value / mixture pdf there (f and p before the weight is formed; ln / st for the backward pass)
__device__ __forceinline__ void path_sample_st(float sample1, float u0, float u1, const float wo[3], const float n[3], const float a[3], float r,
                                               float m, float wi[3], PLane& ln, BrdfState<float>& st, float f[3], float& p) {
    float s[3], t[3];
    frame(n, s, t);
    float sp, cp;
    sincosf(2.0f * kPi * u1, &sp, &cp);
    float sin2_h = -1.0f, cos_h = 0.0f;
    if (sample1 > 0.5f) {  // diffuse lobe (mi_plugin.py:1328-1329)
        const float st_ = fsqrt(fmaxf(u0, 0.0f)), ct = fsqrt(fmaxf(1.0f - u0, 0.0f));
        to_world(s, t, n, st_ * cp, st_ * sp, ct, wi);
    } else {  // GGX lobe (mi_plugin.py:1330-1331)
        const float alpha2 = pow4(r);
        const float q = rcp(fmaf(u0, alpha2 - 1.0f, 1.0f));
        const float ct = fsqrt(fmaxf((1.0f - u0) * q, 0.0f)), st_ = fsqrt(fmaxf(u0 * alpha2 * q, 0.0f));
        float wh[3];
        to_world(s, t, n, st_ * cp, st_ * sp, ct, wh);
        const float d = 2.0f * dot3(wo, wh);
#pragma unroll
        for (int c = 0; c < 3; ++c) wi[c] = fmaf(d, wh[c], -wo[c]);
        const float il = rsq(dot3(wi, wi));
#pragma unroll
        for (int c = 0; c < 3; ++c) wi[c] *= il;
        if (d > 0.0f) { sin2_h = u0 * alpha2 * q; cos_h = ct; }
    }
    path_lane(ln, wi, wo, n, a, r, m);
    if (sin2_h >= 0.0f) {  // same value as the literal form, without the fp32 cancellation at the GGX peak
        ln.NoH = cos_h;
        ln.den = ggx_den_stable(ln.pc, sin2_h);
    }
    brdf_core(ln.pc, ln.NoL_raw, ln.NoH, ln.VoH, ln.den, st, f, p);
}
// sample_brdf: lobe by sample1 > 0.5 (diffuse) else GGX; weight = f/(pdf + 1e-6) where pdf > 1e-6, else 0
__device__ __forceinline__ void path_sample(float sample1, float u0, float u1, const float wo[3], const float n[3], const float a[3], float r,
                                            float m, float wi[3], float w[3], float& pdf_out) {
    PLane ln;
    BrdfState<float> st;
    float f[3], p;
    path_sample_st(sample1, u0, u1, wo, n, a, r, m, wi, ln, st, f, p);
    const float ip = p > 1e-6f ? 1.0f / (p + 1e-6f) : 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) w[c] = f[c] * ip;
    pdf_out = p > 0.0f ? p : 0.0f;
}

// power heuristic (Mitsuba 3 path: mis_weight), 0 where it is not finite
__device__ __forceinline__ float mis_weight(float a, float b) {
    const float a2 = a * a, w = a2 / (a2 + b * b);
    return isfinite(w) ? w : 0.0f;
}

// ---- inserted objects ("Inserted objects"): Mitsuba's smooth `dielectric` and `diffuse` ------------------
// The table travels to the kernel by value.  An id (the triangle's index in the input mesh) in no range is the depth mesh's.
struct ObjTable {
    MatpbrPathObject o[MATPBR_PATH_MAX_OBJECTS];
    int32_t n, min_id;   // min_id: the smallest first_tri, below which no lookup is needed
};
struct NoObjects {};   // the kernel's table when there is none
constexpr int kFlagDelta = 1, kFlagTransmitted = 2;

// kind and parameters of triangle `id` (0: the depth mesh).  Unrolled selects over wave-uniform table reads: no indexed private array.
__device__ __forceinline__ int object_of(const NoObjects&, int, float[3]) { return 0; }
__device__ __forceinline__ int object_of(const ObjTable& ot, int id, float p[3]) {
    int kind = 0;
    if (id < ot.min_id) return kind;
#pragma unroll
    for (int k = 0; k < MATPBR_PATH_MAX_OBJECTS; ++k) {
        const MatpbrPathObject& ob = ot.o[k];
        if (k < ot.n && id >= ob.first_tri && id - ob.first_tri < ob.n_tri) {
            kind = ob.kind;
            p[0] = ob.p[0]; p[1] = ob.p[1]; p[2] = ob.p[2];
        }
    }
    return kind;
}

// exact unpolarised Fresnel reflectance of a smooth dielectric: cos_i = |n . wo|, eta_it = n_transmitted side / n_incident side;
// cos_t written (0 at total internal reflection, where R = 1)
__host__ __device__ inline float fresnel_dielectric(float cos_i, float eta_it, float& cos_t) {
    const float eta_ti = 1.0f / eta_it;
    const float cos_t2 = 1.0f - (eta_ti * eta_ti) * (1.0f - cos_i * cos_i);
    if (!(cos_t2 > 0.0f)) { cos_t = 0.0f; return 1.0f; }
    cos_t = sqrtf(cos_t2);
    const float a_s = (cos_i - eta_it * cos_t) / (cos_i + eta_it * cos_t);
    const float a_p = (cos_t - eta_it * cos_i) / (cos_t + eta_it * cos_i);
    return 0.5f * (a_s * a_s + a_p * a_p);
}

// BSDF sample of an inserted object at a vertex with the outward face normal n and the direction wo towards the viewer; u_lobe, u0,
// u1 = dims 6, 7, 8.  -> wi, weight = f cos / pdf (0: the path ends), pdf, flags.
//   dielectric: u_lobe <= R reflects about n (weight 1), else refracts by Snell with weight eta_ti^2 (radiance transport; Mitsuba's
//     `dielectric`); pdf = the probability of the event chosen.  Both sides shade: n . wo > 0 enters, < 0 leaves.
//   diffuse: one-sided, cosine-weighted about n (sin^2 = u0, phi = 2 pi u1, the frame of Duff et al. 2017), pdf = cos / pi, weight rho.
__host__ __device__ inline void object_sample(int kind, const float p[3], const float n[3], const float wo[3], float u_lobe, float u0, float u1,
                                              float wi[3], float w[3], float& pdf, int& flags) {
    const float cos_o = dot3h(n, wo);
    if (kind == MATPBR_PATH_BSDF_DIELECTRIC) {
        const float eta = p[0] / p[1];
        const bool entering = cos_o > 0.0f;
        const float eta_it = entering ? eta : 1.0f / eta, eta_ti = entering ? 1.0f / eta : eta;
        const float ci = fabsf(cos_o);
        float ct;
        const float R = fresnel_dielectric(ci, eta_it, ct);
        if (u_lobe <= R) {
            for (int c = 0; c < 3; ++c) wi[c] = 2.0f * cos_o * n[c] - wo[c];
            w[0] = w[1] = w[2] = 1.0f;
            pdf = R;
            flags = kFlagDelta;
        } else {
            const float s = (entering ? 1.0f : -1.0f) * (eta_ti * ci - ct);   // along the normal on wo's side
            for (int c = 0; c < 3; ++c) wi[c] = s * n[c] - eta_ti * wo[c];
            w[0] = w[1] = w[2] = eta_ti * eta_ti;
            pdf = 1.0f - R;
            flags = kFlagDelta | kFlagTransmitted;
        }
        return;
    }
    flags = 0;
    if (!(cos_o > 0.0f)) {   // seen from inside
        wi[0] = wi[1] = wi[2] = 0.0f;
        w[0] = w[1] = w[2] = 0.0f;
        pdf = 0.0f;
        return;
    }
    const float st = sqrtf(fmaxf(u0, 0.0f)), ct = sqrtf(fmaxf(1.0f - u0, 0.0f));
    const float ph = 6.28318530717958647692f * u1;
    const float x = st * cosf(ph), y = st * sinf(ph);
    const float sg = copysignf(1.0f, n[2]), a = -1.0f / (sg + n[2]), b = n[0] * n[1] * a;
    const float s[3] = {1.0f + sg * n[0] * n[0] * a, sg * b, -sg * n[0]}, t[3] = {b, sg + n[1] * n[1] * a, -n[1]};
    for (int c = 0; c < 3; ++c) wi[c] = s[c] * x + t[c] * y + n[c] * ct;
    for (int c = 0; c < 3; ++c) w[c] = p[c];
    pdf = ct * 0.31830988618379067154f;
}

// ---- smooth inserted objects ("Smooth inserted objects") --------------------------------------------------
// An object whose kind carries MATPBR_PATH_OBJECT_SMOOTH shades with its corner normals interpolated at the hit point; the face
// normal ng keeps everything geometric.  The table, the corner normals (one per corner of every inserted triangle, in input order,
// indexed by id - n_scene_tri) and n_scene_tri travel to the kernel by value.  Interpolation, the fallbacks and the redo are
// __host__ __device__ (plain divisions and sqrtf): the CPU entry points run what the kernel runs.
struct SmoothObjects {
    ObjTable t;
    const float* nrm;   // [n_tri - n_scene_tri, 3, 3]
    int32_t n_scene_tri;
};
// object_of for the smooth table: the kind still carries the flag bit
__device__ __forceinline__ int object_of(const SmoothObjects& so, int id, float p[3]) { return object_of(so.t, id, p); }

// ---- PBR inserted objects ("PBR inserted objects") --------------------------------------------------------
// An object of kind MATPBR_PATH_BSDF_PBR shades as the depth mesh does, MatDiffBSDF, on the constants of its record instead of a
// texel's.  MatpbrPathObject is frozen, so the eight records travel to the kernel by value beside the smooth table.
struct PbrObjects : SmoothObjects {
    MatpbrPathObjectPbr pbr[MATPBR_PATH_MAX_OBJECTS];
};
// object_of for that table: kind (with its flag bit) and p as above; a, r, m written where the object is of kind 3 and left alone
// elsewhere.  The same unrolled selects over wave-uniform reads.  __host__ __device__: matpbr_path_object_lookup_host runs it.
__host__ __device__ inline int object_lookup(const ObjTable& ot, const MatpbrPathObjectPbr* pbr, int id, float p[3], float a[3], float& r, float& m) {
    int kind = 0;
    if (id < ot.min_id) return kind;
#pragma unroll
    for (int k = 0; k < MATPBR_PATH_MAX_OBJECTS; ++k) {
        const MatpbrPathObject& ob = ot.o[k];
        if (k < ot.n && id >= ob.first_tri && id - ob.first_tri < ob.n_tri) {
            kind = ob.kind;
            p[0] = ob.p[0]; p[1] = ob.p[1]; p[2] = ob.p[2];
            if ((ob.kind & ~MATPBR_PATH_OBJECT_SMOOTH) == MATPBR_PATH_BSDF_PBR) {
                a[0] = pbr[k].a[0]; a[1] = pbr[k].a[1]; a[2] = pbr[k].a[2];
                r = pbr[k].r;
                m = pbr[k].m;
            }
        }
    }
    return kind;
}

// Moller-Trumbore's u, v of the ray o + t d on (v0, e1, e2), tri_test's operations: u belongs to the second input vertex, v to the
// third.  A ray in the triangle's plane (det 0) gives values that are not finite, which the interpolation below turns into flat.
__host__ __device__ inline void tri_uv(const float v0[3], const float e1[3], const float e2[3], const float o[3], const float d[3], float& u,
                                       float& v) {
    float pv[3], qv[3];
    cross3(d, e2, pv);
    const float idet = 1.0f / dot3h(e1, pv);
    const float tv[3] = {o[0] - v0[0], o[1] - v0[1], o[2] - v0[2]};
    u = dot3h(tv, pv) * idet;
    cross3(tv, e1, qv);
    v = dot3h(d, qv) * idet;
}
// ns = normalize((1 - u - v) n0 + u n1 + v n2) for the corner normals cn = (n0, n1, n2); ns = ng where the sum is not finite or has
// zero length, or where ns . ng <= 0
__host__ __device__ inline void smooth_normal(const float cn[9], float u, float v, const float ng[3], float ns[3]) {
    const float w = (1.0f - u) - v;
    for (int c = 0; c < 3; ++c) ns[c] = w * cn[c] + u * cn[3 + c] + v * cn[6 + c];
    const float l2 = dot3h(ns, ns);
    bool ok = l2 > 0.0f && l2 <= FLT_MAX;
    if (ok) {
        const float il = 1.0f / sqrtf(l2);
        for (int c = 0; c < 3; ++c) ns[c] *= il;
        ok = dot3h(ns, ng) > 0.0f;
    }
    if (!ok)
        for (int c = 0; c < 3; ++c) ns[c] = ng[c];
}
// the third fallback: ns = ng where the two normals disagree about the side the viewer is on
__host__ __device__ inline void smooth_side(const float ng[3], const float wo[3], float ns[3]) {
    if (!(dot3h(ns, wo) * dot3h(ng, wo) > 0.0f))
        for (int c = 0; c < 3; ++c) ns[c] = ng[c];
}
// object_sample at a vertex with the face normal ng and the shading normal ns (the third fallback applied here too: it is
// idempotent).  dielectric: the event about ns must agree with the geometry, a reflected wi on wo's side of ng and a transmitted
// one on the other; if it does not, the event is redone about ng with the same dim 6, so that "transmitted" always means "crossed
// the surface".  diffuse: sampled about ns; seen from behind ng, or sampled below ng, the path ends (weight 0).
__host__ __device__ inline void object_sample_shading(int kind, const float p[3], const float ng[3], const float ns_in[3], const float wo[3],
                                                      float u_lobe, float u0, float u1, float wi[3], float w[3], float& pdf, int& flags) {
    float n[3] = {ns_in[0], ns_in[1], ns_in[2]};
    smooth_side(ng, wo, n);
    const float go = dot3h(ng, wo);
    for (int pass = 0;; ++pass) {
        object_sample(kind, p, n, wo, u_lobe, u0, u1, wi, w, pdf, flags);
        if (kind != MATPBR_PATH_BSDF_DIELECTRIC || pass == 1) break;
        const float side = dot3h(ng, wi) * go;
        if ((flags & kFlagTransmitted) ? side < 0.0f : side > 0.0f) break;
        for (int c = 0; c < 3; ++c) n[c] = ng[c];
    }
    if (kind != MATPBR_PATH_BSDF_DIELECTRIC && !(go > 0.0f && dot3h(ng, wi) > 0.0f)) w[0] = w[1] = w[2] = 0.0f;
}

// ---- transparency editing ("Transparency editing"): TransBSDF (myutils/mi_plugin.py:1477-1771) -----------
// Where mask[tp] is set the depth mesh shades as a sheet of glass in front of the photograph `bg`, read at the texel a ray refracted
// twice through the sheet lands on.  The edit travels to the kernel by value, in the place of the object table.  The masked-branch
// arithmetic and the lookup are __host__ __device__ (plain divisions and sqrtf): the CPU entry points run what the kernel runs.
struct TransEdit {
    const uint8_t* mask;   // [H,W], non-zero = edited
    const float* bg;       // [H,W,3]
    float ior, spec_trans, refract_distance;
};
__device__ __forceinline__ int object_of(const TransEdit&, int, float[3]) { return 0; }

// the texel a point projects to ("Material at a hit": floor, clamped to the image; a NaN coordinate clamps to 0)
__host__ __device__ inline long screen_texel(const float p[3], float f_ndc, float aspect, int H, int W) {
    const float ndc0 = f_ndc * (-p[0]) / p[2], ndc1 = (f_ndc * aspect) * p[1] / p[2];
    const float sx = (ndc0 + 1.0f) * 0.5f * (float)W, sy = (ndc1 + 1.0f) * 0.5f * (float)H;
    const int tx = (int)fminf(fmaxf(floorf(sx), 0.0f), (float)(W - 1)), ty = (int)fminf(fmaxf(floorf(sy), 0.0f), (float)(H - 1));
    return (long)ty * W + tx;
}
// calculate_refraction (:1494-1501): w refracted about n with the ratio eta, normalised
__host__ __device__ inline void trans_refract(const float w[3], const float n[3], float eta, float out[3]) {
    const float c = dot3h(w, n);
    const float s2 = fmaxf(0.0f, 1.0f - c * c);
    const float ct = sqrtf(fmaxf(0.0f, 1.0f - eta * eta * s2));
    for (int k = 0; k < 3; ++k) out[k] = eta * (n[k] * c - w[k]) - n[k] * ct;
    const float il = 1.0f / sqrtf(dot3h(out, out));
    for (int k = 0; k < 3; ++k) out[k] *= il;
}
// calculate_refracted_screen_coor (:1503-1519): into the sheet for 0.3 D, out of it for D, and the texel of that point
__host__ __device__ inline long trans_lookup(float ior, float dist, const float p[3], const float n[3], const float wo[3], float f_ndc,
                                             float aspect, int H, int W) {
    float d1[3], d2[3], p2[3];
    trans_refract(wo, n, ior, d1);
    const float md1[3] = {-d1[0], -d1[1], -d1[2]};
    trans_refract(md1, n, 1.0f / ior, d2);
    for (int k = 0; k < 3; ++k) p2[k] = (p[k] + (0.3f * dist) * d1[k]) + dist * d2[k];
    return screen_texel(p2, f_ndc, aspect, H, W);
}
// eval_brdf's masked branch (:1650-1724): f (RGB, with its cosine) and the pdf.  The GGX denominator takes 1 - NoH^2 from n x h
// where n is a unit vector (ggx_den_stable's form: the literal one loses its digits on the peak).
__host__ __device__ inline void trans_eval(float ior, float T, const float n[3], const float wo[3], const float wi[3], const float a[3], float r,
                                           float m, const float bg[3], float f[3], float& pdf) {
    const float kInvPiF = 0.31830988618379067154f;
    float h[3] = {wi[0] + wo[0], wi[1] + wo[1], wi[2] + wo[2]};
    const float il = 1.0f / sqrtf(dot3h(h, h));
    for (int k = 0; k < 3; ++k) h[k] *= il;
    const float nh_raw = dot3h(n, h);
    const float NoL = fmaxf(dot3h(n, wi), 0.0f), NoV = fmaxf(dot3h(n, wo), 0.0f), VoH = fmaxf(dot3h(wo, h), 0.0f), NoH = fmaxf(nh_raw, 0.0f);
    const float LoH = fmaxf(dot3h(wi, h), 0.0f);
    const float alpha2 = (r * r) * (r * r);
    float den;
    if (fabsf(dot3h(n, n) - 1.0f) < 1e-5f && nh_raw > 0.0f) {
        float cr[3];
        cross3(n, h, cr);
        den = (alpha2 + dot3h(cr, cr) * (1.0f - alpha2)) + 1e-6f;
    } else {
        den = (NoH * NoH * (alpha2 - 1.0f) + 1.0f) + 1e-6f;
    }
    const float D = alpha2 * kInvPiF / (den * den);
    pdf = 0.5f * (D / (4.0f * fmaxf(VoH, 1e-4f)) * NoH) + 0.5f * (NoL * kInvPiF);
    if (!(pdf > 0.0f)) pdf = 0.0f;
    const float k = (r + 1.0f) * (r + 1.0f) * 0.125f;
    const float G = (1.0f / (NoL * (1.0f - k) + k + 1e-6f)) * (1.0f / (NoV * (1.0f - k) + k + 1e-6f));
    const float x = 1.0f - VoH, x5 = (x * x) * (x * x) * x;
    float glass;   // f_glass without its colour
    const bool reflect = NoL * NoV > 0.0f;
    if (reflect) {
        glass = D * G * 0.25f * (NoL + 1e-6f);
    } else {   // btdf_glass (:1702-1712), literally: of order 1e-6, not zero
        const float hw_in = 1.0f / (LoH + 1e-6f), hw_out = 1.0f / (VoH + 1e-6f);
        const float nw_in = 1.0f / (NoL + 1e-6f), nw_out = 1.0f / (NoV + 1e-6f);
        const float R_s = (hw_in - ior * hw_out) / (hw_in + ior * hw_out), R_p = (ior * hw_in - hw_out) / (ior * hw_in + hw_out);
        const float F_glass = 0.5f * (R_s * R_s + R_p * R_p);
        const float e = 1.0f + 1e-6f, D_hack = kInvPiF / (e * e);   // D_GGX(NoH, 1)
        const float q = ior * hw_in + hw_out;
        glass = G * D_hack * (1.0f - F_glass) * (ior * ior * hw_in * hw_out) / (nw_in * nw_out * (q * q));
    }
    for (int c = 0; c < 3; ++c) {
        const float kd = a[c] * (1.0f - m) * (1.0f - T);
        const float C0 = (1.0f - m) * 0.04f + m * a[c];
        const float F_m = C0 + (1.0f - C0) * x5;
        const float bcg = (1.0f - m) * (bg[c] * T);
        const float v = kd * kInvPiF * NoL + D * G * F_m * 0.25f * NoL + (reflect ? bcg : sqrtf(bcg)) * glass;
        f[c] = v > 0.0f ? v : 0.0f;
    }
}
// the pdf of the unmasked branch while the edit is on: MatDiffBSDF's mixture with TransBSDF's clamp of VoH, 1e-4 (:1658)
__device__ __forceinline__ float trans_pdf(const PLane& ln, const BrdfState<float>& st) {
    return fmaf(0.125f * (st.D * ln.NoH), rcp(fmaxf(ln.VoH, 1e-4f)), (0.5f * kInvPi) * st.NoL);
}

// ---- shading normals ("Shading normals") -------------------------------------------------------------------
// The map travels to the kernel in the table's place.  A vertex then has two normals: ng, the face normal, keeps everything geometric
// (the back-face test, the spawn offset, which side a direction leaves on); ns = nrm[tp] takes the place of MatDiffBSDF's `normal`.
struct ShadeNormals {
    const float* nrm;   // [H,W,3], unit length, used as given
};
__device__ __forceinline__ int object_of(const ShadeNormals&, int, float[3]) { return 0; }

// d f / d n for one BSDF value at a vertex, added to dn: gl wi + gv wo + gh h with each cosine's gradient passed where the raw cosine
// is positive (eval_brdf_bwd_kernel's gates; dr.maximum passes the gradient where its argument is > 0)
__host__ __device__ inline void normal_grad(float gl, float gv, float gh, float NoL_raw, float NoV_raw, float nh_raw, const float wi[3],
                                            const float wo[3], const float h[3], float dn[3]) {
    gl = NoL_raw > 0.0f ? gl : 0.0f;
    gv = NoV_raw > 0.0f ? gv : 0.0f;
    gh = nh_raw > 0.0f ? gh : 0.0f;
    for (int c = 0; c < 3; ++c) dn[c] += fmaf(gl, wi[c], fmaf(gv, wo[c], gh * h[c]));
}

// The cosine gradients gl, gv, gh of brdf_core_grad<float, true> at (n, wo, wi) for the host entry point.  matpbr_device.hpp's
// functions are device code (hardware reciprocals), so the CPU restates path_lane, brdf_core and the WANT_N branch with plain
// divisions; the gates and the composition it feeds, normal_grad above, are the code the kernel runs.  cosines = n.wi, n.wo, n.h raw.
inline void cosine_grads_host(const float n[3], const float wo[3], const float wi[3], const float a[3], float r, float m, const float g[3],
                              float& gl, float& gv, float& gh, float cosines[3], float h[3]) {
    const float kInvPiF = 0.31830988618379067154f;
    for (int c = 0; c < 3; ++c) h[c] = wi[c] + wo[c];
    const float il = 1.0f / sqrtf(dot3h(h, h));
    for (int c = 0; c < 3; ++c) h[c] *= il;
    const float nh_raw = dot3h(n, h);
    cosines[0] = dot3h(n, wi); cosines[1] = dot3h(n, wo); cosines[2] = nh_raw;
    const float NoL = fmaxf(cosines[0], 0.0f), NoV = fmaxf(cosines[1], 0.0f), NoH = fmaxf(nh_raw, 0.0f), VoH = fmaxf(dot3h(wo, h), 0.0f);
    const float alpha2 = (r * r) * (r * r), am1 = alpha2 - 1.0f;
    float den;
    if (fabsf(dot3h(n, n) - 1.0f) < 1e-5f && nh_raw > 0.0f) {
        float cr[3];
        cross3(n, h, cr);
        den = (alpha2 - dot3h(cr, cr) * am1) + 1e-6f;
    } else {
        den = (NoH * NoH * am1 + 1.0f) + 1e-6f;
    }
    const float iden = 1.0f / den, D = alpha2 * kInvPiF * (iden * iden);
    const float k = (r + 1.0f) * (r + 1.0f) * 0.125f, omk = 1.0f - k, kpe = k + 1e-6f;
    const float g1l = 1.0f / (NoL * omk + kpe), g1v = 1.0f / (NoV * omk + kpe), G = g1l * g1v;
    const float FDm1 = 2.0f * r * VoH * VoH - 0.5f;
    const float ol = 1.0f - NoL, ov = 1.0f - NoV, ol4 = (ol * ol) * (ol * ol), ov4 = (ov * ov) * (ov * ov);
    const float Fi = FDm1 * (ol4 * ol) + 1.0f, Fo = FDm1 * (ov4 * ov) + 1.0f;
    const float xh = 1.0f - VoH, x5 = (xh * xh) * (xh * xh) * xh;
    float gd = 0.0f, gs = 0.0f;
    for (int c = 0; c < 3; ++c) {
        const float C0 = m * a[c] + (1.0f - m) * 0.04f;
        gd += g[c] * ((a[c] * (1.0f - m)) * kInvPiF);
        gs += g[c] * (x5 * (1.0f - C0) + C0);
    }
    const float dFi = -5.0f * FDm1 * ol4, dFo = -5.0f * ov4 * FDm1;
    const float dG_dNoL = -omk * g1l * G, dG_dNoV = -g1v * omk * G;
    const float gsq = gs * 0.25f * NoL;
    gl = gd * Fo * (dFi * NoL + Fi) + gs * 0.25f * D * (dG_dNoL * NoL + G);
    gv = gd * dFo * (Fi * NoL) + gsq * D * dG_dNoV;
    gh = gsq * G * (-4.0f * am1 * D * NoH * iden);
}

struct PathArgs {
    const float4* nodes;
    const float4* tris;
    const float *a, *r, *m;
    const float *env, *row_cdf, *col_cdf, *env_pdf;
    float* out;
    uint32_t* rays;        // nullable: rays traced per pixel, added to (a count for reporting rates)
    int H, W, He, We, spp, max_depth;
    float f_pix, cx, cy;   // camera rays: ((x - cx)/f_pix, -(y - cy)/f_pix, -1)
    float f_ndc, aspect;   // texel lookup: 1/tan(fov_x/2), W/H (ndc0 = f_ndc x/(-z), ndc1 = f_ndc aspect y/z)
    uint32_t seed_hash;    // pcg(seed)
};

// spawn offset along the (camera-side) face normal, relative to the point's magnitude
__device__ __forceinline__ float spawn_eps(const float p[3]) { return 1e-5f * (1.0f + fmaxf(fmaxf(fabsf(p[0]), fabsf(p[1])), fabsf(p[2]))); }

// samples [s0, s1) of every pixel added to out (first: start from 0; last: divide by spp).  OBJ: the BVH holds inserted objects
// (Objects = ObjTable, passed by value); EDIT: transparency editing (Objects = TransEdit, by value in the table's place).  With
// NoObjects every `if (OBJ ...)`, `if (EDIT ...)` and `if (NRM ...)` below folds away and the walk is the depth mesh's alone, the code
// the kernel had before there were objects; with ObjTable every `if (EDIT ...)` folds away.  NRM: shading normals (Objects =
// ShadeNormals): `n` stays the face normal ng and `ns` is the map's.  SMOOTH: smooth inserted objects (Objects = SmoothObjects): OBJ
// with `ns` the interpolated corner normal at the vertices of a flagged object; every `if (SMOOTH ...)` folds away in the other four.
// PBR: SMOOTH with objects of kind 3 (Objects = PbrObjects), whose vertices run the depth mesh's branch about `ns` on the constants of
// their record; every `if (PBR ...)` folds away in the other five.
template <class Objects>
__global__ __launch_bounds__(kBlock) void path_kernel(const PathArgs q, int s0, int s1, int first, int last, const Objects ot) {
    constexpr bool PBR = std::is_same<Objects, PbrObjects>::value;
    constexpr bool SMOOTH = std::is_same<Objects, SmoothObjects>::value || PBR;
    constexpr bool OBJ = std::is_same<Objects, ObjTable>::value || SMOOTH;
    constexpr bool EDIT = std::is_same<Objects, TransEdit>::value;
    constexpr bool NRM = std::is_same<Objects, ShadeNormals>::value;
    __shared__ int s_stack[kStack * kBlock];
    const int tid = threadIdx.y * kTileX + threadIdx.x;
    const int j = blockIdx.x * kTileX + threadIdx.x, i = blockIdx.y * kTileY + threadIdx.y;
    if (i >= q.H || j >= q.W) return;   // no barriers below: each lane's stack column is its own
    LdsStack stk{s_stack + tid};
    const long pix = (long)i * q.W + j;
    const bool have_tab = q.row_cdf[q.He] > 0.0f;   // an envmap of zero luminance has no emitter sampling
    float acc[3] = {0.0f, 0.0f, 0.0f};
    if (!first) {
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = q.out[3 * pix + c];
    }
    const uint32_t pix_hash = pcg_hash(q.seed_hash + (uint32_t)pix);
    uint32_t n_rays = 0;
    for (int s = s0; s < s1; ++s) {
        const uint32_t base = pcg_hash(pix_hash + (uint32_t)s);
        float L[3] = {0.0f, 0.0f, 0.0f}, thr[3] = {1.0f, 1.0f, 1.0f};
        // camera ray through a uniformly jittered position of the pixel (box filter)
        const float x = (float)j - 0.5f + rng_u(base, 0, 0), y = (float)i - 0.5f + rng_u(base, 0, 1);
        float o[3] = {0.0f, 0.0f, 0.0f}, d[3] = {(x - q.cx) / q.f_pix, -(y - q.cy) / q.f_pix, -1.0f};
        {
            const float il = rsq(dot3(d, d));
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] *= il;
        }
        float prev_pdf = 0.0f;
        bool prev_delta = false;   // (OBJ) the ray left a delta vertex: no emitter sample competed with it
        for (int depth = 0;; ++depth) {
            float t = FLT_MAX;
            ++n_rays;
            const int k = trace<false>(q.nodes, q.tris, o, d, 0.0f, t, stk);
            if (k < 0) {   // escaped: the envmap, MIS-weighted against emitter sampling after a BSDF sample
                const int tx = env_texel(d, q.He, q.We);
                const float w = depth == 0 || (OBJ && prev_delta) ? 1.0f : mis_weight(prev_pdf, have_tab ? q.env_pdf[tx] : 0.0f);
#pragma unroll
                for (int c = 0; c < 3; ++c) L[c] += thr[c] * (q.env[3 * tx + c] * w);
                break;
            }
            if (depth + 1 >= q.max_depth) break;   // Mitsuba's active_next: the surfaces emit nothing
            const float4 B = q.tris[3 * k + 1], C = q.tris[3 * k + 2];
            const float e1[3] = {B.x, B.y, B.z}, e2[3] = {C.x, C.y, C.z};
            float n[3];
            cross3(e1, e2, n);   // the face normal, oriented to the camera side by the builder
            {
                const float il = rsq(dot3(n, n));
#pragma unroll
                for (int c = 0; c < 3; ++c) n[c] *= il;
            }
            const float wo[3] = {-d[0], -d[1], -d[2]};
            int kind = 0;          // (OBJ) 0: the depth mesh; else the inserted object's BSDF and its parameters
            float op[3] = {0.0f, 0.0f, 0.0f};
            float oa[3] = {0.0f, 0.0f, 0.0f}, o_r = 0.0f, o_m = 0.0f;   // (PBR) the record of an object of kind 3
            if constexpr (PBR) kind = object_lookup(ot.t, ot.pbr, __float_as_int(q.tris[3 * k].w), op, oa, o_r, o_m);
            else if (OBJ) kind = object_of(ot, __float_as_int(q.tris[3 * k].w), op);
            bool smooth = false;   // (SMOOTH) the object shades with its interpolated corner normals, `ns` below
            if constexpr (SMOOTH) {
                smooth = (kind & MATPBR_PATH_OBJECT_SMOOTH) != 0;
                kind &= ~MATPBR_PATH_OBJECT_SMOOTH;
            }
            // a hit on the back of a triangle ends the path (glass shades from both sides)
            if (!(OBJ && kind == MATPBR_PATH_BSDF_DIELECTRIC) && !(dot3(n, wo) > 0.0f)) break;
            float p[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) p[c] = fmaf(t, d[c], o[c]);
            // material: the texel the hit point projects to by the inverse of the camera above (one focal length for both axes; a6
            // world_to_screen when H = W), floor, clamped to the image (MatDiffBSDF)
            const float ndc0 = q.f_ndc * (-p[0]) / p[2], ndc1 = (q.f_ndc * q.aspect) * p[1] / p[2];
            const float sx = (ndc0 + 1.0f) * 0.5f * (float)q.W, sy = (ndc1 + 1.0f) * 0.5f * (float)q.H;
            const int tx = (int)fminf(fmaxf(floorf(sx), 0.0f), (float)(q.W - 1)), ty = (int)fminf(fmaxf(floorf(sy), 0.0f), (float)(q.H - 1));
            const long tp = OBJ && kind != 0 ? 0 : (long)ty * q.W + tx;   // an object reads no texel
            float av[3] = {q.a[3 * tp], q.a[3 * tp + 1], q.a[3 * tp + 2]}, rv = q.r[tp], mv = q.m[tp];
            const bool pbr = PBR && kind == MATPBR_PATH_BSDF_PBR;   // (PBR) the depth mesh's branch on the object's constants
            if constexpr (PBR) {
                if (pbr) { av[0] = oa[0]; av[1] = oa[1]; av[2] = oa[2]; rv = o_r; mv = o_m; }
            }
            float ns[3] = {n[0], n[1], n[2]};   // (NRM) the shading normal: every cosine, both samplers' frames, the pdf
            if constexpr (NRM) {
#pragma unroll
                for (int c = 0; c < 3; ++c) ns[c] = ot.nrm[3 * tp + c];
            }
            if constexpr (SMOOTH) {
                if (smooth) {   // u, v of the winning triangle once more; its nine corner normals, consumed at once
                    const float4 A = q.tris[3 * k];
                    const float v0[3] = {A.x, A.y, A.z};
                    const float* cp = ot.nrm + 9 * (long)(__float_as_int(A.w) - ot.n_scene_tri);
                    float cn[9], bu, bv;
#pragma unroll
                    for (int c = 0; c < 9; ++c) cn[c] = cp[c];
                    tri_uv(v0, e1, e2, o, d, bu, bv);
                    smooth_normal(cn, bu, bv, n, ns);
                    smooth_side(n, wo, ns);
                }
            }
            bool masked = false;   // (EDIT) the vertex reads a masked texel: TransBSDF's glass over bg at the refracted texel
            float bgv[3] = {0.0f, 0.0f, 0.0f};
            if constexpr (EDIT) {
                masked = ot.mask[tp] != 0;
                if (masked) {
                    const long tq = trans_lookup(ot.ior, ot.refract_distance, p, n, wo, q.f_ndc, q.aspect, q.H, q.W);
#pragma unroll
                    for (int c = 0; c < 3; ++c) bgv[c] = ot.bg[3 * tq + c];
                }
            }
            const float eps = spawn_eps(p);
            float po[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) po[c] = fmaf(eps, n[c], p[c]);
            // emitter sample with a shadow ray (none at a delta vertex)
            if (have_tab && !(OBJ && kind == MATPBR_PATH_BSDF_DIELECTRIC)) {
                float wl[3], pdf_e;
                const int te = env_sample(q.row_cdf, q.col_cdf, q.env_pdf, q.He, q.We, rng_u(base, depth, 2), rng_u(base, depth, 3),
                                          rng_u(base, depth, 4), rng_u(base, depth, 5), wl, pdf_e);
                if (pdf_e > 0.0f && dot3(n, wl) > 0.0f) {
                    float f[3], pdf_b;
                    if (OBJ && kind == MATPBR_PATH_BSDF_DIFFUSE) {   // f cos = rho / pi max(n . wi, 0), pdf = cos / pi
                        if constexpr (SMOOTH) pdf_b = fmaxf(dot3(ns, wl), 0.0f) * kInvPi;   // ns = n on a flat object
                        else pdf_b = dot3(n, wl) * kInvPi;
#pragma unroll
                        for (int c = 0; c < 3; ++c) f[c] = op[c] * pdf_b;
                    } else if (EDIT && masked) {
                        if constexpr (EDIT) trans_eval(ot.ior, ot.spec_trans, n, wo, wl, av, rv, mv, bgv, f, pdf_b);
                    } else if (EDIT) {   // MatDiffBSDF's value, TransBSDF's pdf
                        PLane ln;
                        BrdfState<float> st;
                        path_eval_st(wl, wo, n, av, rv, mv, ln, st, f, pdf_b);
                        pdf_b = trans_pdf(ln, st);
                    } else {
                        path_eval(wl, wo, NRM || PBR ? ns : n, av, rv, mv, f, pdf_b);   // (PBR) ns = n on the depth mesh
                    }
                    if (f[0] > 0.0f || f[1] > 0.0f || f[2] > 0.0f) {
                        float ts = FLT_MAX;
                        ++n_rays;
                        if (trace<true>(q.nodes, q.tris, po, wl, 0.0f, ts, stk) < 0) {
                            const float w = mis_weight(pdf_e, pdf_b) / pdf_e;
#pragma unroll
                            for (int c = 0; c < 3; ++c) L[c] += thr[c] * (f[c] * (q.env[3 * te + c] * w));
                        }
                    }
                }
            }
            // BSDF sample: the next ray
            float wi[3], wgt[3], pdf_s;
            if (OBJ && kind != 0 && !pbr) {
                int flags;
                if (SMOOTH && smooth)
                    object_sample_shading(kind, op, n, ns, wo, rng_u(base, depth, 6), rng_u(base, depth, 7), rng_u(base, depth, 8), wi, wgt, pdf_s, flags);
                else
                    object_sample(kind, op, n, wo, rng_u(base, depth, 6), rng_u(base, depth, 7), rng_u(base, depth, 8), wi, wgt, pdf_s, flags);
                prev_delta = (flags & kFlagDelta) != 0;
                const float side = dot3(n, wi) > 0.0f ? eps : -eps;   // spawn on the side the new ray leaves on
#pragma unroll
                for (int c = 0; c < 3; ++c) po[c] = fmaf(side, n[c], p[c]);
            } else if (EDIT) {   // MatDiffBSDF's directions; weight f / (pdf + 1e-4) where pdf > 0, masked or not (:1612-1615)
                PLane ln;
                BrdfState<float> st;
                float f[3], pt;
                path_sample_st(rng_u(base, depth, 6), rng_u(base, depth, 7), rng_u(base, depth, 8), wo, n, av, rv, mv, wi, ln, st, f, pt);
                pt = trans_pdf(ln, st);
                if constexpr (EDIT) {
                    if (masked) trans_eval(ot.ior, ot.spec_trans, n, wo, wi, av, rv, mv, bgv, f, pt);
                }
                const float ip = pt > 0.0f ? 1.0f / (pt + 1e-4f) : 0.0f;
#pragma unroll
                for (int c = 0; c < 3; ++c) wgt[c] = f[c] > 0.0f ? f[c] * ip : 0.0f;
                pdf_s = pt > 0.0f ? pt : 0.0f;
            } else {
                path_sample(rng_u(base, depth, 6), rng_u(base, depth, 7), rng_u(base, depth, 8), wo, NRM || PBR ? ns : n, av, rv, mv, wi, wgt, pdf_s);
                if (OBJ) prev_delta = false;
                if (NRM && !(dot3(n, wi) > 0.0f)) break;   // sampled below the sheet: nothing is carried through it
                if (PBR && pbr && !(dot3(n, wi) > 0.0f)) break;   // a reflection that leaves below the object's face carries nothing
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) thr[c] *= wgt[c];
            if (!(thr[0] > 0.0f || thr[1] > 0.0f || thr[2] > 0.0f)) break;
            prev_pdf = pdf_s;
#pragma unroll
            for (int c = 0; c < 3; ++c) { o[c] = po[c]; d[c] = wi[c]; }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += L[c];
    }
    const float sc = last ? 1.0f / (float)q.spp : 1.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) q.out[3 * pix + c] = last ? acc[c] * sc : acc[c];
    if (q.rays) q.rays[pix] += n_rays;
}
// ---- backward pass ("Gradients") ------------------------------------------------------------------------
// The exact derivative of the fixed-seed estimator with the sampling detached: directions, pdfs, MIS weights, lobe choices and the
// envmap tables are constants; the gradient flows through the BSDF value f (trailing cosine included) at every vertex and through
// the envmap texels Le.  Path replay (Vicini et al. 2021, "Path Replay Backpropagation"): pass 1 replays a sample to get its
// radiance L; pass 2 replays it again carrying the radiance still to come, `rem`.  At a vertex, the emitter term E = thr f_e Le w
// gives d/d theta through f_e with upstream g thr Le w; after E is taken off, `rem` is exactly the part of L that carries the
// vertex's BSDF-sample factor f_s / (pdf_s + 1e-6), so its upstream through f_s is g rem / f_s.
//
// Determinism: every gradient is summed as 64-bit fixed point, integer addition being associative.  The quantum is a power of two
// derived on the device from max|d_out| (path_bwd_scale_kernel): q = 2^(e - 24) with max|d_out| < 2^e.  A contribution is rounded
// to the nearest multiple of q (error <= q/2 <= 2^-24 max|d_out|) and clamped to +-2^46 q (over 2^22 max|d_out|); the sum of an
// element's n contributions is then off by at most n q / 2 before the final division by spp, and 2^17 clamped contributions still
// fit in 63 bits.  Maps: the vertex a lane shades on its own texel (the camera vertex, nearly always) goes to the lane's registers,
// one integer atomic per launch; the other vertices scatter with integer atomics.  Envmap: per workgroup in LDS (integer LDS
// atomics), one row per workgroup in the workspace, and the rows are added in a small second launch.
constexpr int kBwdMaxEnvTexels = MATPBR_PATH_BWD_MAX_ENV_TEXELS;   // the workgroup's LDS row: 3 x 8 bytes per texel
constexpr float kFixClamp = 70368744177664.0f;   // 2^46 quanta
constexpr double kRemFloor = 1.7763568394002505e-15;  // 2^-49: below kRemFloor * max_depth * L the radiance still to come is rounding

struct BwdArgs {
    const float* d_out;
    unsigned long long* acc;       // [H*W, 5] fixed point: a (3), r, m
    unsigned long long* env_rows;  // [n_wg, He*We*3] fixed point
    const float* scale;            // [0] = 1/q, [1] = q (path_bwd_scale_kernel)
    int want_a, want_r, want_m, want_env;
};

__device__ __forceinline__ long long to_fix(float v, float inv_q) {
    return __float2ll_rn(fminf(fmaxf(v * inv_q, -kFixClamp), kFixClamp));
}

// the backward pass's shading normals: a trailing kernel argument that the plain instantiation does not have (an empty pack, so its
// kernel arguments are what they were).  Without it the accumulators are a (3), r, m per pixel and every `if (NRM ...)` folds away;
// with it three more follow, the normal's.
struct BwdNormals {
    const float* nrm;   // [H,W,3]
    int want_n;
};
__device__ __forceinline__ bool want_n_of() { return false; }
__device__ __forceinline__ bool want_n_of(const BwdNormals& nm) { return nm.want_n != 0; }
__device__ __forceinline__ const float* nrm_of() { return nullptr; }
__device__ __forceinline__ const float* nrm_of(const BwdNormals& nm) { return nm.nrm; }
template <class... Normals> constexpr int kAccOf = sizeof...(Normals) ? 8 : 5;

// one vertex's material gradient to its texel: the lane's own texel in registers, any other with integer atomics
template <int ACC>
__device__ __forceinline__ void put_material(const BwdArgs& b, const BrdfGrad<float>& gv, long tp, long pix, float inv_q, long long* own) {
    const float v[5] = {gv.d_a[0], gv.d_a[1], gv.d_a[2], gv.d_r, gv.d_m};
    const int want[5] = {b.want_a, b.want_a, b.want_a, b.want_r, b.want_m};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        if (!want[k]) continue;
        const long long x = to_fix(v[k], inv_q);
        if (x == 0) continue;
        if (tp == pix) own[k] += x;
        else atomicAdd(b.acc + ACC * tp + k, (unsigned long long)x);
    }
}
// one vertex's normal gradient, to accumulators 5..7 of its texel
__device__ __forceinline__ void put_normal(const BwdArgs& b, const float dn[3], long tp, long pix, float inv_q, long long* own) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const long long x = to_fix(dn[c], inv_q);
        if (x == 0) continue;
        if (tp == pix) own[5 + c] += x;
        else atomicAdd(b.acc + 8 * tp + 5 + c, (unsigned long long)x);
    }
}
__device__ __forceinline__ void put_env(unsigned long long* s_env, int tx, const float v[3], float inv_q) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const long long x = to_fix(v[c], inv_q);
        if (x != 0) atomicAdd(s_env + 3 * tx + c, (unsigned long long)x);
    }
}

// One sample of pixel (i, j): GRAD = false adds its radiance to L (the forward kernel's walk, statement for statement, each fp32 term
// added in fp64); GRAD = true replays it with rem = that radiance, takes the same fp32 terms off in fp64, and sends the gradients of
// g . L to the sinks.  In fp32, rem = L - (terms so far) would be off by ~2^-24 L per term: at a black metal under a sun, where the
// radiance still to come is a small part of L and is divided by a tiny f_s, that cancellation alone made d_a several % wrong.
template <bool GRAD, class... Normals>
__device__ __forceinline__ void replay(const PathArgs& q, const BwdArgs& b, const Normals&... nm, uint32_t base, int i, int j, long pix, bool have_tab,
                                       LdsStack& stk, double L[3], const float g[3], float inv_q, long long* own, unsigned long long* s_env,
                                       uint32_t& n_rays) {
    constexpr bool NRM = sizeof...(Normals) != 0;   // `n` stays the face normal ng, `ns` is the map's
    constexpr int ACC = kAccOf<Normals...>;
    float thr[3] = {1.0f, 1.0f, 1.0f};
    double rem[3] = {L[0], L[1], L[2]};
    const float x = (float)j - 0.5f + rng_u(base, 0, 0), y = (float)i - 0.5f + rng_u(base, 0, 1);
    float o[3] = {0.0f, 0.0f, 0.0f}, d[3] = {(x - q.cx) / q.f_pix, -(y - q.cy) / q.f_pix, -1.0f};
    {
        const float il = rsq(dot3(d, d));
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] *= il;
    }
    const bool want_mat = b.want_a || b.want_r || b.want_m;
    const bool want_n = want_n_of(nm...), want_brdf = NRM ? want_mat || want_n : want_mat;
    float prev_pdf = 0.0f;
    for (int depth = 0;; ++depth) {
        float t = FLT_MAX;
        ++n_rays;
        const int k = trace<false>(q.nodes, q.tris, o, d, 0.0f, t, stk);
        if (k < 0) {
            const int tx = env_texel(d, q.He, q.We);
            const float w = depth == 0 ? 1.0f : mis_weight(prev_pdf, have_tab ? q.env_pdf[tx] : 0.0f);
            if (GRAD) {
                if (b.want_env) {
                    const float v[3] = {g[0] * (thr[0] * w), g[1] * (thr[1] * w), g[2] * (thr[2] * w)};
                    put_env(s_env, tx, v, inv_q);
                }
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) L[c] += (double)(thr[c] * (q.env[3 * tx + c] * w));
            }
            break;
        }
        if (depth + 1 >= q.max_depth) break;
        const float4 B = q.tris[3 * k + 1], C = q.tris[3 * k + 2];
        const float e1[3] = {B.x, B.y, B.z}, e2[3] = {C.x, C.y, C.z};
        float n[3];
        cross3(e1, e2, n);
        {
            const float il = rsq(dot3(n, n));
#pragma unroll
            for (int c = 0; c < 3; ++c) n[c] *= il;
        }
        const float wo[3] = {-d[0], -d[1], -d[2]};
        if (!(dot3(n, wo) > 0.0f)) break;
        float p[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) p[c] = fmaf(t, d[c], o[c]);
        const float ndc0 = q.f_ndc * (-p[0]) / p[2], ndc1 = (q.f_ndc * q.aspect) * p[1] / p[2];
        const float sx = (ndc0 + 1.0f) * 0.5f * (float)q.W, sy = (ndc1 + 1.0f) * 0.5f * (float)q.H;
        const int tx = (int)fminf(fmaxf(floorf(sx), 0.0f), (float)(q.W - 1)), ty = (int)fminf(fmaxf(floorf(sy), 0.0f), (float)(q.H - 1));
        const long tp = (long)ty * q.W + tx;
        const float av[3] = {q.a[3 * tp], q.a[3 * tp + 1], q.a[3 * tp + 2]}, rv = q.r[tp], mv = q.m[tp];
        float ns[3] = {n[0], n[1], n[2]};
        if constexpr (NRM) {
#pragma unroll
            for (int c = 0; c < 3; ++c) ns[c] = nrm_of(nm...)[3 * tp + c];
        }
        const float eps = spawn_eps(p);
        float po[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) po[c] = fmaf(eps, n[c], p[c]);
        BrdfGrad<float> gv;
        brdf_grad_zero(gv);
        float gl, gh;   // cosine gradients: read with NRM only
        float dn[3] = {0.0f, 0.0f, 0.0f};
        if (have_tab) {
            float wl[3], pdf_e;
            const int te = env_sample(q.row_cdf, q.col_cdf, q.env_pdf, q.He, q.We, rng_u(base, depth, 2), rng_u(base, depth, 3),
                                      rng_u(base, depth, 4), rng_u(base, depth, 5), wl, pdf_e);
            if (pdf_e > 0.0f && dot3(n, wl) > 0.0f) {
                float f[3], pdf_b;
                PLane ln;
                BrdfState<float> st;
                path_eval_st(wl, wo, NRM ? ns : n, av, rv, mv, ln, st, f, pdf_b);
                if (f[0] > 0.0f || f[1] > 0.0f || f[2] > 0.0f) {
                    float ts = FLT_MAX;
                    ++n_rays;
                    if (trace<true>(q.nodes, q.tris, po, wl, 0.0f, ts, stk) < 0) {
                        const float w = mis_weight(pdf_e, pdf_b) / pdf_e;
                        if (GRAD) {
                            float ge[3], ve[3];
#pragma unroll
                            for (int c = 0; c < 3; ++c) {
                                const float Le = q.env[3 * te + c];
                                rem[c] -= (double)(thr[c] * (f[c] * (Le * w)));
                                ge[c] = g[c] * (thr[c] * (Le * w));
                                ve[c] = g[c] * (thr[c] * (f[c] * w));
                            }
                            if constexpr (NRM) {
                                if (want_brdf) {   // gv.dNoV gathers both BSDF values' d/d(n . wo): composed once, below
                                    brdf_core_grad<float, true>(ln.pc, st, ge, gv, gl, gh);
                                    float h[3];
                                    const float nh_raw = half_vector(wl, wo, ns, h);
                                    normal_grad(gl, 0.0f, gh, ln.NoL_raw, 0.0f, nh_raw, wl, wo, h, dn);
                                }
                            } else {
                                if (want_mat) brdf_core_grad<float, false>(ln.pc, st, ge, gv, gl, gh);
                            }
                            if (b.want_env) put_env(s_env, te, ve, inv_q);
                        } else {
#pragma unroll
                            for (int c = 0; c < 3; ++c) L[c] += (double)(thr[c] * (f[c] * (q.env[3 * te + c] * w)));
                        }
                    }
                }
            }
        }
        float wi[3], fs[3], ps;
        PLane ln;
        BrdfState<float> st;
        path_sample_st(rng_u(base, depth, 6), rng_u(base, depth, 7), rng_u(base, depth, 8), wo, NRM ? ns : n, av, rv, mv, wi, ln, st, fs, ps);
        // (NRM) sampled below the sheet: the path ends here (thr = 0), after the emitter term's gradient has gone out
        const float ip = ps > 1e-6f && !(NRM && !(dot3(n, wi) > 0.0f)) ? 1.0f / (ps + 1e-6f) : 0.0f;
        if (GRAD && want_brdf) {
            if (ip > 0.0f) {   // d (f_s / (pdf_s + 1e-6)) / d theta carried by everything after this vertex: rem / f_s per channel
                // rem is L minus at most 2 max_depth fp32 terms in fp64, off by <= 2 max_depth 2^-53 L: a rem below kRemFloor
                // max_depth L is that rounding (the path gathers nothing more), and dividing it by a small f_s (a black metal) would
                // make it a gradient
                float gs[3];
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    gs[c] = fs[c] > 0.0f && rem[c] > kRemFloor * (double)q.max_depth * L[c] ? g[c] * ((float)rem[c] / fs[c]) : 0.0f;
                if constexpr (NRM) {
                    brdf_core_grad<float, true>(ln.pc, st, gs, gv, gl, gh);
                    float h[3];
                    const float nh_raw = half_vector(wi, wo, ns, h);
                    normal_grad(gl, 0.0f, gh, ln.NoL_raw, 0.0f, nh_raw, wi, wo, h, dn);
                } else {
                    brdf_core_grad<float, false>(ln.pc, st, gs, gv, gl, gh);
                }
            }
            if (!NRM || want_mat) put_material<ACC>(b, gv, tp, pix, inv_q, own);
            if constexpr (NRM) {
                if (want_n) {
                    normal_grad(0.0f, gv.dNoV, 0.0f, 0.0f, ln.pc.NoV_raw, 0.0f, wi, wo, wo, dn);
                    put_normal(b, dn, tp, pix, inv_q, own);
                }
            }
        }
        (void)gl; (void)gh;
#pragma unroll
        for (int c = 0; c < 3; ++c) thr[c] *= fs[c] * ip;
        if (!(thr[0] > 0.0f || thr[1] > 0.0f || thr[2] > 0.0f)) break;
        prev_pdf = ps > 0.0f ? ps : 0.0f;
#pragma unroll
        for (int c = 0; c < 3; ++c) { o[c] = po[c]; d[c] = wi[c]; }
    }
}

// samples [s0, s1) of every pixel: both passes per sample; the lane's own-texel sums and the workgroup's envmap row go out at the end
template <class... Normals>
__global__ __launch_bounds__(kBlock) void path_bwd_kernel(const PathArgs q, const BwdArgs b, int s0, int s1, const Normals... nm) {
    constexpr int ACC = kAccOf<Normals...>;
    __shared__ int s_stack[kStack * kBlock];
    extern __shared__ unsigned long long s_env[];   // [He*We*3] when d_env is asked for
    const int tid = threadIdx.y * kTileX + threadIdx.x;
    const int n_env = b.want_env ? 3 * q.He * q.We : 0;
    for (int k = tid; k < n_env; k += kBlock) s_env[k] = 0ull;
    __syncthreads();
    const int j = blockIdx.x * kTileX + threadIdx.x, i = blockIdx.y * kTileY + threadIdx.y;
    if (i < q.H && j < q.W) {
        LdsStack stk{s_stack + tid};
        const long pix = (long)i * q.W + j;
        const bool have_tab = q.row_cdf[q.He] > 0.0f;
        const float inv_q = b.scale[0];
        const float g[3] = {b.d_out[3 * pix], b.d_out[3 * pix + 1], b.d_out[3 * pix + 2]};
        long long own[ACC] = {};
        const uint32_t pix_hash = pcg_hash(q.seed_hash + (uint32_t)pix);
        uint32_t n_rays = 0;
        for (int s = s0; s < s1; ++s) {
            const uint32_t base = pcg_hash(pix_hash + (uint32_t)s);
            double L[3] = {0.0, 0.0, 0.0};
            replay<false, Normals...>(q, b, nm..., base, i, j, pix, have_tab, stk, L, g, inv_q, own, s_env, n_rays);
            replay<true, Normals...>(q, b, nm..., base, i, j, pix, have_tab, stk, L, g, inv_q, own, s_env, n_rays);
        }
#pragma unroll
        for (int k = 0; k < ACC; ++k)
            if (own[k] != 0) atomicAdd(b.acc + ACC * pix + k, (unsigned long long)own[k]);
        if (q.rays) q.rays[pix] += n_rays;
    }
    __syncthreads();
    unsigned long long* row = b.env_rows + (long)(blockIdx.y * gridDim.x + blockIdx.x) * n_env;
    for (int k = tid; k < n_env; k += kBlock) row[k] += s_env[k];   // each workgroup owns its row; launches follow each other on the stream
}

// the quantum: q = 2^(e - 24) with max|d_out| < 2^e (1 when d_out is all zero)
__global__ __launch_bounds__(1024) void path_bwd_scale_kernel(const float* __restrict__ d_out, long n, float* scale) {
    __shared__ float s_max[1024];
    float mx = 0.0f;
    for (long k = threadIdx.x; k < n; k += 1024) mx = fmaxf(mx, fabsf(d_out[k]));
    s_max[threadIdx.x] = mx;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s_max[threadIdx.x] = fmaxf(s_max[threadIdx.x], s_max[threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float m = s_max[0];
        int e = 24;
        if (m > 0.0f && isfinite(m)) frexpf(m, &e);
        scale[0] = ldexpf(1.0f, 24 - e);
        scale[1] = ldexpf(1.0f, e - 24);
    }
}

// fixed point -> fp32, ADDED to the caller's maps: d_x += sum * q / spp
template <int ACC>
__global__ __launch_bounds__(256) void path_bwd_maps_kernel(const unsigned long long* __restrict__ acc, const float* __restrict__ scale, long P,
                                                            int spp, float* d_a, float* d_r, float* d_m) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const double s = (double)scale[1] / (double)spp;
    const unsigned long long* e = acc + ACC * p;
    if (d_a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) d_a[3 * p + c] += (float)((double)(long long)e[c] * s);
    }
    if (d_r) d_r[p] += (float)((double)(long long)e[3] * s);
    if (d_m) d_m[p] += (float)((double)(long long)e[4] * s);
}
// accumulators 5..7 of a pixel -> d_n += sum * q / spp
__global__ __launch_bounds__(256) void path_bwd_normal_kernel(const unsigned long long* __restrict__ acc, const float* __restrict__ scale, long P,
                                                              int spp, float* d_n) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const double s = (double)scale[1] / (double)spp;
#pragma unroll
    for (int c = 0; c < 3; ++c) d_n[3 * p + c] += (float)((double)(long long)acc[8 * p + 5 + c] * s);
}
// the workgroups' envmap rows, added in row order, -> d_env += sum * q / spp
__global__ __launch_bounds__(256) void path_bwd_env_kernel(const unsigned long long* __restrict__ rows, const float* __restrict__ scale, int n_env,
                                                           int n_rows, int spp, float* d_env) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_env) return;
    unsigned long long sum = 0ull;
    for (int w = 0; w < n_rows; ++w) sum += rows[(long)w * n_env + k];
    d_env[k] += (float)((double)(long long)sum * ((double)scale[1] / (double)spp));
}

// ---- host: binned-SAH builder --------------------------------------------------------------------------------------------
struct Box {
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    void grow(const Box& b) {
        for (int c = 0; c < 3; ++c) { lo[c] = std::min(lo[c], b.lo[c]); hi[c] = std::max(hi[c], b.hi[c]); }
    }
    double area() const {
        if (lo[0] > hi[0]) return 0.0;
        const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
        return dx * dy + dy * dz + dz * dx;
    }
};

struct Builder {
    std::vector<Box> tb;            // per-triangle box (padded)
    std::vector<float> cen;         // per-triangle centroid [3N]
    std::vector<int32_t> idx;       // permutation: leaf order
    BNode* nodes;
    long max_nodes, n_nodes = 0, n_leaves = 0;
    int depth = 0;

    Box range_box(int b, int e) const {
        Box r;
        for (int k = b; k < e; ++k) r.grow(tb[idx[k]]);
        return r;
    }
    // split [b, e) in two non-empty halves: the binned-SAH plane, or the middle when every centroid coincides
    int split(int b, int e) {
        float clo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, chi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
        for (int k = b; k < e; ++k)
            for (int c = 0; c < 3; ++c) { clo[c] = std::min(clo[c], cen[3 * idx[k] + c]); chi[c] = std::max(chi[c], cen[3 * idx[k] + c]); }
        double best = DBL_MAX;
        int best_axis = -1, best_plane = 0;
        for (int ax = 0; ax < 3; ++ax) {
            const float ext = chi[ax] - clo[ax];
            if (!(ext > 0.0f)) continue;
            const float scale = (float)kBins / ext;
            Box bb[kBins];
            int bn[kBins] = {0};
            for (int k = b; k < e; ++k) {
                const int t = idx[k];
                const int bi = std::min(kBins - 1, (int)((cen[3 * t + ax] - clo[ax]) * scale));
                bb[bi].grow(tb[t]);
                ++bn[bi];
            }
            double right_cost[kBins];
            Box acc;
            int cnt = 0;
            for (int p = kBins - 1; p > 0; --p) {   // plane p: bins [0,p) left, [p,kBins) right
                acc.grow(bb[p]);
                cnt += bn[p];
                right_cost[p] = cnt ? acc.area() * cnt : 0.0;
            }
            Box lacc;
            int lcnt = 0;
            for (int p = 1; p < kBins; ++p) {
                lacc.grow(bb[p - 1]);
                lcnt += bn[p - 1];
                if (lcnt == 0 || lcnt == e - b) continue;
                const double cost = lacc.area() * lcnt + right_cost[p];
                if (cost < best) { best = cost; best_axis = ax; best_plane = p; }
            }
        }
        if (best_axis < 0) return b + (e - b) / 2;
        const float lo = clo[best_axis], scale = (float)kBins / (chi[best_axis] - clo[best_axis]);
        int32_t* mid = std::partition(idx.data() + b, idx.data() + e, [&](int32_t t) {
            return std::min(kBins - 1, (int)((cen[3 * t + best_axis] - lo) * scale)) < best_plane;
        });
        return (int)(mid - idx.data());
    }
    struct Item { long node; int slot, b, e, level; };
    bool build(int N) {
        if (max_nodes < 1) return false;
        n_nodes = 1;
        std::memset(&nodes[0], 0, sizeof(BNode));
        std::vector<Item> work;
        if (N <= kLeafMax) {
            work.push_back({0, 0, 0, N, 1});
            work.push_back({0, 1, N, N, 1});
        } else {
            const int m = split(0, N);
            work.push_back({0, 1, m, N, 1});
            work.push_back({0, 0, 0, m, 1});
        }
        while (!work.empty()) {
            const Item it = work.back();
            work.pop_back();
            depth = std::max(depth, it.level);
            BNode& nd = nodes[it.node];
            const Box bx = range_box(it.b, it.e);
            if (it.e == it.b) {   // empty slot (root of a mesh of <= kLeafMax triangles): a point box, a leaf without triangles
                for (int c = 0; c < 6; ++c) nd.b[6 * it.slot + c] = 0.0f;
            } else {
                for (int c = 0; c < 3; ++c) { nd.b[6 * it.slot + c] = bx.lo[c]; nd.b[6 * it.slot + 3 + c] = bx.hi[c]; }
            }
            if (it.e - it.b <= kLeafMax || it.level >= kMaxBvhDepth) {
                nd.child[it.slot] = it.b;
                nd.count[it.slot] = it.e - it.b;
                ++n_leaves;
                continue;
            }
            if (n_nodes >= max_nodes) return false;
            const long q = n_nodes++;
            nd.child[it.slot] = (int32_t)q;
            nd.count[it.slot] = -1;
            std::memset(&nodes[q], 0, sizeof(BNode));
            const int m = split(it.b, it.e);
            work.push_back({q, 1, m, it.e, it.level + 1});
            work.push_back({q, 0, it.b, m, it.level + 1});
        }
        return true;
    }
};

// the caller's objects, checked, as the kernel's table
bool object_valid(const MatpbrPathObject& ob) {
    if (ob.first_tri < 0 || ob.n_tri < 0 || ob.n_tri > INT32_MAX - ob.first_tri) return false;
    if (ob.kind == MATPBR_PATH_BSDF_DIELECTRIC) return ob.p[0] > 0.0f && ob.p[1] > 0.0f && std::isfinite(ob.p[0]) && std::isfinite(ob.p[1]);
    if (ob.kind == MATPBR_PATH_BSDF_DIFFUSE) {
        for (int c = 0; c < 3; ++c)
            if (!(ob.p[c] >= 0.0f && ob.p[c] <= 1.0f)) return false;
        return true;
    }
    return false;
}
// the record of an object of kind MATPBR_PATH_BSDF_PBR: a in [0, 1], r in [0.07, 1], m in [0, 1] (a NaN fails every comparison)
bool pbr_valid(const MatpbrPathObjectPbr& pr) {
    for (int c = 0; c < 3; ++c)
        if (!(pr.a[c] >= 0.0f && pr.a[c] <= 1.0f)) return false;
    return pr.r >= 0.07f && pr.r <= 1.0f && pr.m >= 0.0f && pr.m <= 1.0f;
}
// `n_smooth` (nullable): where given, a kind may carry MATPBR_PATH_OBJECT_SMOOTH, and the flagged objects are counted.  `n_pbr`
// (nullable): where given, a kind may be MATPBR_PATH_BSDF_PBR (its p[] is ignored), and those objects are counted; their records
// are checked where `pbr` is given.
bool object_table(const MatpbrPathObject* objects, int n_objects, ObjTable& ot, int* n_smooth = nullptr, int* n_pbr = nullptr,
                  const MatpbrPathObjectPbr* pbr = nullptr) {
    if (n_objects < 0 || n_objects > MATPBR_PATH_MAX_OBJECTS || (n_objects > 0 && !objects)) return false;
    ot.n = n_objects;
    ot.min_id = INT32_MAX;
    if (n_smooth) *n_smooth = 0;
    if (n_pbr) *n_pbr = 0;
    for (int k = 0; k < n_objects; ++k) {
        MatpbrPathObject plain = objects[k];
        if (n_smooth && (plain.kind & MATPBR_PATH_OBJECT_SMOOTH)) {
            plain.kind &= ~MATPBR_PATH_OBJECT_SMOOTH;
            ++*n_smooth;
        }
        if (n_pbr && plain.kind == MATPBR_PATH_BSDF_PBR) {   // checked as a diffuse object of reflectance 0: the range alone
            if (pbr && !pbr_valid(pbr[k])) return false;
            plain.kind = MATPBR_PATH_BSDF_DIFFUSE;
            plain.p[0] = plain.p[1] = plain.p[2] = 0.0f;
            ++*n_pbr;
        }
        if (!object_valid(plain)) return false;
        for (int j = 0; j < k; ++j)   // ranges may not overlap
            if (objects[k].first_tri < objects[j].first_tri + objects[j].n_tri && objects[j].first_tri < objects[k].first_tri + objects[k].n_tri)
                return false;
        ot.o[k] = objects[k];
        ot.min_id = std::min(ot.min_id, objects[k].first_tri);
    }
    return true;
}

}  // namespace

// =================================================================================================================================
// C ABI
// =================================================================================================================================
extern "C" {

int matpbr_path_version(void) { return MATPBR_PATH_VERSION; }

const char* matpbr_path_strerror(int code) {
    switch (code) {
        case MATPBR_PATH_OK: return "ok";
        case MATPBR_PATH_ERR_INVALID_ARG: return "invalid argument (null pointer, non-positive size, index out of range, max_depth outside 1..16, "
                                                  "a workspace too small, an envmap of more than 1024 texels with d_env, a bad object table, a smooth object without corner normals or a bad transparency edit)";
        case MATPBR_PATH_ERR_LAUNCH: return "HIP kernel launch failed";
        case MATPBR_PATH_ERR_CAPACITY: return "node buffer smaller than matpbr_path_bvh_size() asks for";
        default: return "unknown error";
    }
}

int matpbr_path_bvh_size(long n_tri, long* max_nodes) {
    if (n_tri < 0 || n_tri > INT32_MAX / 3 || !max_nodes) return MATPBR_PATH_ERR_INVALID_ARG;
    *max_nodes = std::max(1L, n_tri);   // inner nodes of a binary tree with non-empty leaves: <= n_tri - 1 (+ the root)
    return MATPBR_PATH_OK;
}

int matpbr_path_bvh_build(const double* vert, long n_vert, const int32_t* tri, long n_tri, void* nodes, long max_nodes, void* tris,
                          long* n_nodes, int* depth, long* n_leaves) {
    return matpbr_path_bvh_build_objects(vert, n_vert, tri, n_tri, n_tri, nodes, max_nodes, tris, n_nodes, depth, n_leaves);
}

int matpbr_path_bvh_build_objects(const double* vert, long n_vert, const int32_t* tri, long n_tri, long n_scene_tri, void* nodes,
                                  long max_nodes, void* tris, long* n_nodes, int* depth, long* n_leaves) {
    if (!vert || !tri || !nodes || !tris || !n_nodes || !depth || !n_leaves || n_vert <= 0 || n_tri < 0 || n_tri > INT32_MAX / 3 ||
        n_scene_tri < 0 || n_scene_tri > n_tri)
        return MATPBR_PATH_ERR_INVALID_ARG;
    long need = 0;
    matpbr_path_bvh_size(n_tri, &need);
    if (max_nodes < need) return MATPBR_PATH_ERR_CAPACITY;
    for (long k = 0; k < 3 * n_tri; ++k)
        if (tri[k] < 0 || tri[k] >= n_vert) return MATPBR_PATH_ERR_INVALID_ARG;
    const int N = (int)n_tri;
    double S = 0.0;   // scene scale: boxes are padded by 1e-6 of it so that fp32 rounding of (v0, e1, e2) stays inside
    for (long k = 0; k < 3 * n_vert; ++k) S = std::max(S, std::fabs(vert[k]));
    const float pad = (float)(1e-6 * S);
    Builder bld;
    bld.nodes = static_cast<BNode*>(nodes);
    bld.max_nodes = max_nodes;
    bld.tb.resize(N);
    bld.cen.resize(3 * (size_t)N);
    bld.idx.resize(N);
    for (int t = 0; t < N; ++t) {
        Box b;
        for (int c = 0; c < 3; ++c) {
            double lo = DBL_MAX, hi = -DBL_MAX;
            for (int v = 0; v < 3; ++v) { lo = std::min(lo, vert[3 * (long)tri[3 * t + v] + c]); hi = std::max(hi, vert[3 * (long)tri[3 * t + v] + c]); }
            b.lo[c] = (float)lo - pad;
            b.hi[c] = (float)hi + pad;
            bld.cen[3 * t + c] = (float)(0.5 * (lo + hi));
        }
        bld.tb[t] = b;
        bld.idx[t] = t;
    }
    if (!bld.build(N)) return MATPBR_PATH_ERR_CAPACITY;
    float4* T = static_cast<float4*>(tris);
    for (int k = 0; k < N; ++k) {
        const int t = bld.idx[k];
        const double* v0 = vert + 3 * (long)tri[3 * t];
        const double* v1 = vert + 3 * (long)tri[3 * t + 1];
        const double* v2 = vert + 3 * (long)tri[3 * t + 2];
        double e1[3], e2[3];
        for (int c = 0; c < 3; ++c) { e1[c] = v1[c] - v0[c]; e2[c] = v2[c] - v0[c]; }
        const double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
        // depth mesh: e1 x e2 faces the camera at the origin; an inserted mesh keeps its winding (e1 x e2 = its outward normal)
        if (t < n_scene_tri && nx * v0[0] + ny * v0[1] + nz * v0[2] > 0.0) std::swap(e1, e2);
        int32_t id = t;
        float idf;
        std::memcpy(&idf, &id, 4);
        T[3 * k] = make_float4((float)v0[0], (float)v0[1], (float)v0[2], idf);
        T[3 * k + 1] = make_float4((float)e1[0], (float)e1[1], (float)e1[2], 0.0f);
        T[3 * k + 2] = make_float4((float)e2[0], (float)e2[1], (float)e2[2], 0.0f);
    }
    *n_nodes = bld.n_nodes;
    *depth = bld.depth;
    *n_leaves = bld.n_leaves;
    return MATPBR_PATH_OK;
}

int matpbr_path_trace_host(const void* nodes, const void* tris, const float* o, const float* d, long N, float tmin, float tmax,
                           float* t_hit, int32_t* tri_hit) {
    if (!nodes || !tris || !o || !d || !t_hit || !tri_hit || N < 0) return MATPBR_PATH_ERR_INVALID_ARG;
    const float4* T = static_cast<const float4*>(tris);
    for (long k = 0; k < N; ++k) {
        HostStack stk;
        float t = tmax;
        const int h = trace<false>(static_cast<const float4*>(nodes), T, o + 3 * k, d + 3 * k, tmin, t, stk);
        t_hit[k] = t;
        int32_t id = -1;
        if (h >= 0) std::memcpy(&id, &T[3 * h].w, 4);
        tri_hit[k] = id;
    }
    return MATPBR_PATH_OK;
}

int matpbr_path_env_tables(const float* env, int He, int We, float* row_cdf, float* col_cdf, float* pdf, double* total) {
    if (!env || !row_cdf || !col_cdf || !pdf || !total || He <= 0 || We <= 0) return MATPBR_PATH_ERR_INVALID_ARG;
    const double pi = 3.14159265358979323846;
    std::vector<double> w((size_t)He * We), row_w(He, 0.0);
    double tot = 0.0;
    for (int r = 0; r < He; ++r) {
        const double omega = (std::cos(r * pi / He) - std::cos((r + 1) * pi / He)) * (2.0 * pi / We);   // sh.envmap_solid_angles
        for (int c = 0; c < We; ++c) {
            const float* e = env + 3 * ((size_t)r * We + c);
            const double lum = std::max(0.0, 0.2126 * e[0] + 0.7152 * e[1] + 0.0722 * e[2]);
            w[(size_t)r * We + c] = lum;
            row_w[r] += lum * omega;
        }
        tot += row_w[r];
    }
    *total = tot;
    if (!(tot > 0.0) || !std::isfinite(tot)) {
        std::fill(row_cdf, row_cdf + He + 1, 0.0f);
        std::fill(col_cdf, col_cdf + (size_t)He * (We + 1), 0.0f);
        std::fill(pdf, pdf + (size_t)He * We, 0.0f);
        return MATPBR_PATH_OK;
    }
    double run = 0.0;
    row_cdf[0] = 0.0f;
    for (int r = 0; r < He; ++r) {
        run += row_w[r];
        row_cdf[r + 1] = (float)(run / tot);
        float* cc = col_cdf + (size_t)r * (We + 1);
        double rs = 0.0, rsum = 0.0;
        for (int c = 0; c < We; ++c) rsum += w[(size_t)r * We + c];
        cc[0] = 0.0f;
        for (int c = 0; c < We; ++c) {
            rs += w[(size_t)r * We + c];
            cc[c + 1] = rsum > 0.0 ? (float)(rs / rsum) : (float)(c + 1) / (float)We;
            pdf[(size_t)r * We + c] = (float)(w[(size_t)r * We + c] / tot);
        }
        cc[We] = 1.0f;
    }
    row_cdf[He] = 1.0f;
    return MATPBR_PATH_OK;
}

int matpbr_path_env_sample_host(const float* row_cdf, const float* col_cdf, const float* pdf, int He, int We, const float* u, long N,
                                float* dir, float* pdf_out, int32_t* texel) {
    if (!row_cdf || !col_cdf || !pdf || !u || !dir || !pdf_out || !texel || He <= 0 || We <= 0 || N < 0) return MATPBR_PATH_ERR_INVALID_ARG;
    const bool have = row_cdf[He] > 0.0f;
    for (long k = 0; k < N; ++k) {
        if (!have) {
            dir[3 * k] = dir[3 * k + 1] = dir[3 * k + 2] = 0.0f;
            pdf_out[k] = 0.0f;
            texel[k] = -1;
            continue;
        }
        texel[k] = env_sample(row_cdf, col_cdf, pdf, He, We, u[4 * k], u[4 * k + 1], u[4 * k + 2], u[4 * k + 3], dir + 3 * k, pdf_out[k]);
    }
    return MATPBR_PATH_OK;
}

int matpbr_path_object_sample_host(const MatpbrPathObject* object, const float* n, const float* wo, const float* u, long N, float* wi,
                                   float* weight, float* pdf, int32_t* flags) {
    if (!object || !n || !wo || !u || !wi || !weight || !pdf || !flags || N < 0 || !object_valid(*object)) return MATPBR_PATH_ERR_INVALID_ARG;
    for (long k = 0; k < N; ++k) {
        int fl = 0;
        object_sample(object->kind, object->p, n, wo + 3 * k, u[3 * k], u[3 * k + 1], u[3 * k + 2], wi + 3 * k, weight + 3 * k, pdf[k], fl);
        flags[k] = fl;
    }
    return MATPBR_PATH_OK;
}

int matpbr_path_render(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W, float fov_x_deg,
                       const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He, int We, int spp,
                       int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream) {
    return matpbr_path_render_objects(nodes, tris, a, r, m, H, W, fov_x_deg, env, row_cdf, col_cdf, env_pdf, He, We, spp, max_depth, seed,
                                      spp_per_launch, out, rays, stream, nullptr, 0);
}

// the six renders: `edit` (nullable) selects the transparency-editing instantiation, else `nrm` the shading-normal one, else
// `pbr` the PBR-object one (obj_nrm may be null then: no object is smooth), else `obj_nrm` the smooth-object one, else n_objects > 0
// the object one
static int render_common(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W, float fov_x_deg,
                         const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He, int We, int spp,
                         int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream, const ObjTable& ot,
                         int n_objects, const TransEdit* edit, const float* nrm = nullptr, const float* obj_nrm = nullptr,
                         int32_t n_scene_tri = 0, const MatpbrPathObjectPbr* pbr = nullptr) {
    if (!nodes || !tris || !a || !r || !m || !env || !row_cdf || !col_cdf || !env_pdf || !out || H <= 0 || W <= 0 || He <= 0 || We <= 0 ||
        spp <= 0 || spp_per_launch <= 0 || max_depth < 1 || max_depth > MATPBR_PATH_MAX_MAX_DEPTH || !(fov_x_deg > 0.0f && fov_x_deg < 180.0f))
        return MATPBR_PATH_ERR_INVALID_ARG;
    PathArgs q{};
    q.nodes = static_cast<const float4*>(nodes);
    q.tris = static_cast<const float4*>(tris);
    q.a = a; q.r = r; q.m = m;
    q.env = env; q.row_cdf = row_cdf; q.col_cdf = col_cdf; q.env_pdf = env_pdf;
    q.out = out;
    q.rays = rays;
    q.H = H; q.W = W; q.He = He; q.We = We; q.spp = spp; q.max_depth = max_depth;
    const double th = std::tan(0.5 * (double)fov_x_deg * 3.14159265358979323846 / 180.0);
    q.f_pix = (float)((0.5 * W) / th);                       // f = (W/2)/tan(fov/2), c = (W-1)/2, (H-1)/2
    q.cx = 0.5f * (float)(W - 1);
    q.cy = 0.5f * (float)(H - 1);
    q.f_ndc = (float)(1.0 / th);                             // perspective_projection_matrix (mi_plugin.py:585-595)
    q.aspect = (float)W / (float)H;
    q.seed_hash = pcg_hash(seed);
    const dim3 grid((unsigned)((W + kTileX - 1) / kTileX), (unsigned)((H + kTileY - 1) / kTileY));
    PbrObjects pbo{};
    if (pbr) {
        pbo.t = ot;
        pbo.nrm = obj_nrm;
        pbo.n_scene_tri = n_scene_tri;
        for (int k = 0; k < n_objects; ++k) pbo.pbr[k] = pbr[k];
    }
    for (int s0 = 0; s0 < spp; s0 += spp_per_launch) {
        const int s1 = std::min(spp, s0 + spp_per_launch);
        const int first = s0 == 0 ? 1 : 0, last = s1 == spp ? 1 : 0;
        if (edit) hipLaunchKernelGGL(path_kernel<TransEdit>, grid, dim3(kTileX, kTileY), 0, (hipStream_t)stream, q, s0, s1, first, last, *edit);
        else if (nrm) hipLaunchKernelGGL(path_kernel<ShadeNormals>, grid, dim3(kTileX, kTileY), 0, (hipStream_t)stream, q, s0, s1, first, last, ShadeNormals{nrm});
        else if (pbr) hipLaunchKernelGGL(path_kernel<PbrObjects>, grid, dim3(kTileX, kTileY), 0, (hipStream_t)stream, q, s0, s1, first, last, pbo);
        else if (obj_nrm) hipLaunchKernelGGL(path_kernel<SmoothObjects>, grid, dim3(kTileX, kTileY), 0, (hipStream_t)stream, q, s0, s1, first, last, SmoothObjects{ot, obj_nrm, n_scene_tri});
        else if (n_objects > 0) hipLaunchKernelGGL(path_kernel<ObjTable>, grid, dim3(kTileX, kTileY), 0, (hipStream_t)stream, q, s0, s1, first, last, ot);
        else hipLaunchKernelGGL(path_kernel<NoObjects>, grid, dim3(kTileX, kTileY), 0, (hipStream_t)stream, q, s0, s1, first, last, NoObjects{});
        if (hipGetLastError() != hipSuccess) return MATPBR_PATH_ERR_LAUNCH;
    }
    return MATPBR_PATH_OK;
}

static bool trans_edit_valid(const MatpbrPathTransEdit* e) {
    return e && e->ior > 0.0f && std::isfinite(e->ior) && e->spec_trans >= 0.0f && e->spec_trans <= 1.0f && e->refract_distance >= 0.0f &&
           std::isfinite(e->refract_distance);
}

int matpbr_path_render_objects(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                               float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                               int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream,
                               const MatpbrPathObject* objects, int n_objects) {
    ObjTable ot{};
    if (!object_table(objects, n_objects, ot)) return MATPBR_PATH_ERR_INVALID_ARG;
    return render_common(nodes, tris, a, r, m, H, W, fov_x_deg, env, row_cdf, col_cdf, env_pdf, He, We, spp, max_depth, seed, spp_per_launch, out,
                         rays, stream, ot, n_objects, nullptr);
}

int matpbr_path_render_objects_normals(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                       float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                       int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream,
                                       const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri) {
    ObjTable ot{};
    int n_smooth = 0;
    if (!object_table(objects, n_objects, ot, &n_smooth) || n_scene_tri < 0 || n_scene_tri > INT32_MAX || (n_smooth > 0 && !obj_nrm))
        return MATPBR_PATH_ERR_INVALID_ARG;
    for (int k = 0; k < n_objects; ++k)
        if (objects[k].first_tri < n_scene_tri) return MATPBR_PATH_ERR_INVALID_ARG;
    return render_common(nodes, tris, a, r, m, H, W, fov_x_deg, env, row_cdf, col_cdf, env_pdf, He, We, spp, max_depth, seed, spp_per_launch, out,
                         rays, stream, ot, n_objects, nullptr, nullptr, n_smooth > 0 ? obj_nrm : nullptr, (int32_t)n_scene_tri);
}

int matpbr_path_object_normal_host(const float* tri, const float* nrm, const float* o, const float* d, long N, float* u, float* v, float* ns) {
    if (!tri || !nrm || !o || !d || !u || !v || !ns || N < 0) return MATPBR_PATH_ERR_INVALID_ARG;
    for (long k = 0; k < N; ++k) {
        const float *v0 = tri + 9 * k, *e1 = v0 + 3, *e2 = v0 + 6;
        float ng[3];
        cross3(e1, e2, ng);
        const float il = 1.0f / sqrtf(dot3h(ng, ng));
        for (int c = 0; c < 3; ++c) ng[c] *= il;
        tri_uv(v0, e1, e2, o + 3 * k, d + 3 * k, u[k], v[k]);
        smooth_normal(nrm + 9 * k, u[k], v[k], ng, ns + 3 * k);
    }
    return MATPBR_PATH_OK;
}

int matpbr_path_object_sample_shading_host(const MatpbrPathObject* object, const float* ng, const float* ns, const float* wo, const float* u,
                                           long N, float* wi, float* weight, float* pdf, int32_t* flags) {
    if (!object || !ng || !ns || !wo || !u || !wi || !weight || !pdf || !flags || N < 0 || !object_valid(*object)) return MATPBR_PATH_ERR_INVALID_ARG;
    for (long k = 0; k < N; ++k) {
        int fl = 0;
        object_sample_shading(object->kind, object->p, ng + 3 * k, ns + 3 * k, wo + 3 * k, u[3 * k], u[3 * k + 1], u[3 * k + 2], wi + 3 * k,
                              weight + 3 * k, pdf[k], fl);
        flags[k] = fl;
    }
    return MATPBR_PATH_OK;
}

int matpbr_path_render_objects_pbr(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                   float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                   int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream,
                                   const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                   const MatpbrPathObjectPbr* pbr) {
    bool any_pbr = false;
    for (int k = 0; objects && k >= 0 && k < n_objects && k < MATPBR_PATH_MAX_OBJECTS; ++k)
        any_pbr = any_pbr || (objects[k].kind & ~MATPBR_PATH_OBJECT_SMOOTH) == MATPBR_PATH_BSDF_PBR;
    if (!any_pbr)
        return matpbr_path_render_objects_normals(nodes, tris, a, r, m, H, W, fov_x_deg, env, row_cdf, col_cdf, env_pdf, He, We, spp, max_depth, seed,
                                                  spp_per_launch, out, rays, stream, objects, n_objects, obj_nrm, n_scene_tri);
    ObjTable ot{};
    int n_smooth = 0, n_pbr = 0;
    if (!pbr || !object_table(objects, n_objects, ot, &n_smooth, &n_pbr, pbr) || n_scene_tri < 0 || n_scene_tri > INT32_MAX ||
        (n_smooth > 0 && !obj_nrm))
        return MATPBR_PATH_ERR_INVALID_ARG;
    for (int k = 0; k < n_objects; ++k)
        if (objects[k].first_tri < n_scene_tri) return MATPBR_PATH_ERR_INVALID_ARG;
    return render_common(nodes, tris, a, r, m, H, W, fov_x_deg, env, row_cdf, col_cdf, env_pdf, He, We, spp, max_depth, seed, spp_per_launch, out,
                         rays, stream, ot, n_objects, nullptr, nullptr, n_smooth > 0 ? obj_nrm : nullptr, (int32_t)n_scene_tri, pbr);
}

int matpbr_path_object_lookup_host(const MatpbrPathObject* objects, int n_objects, const MatpbrPathObjectPbr* pbr, const int32_t* ids, long N,
                                   int32_t* kind, float* a, float* r, float* m) {
    ObjTable ot{};
    int n_smooth = 0, n_pbr = 0;
    if (!ids || !kind || !a || !r || !m || N < 0 || !object_table(objects, n_objects, ot, &n_smooth, &n_pbr, pbr) || (n_pbr > 0 && !pbr))
        return MATPBR_PATH_ERR_INVALID_ARG;
    for (long k = 0; k < N; ++k) {
        float p[3] = {0.0f, 0.0f, 0.0f};
        a[3 * k] = a[3 * k + 1] = a[3 * k + 2] = 0.0f;
        r[k] = m[k] = 0.0f;
        kind[k] = object_lookup(ot, pbr, ids[k], p, a + 3 * k, r[k], m[k]);
    }
    return MATPBR_PATH_OK;
}

int matpbr_path_render_trans(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                             float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                             int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream,
                             const uint8_t* mask, const float* bg, const MatpbrPathTransEdit* edit) {
    if (!mask || !bg || !trans_edit_valid(edit)) return MATPBR_PATH_ERR_INVALID_ARG;
    const TransEdit te{mask, bg, edit->ior, edit->spec_trans, edit->refract_distance};
    return render_common(nodes, tris, a, r, m, H, W, fov_x_deg, env, row_cdf, col_cdf, env_pdf, He, We, spp, max_depth, seed, spp_per_launch, out,
                         rays, stream, ObjTable{}, 0, &te);
}

int matpbr_path_render_normals(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                               float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                               int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream,
                               const float* nrm) {
    return render_common(nodes, tris, a, r, m, H, W, fov_x_deg, env, row_cdf, col_cdf, env_pdf, He, We, spp, max_depth, seed, spp_per_launch, out,
                         rays, stream, ObjTable{}, 0, nullptr, nrm);
}

int matpbr_path_eval_normal_grad_host(const float* n, const float* wo, const float* wi, const float* a, const float* r, const float* m,
                                      const float* g, long N, float* d_n) {
    if (!n || !wo || !wi || !a || !r || !m || !g || !d_n || N < 0) return MATPBR_PATH_ERR_INVALID_ARG;
    for (long k = 0; k < N; ++k) {
        float gl, gv, gh, cosines[3], h[3];
        cosine_grads_host(n + 3 * k, wo + 3 * k, wi + 3 * k, a + 3 * k, r[k], m[k], g + 3 * k, gl, gv, gh, cosines, h);
        d_n[3 * k] = d_n[3 * k + 1] = d_n[3 * k + 2] = 0.0f;
        normal_grad(gl, gv, gh, cosines[0], cosines[1], cosines[2], wi + 3 * k, wo + 3 * k, h, d_n + 3 * k);
    }
    return MATPBR_PATH_OK;
}

int matpbr_path_trans_eval_host(const MatpbrPathTransEdit* edit, const float* n, const float* wo, const float* wi, const float* a,
                                const float* r, const float* m, const float* bg, long N, float* f, float* pdf) {
    if (!trans_edit_valid(edit) || !n || !wo || !wi || !a || !r || !m || !bg || !f || !pdf || N < 0) return MATPBR_PATH_ERR_INVALID_ARG;
    for (long k = 0; k < N; ++k)
        trans_eval(edit->ior, edit->spec_trans, n + 3 * k, wo + 3 * k, wi + 3 * k, a + 3 * k, r[k], m[k], bg + 3 * k, f + 3 * k, pdf[k]);
    return MATPBR_PATH_OK;
}

int matpbr_path_trans_lookup_host(const MatpbrPathTransEdit* edit, const float* p, const float* n, const float* wo, long N, int H, int W,
                                  float fov_x_deg, int32_t* texel, int32_t* texel_refracted) {
    if (!trans_edit_valid(edit) || !p || !n || !wo || !texel || !texel_refracted || N < 0 || H <= 0 || W <= 0 ||
        !(fov_x_deg > 0.0f && fov_x_deg < 180.0f))
        return MATPBR_PATH_ERR_INVALID_ARG;
    const double th = std::tan(0.5 * (double)fov_x_deg * 3.14159265358979323846 / 180.0);
    const float f_ndc = (float)(1.0 / th), aspect = (float)W / (float)H;   // as the render sets them
    for (long k = 0; k < N; ++k) {
        texel[k] = (int32_t)screen_texel(p + 3 * k, f_ndc, aspect, H, W);
        texel_refracted[k] = (int32_t)trans_lookup(edit->ior, edit->refract_distance, p + 3 * k, n + 3 * k, wo + 3 * k, f_ndc, aspect, H, W);
    }
    return MATPBR_PATH_OK;
}

static size_t bwd_workspace_bytes(int H, int W, int He, int We, int n_acc) {
    if (H <= 0 || W <= 0 || He <= 0 || We <= 0) return 0;
    const size_t n_wg = (size_t)((W + kTileX - 1) / kTileX) * (size_t)((H + kTileY - 1) / kTileY);
    return 256 + (size_t)H * W * n_acc * 8 + n_wg * (size_t)He * We * 3 * 8;
}
size_t matpbr_path_render_bwd_workspace_bytes(int H, int W, int He, int We) { return bwd_workspace_bytes(H, W, He, We, 5); }
size_t matpbr_path_render_bwd_normals_workspace_bytes(int H, int W, int He, int We) { return bwd_workspace_bytes(H, W, He, We, 8); }

int matpbr_path_render_bwd(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W, float fov_x_deg,
                           const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He, int We, int spp,
                           int max_depth, uint32_t seed, int spp_per_launch, const float* d_out, float* d_a, float* d_r, float* d_m,
                           float* d_env, void* workspace, size_t workspace_bytes, uint32_t* rays, void* stream) {
    return matpbr_path_render_bwd_normals(nodes, tris, a, r, m, H, W, fov_x_deg, env, row_cdf, col_cdf, env_pdf, He, We, spp, max_depth, seed,
                                          spp_per_launch, d_out, d_a, d_r, d_m, d_env, workspace, workspace_bytes, rays, stream, nullptr, nullptr);
}

// nrm == NULL: the plain backward kernel and its five accumulators per pixel; else the shading-normal one and eight
int matpbr_path_render_bwd_normals(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                   float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                   int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, const float* d_out, float* d_a, float* d_r,
                                   float* d_m, float* d_env, void* workspace, size_t workspace_bytes, uint32_t* rays, void* stream,
                                   const float* nrm, float* d_n) {
    const int n_acc = nrm ? 8 : 5;
    if ((!nrm && d_n) || !nodes || !tris || !a || !r || !m || !env || !row_cdf || !col_cdf || !env_pdf || !d_out || !workspace || H <= 0 || W <= 0 ||
        He <= 0 || We <= 0 || spp <= 0 || spp_per_launch <= 0 || max_depth < 1 || max_depth > MATPBR_PATH_MAX_MAX_DEPTH ||
        !(fov_x_deg > 0.0f && fov_x_deg < 180.0f) || (d_env && (long)He * We > kBwdMaxEnvTexels) ||
        workspace_bytes < bwd_workspace_bytes(H, W, He, We, n_acc) || ((uintptr_t)workspace & 7))
        return MATPBR_PATH_ERR_INVALID_ARG;
    if (!d_a && !d_r && !d_m && !d_env && !d_n) return MATPBR_PATH_OK;
    PathArgs q{};
    q.nodes = static_cast<const float4*>(nodes);
    q.tris = static_cast<const float4*>(tris);
    q.a = a; q.r = r; q.m = m;
    q.env = env; q.row_cdf = row_cdf; q.col_cdf = col_cdf; q.env_pdf = env_pdf;
    q.out = nullptr;
    q.rays = rays;
    q.H = H; q.W = W; q.He = He; q.We = We; q.spp = spp; q.max_depth = max_depth;
    const double th = std::tan(0.5 * (double)fov_x_deg * 3.14159265358979323846 / 180.0);
    q.f_pix = (float)((0.5 * W) / th);
    q.cx = 0.5f * (float)(W - 1);
    q.cy = 0.5f * (float)(H - 1);
    q.f_ndc = (float)(1.0 / th);
    q.aspect = (float)W / (float)H;
    q.seed_hash = pcg_hash(seed);
    const dim3 grid((unsigned)((W + kTileX - 1) / kTileX), (unsigned)((H + kTileY - 1) / kTileY));
    const int n_wg = (int)(grid.x * grid.y);
    const long P = (long)H * W;
    const int n_env = d_env ? 3 * He * We : 0;
    char* ws = static_cast<char*>(workspace);
    BwdArgs b{};
    b.d_out = d_out;
    b.scale = reinterpret_cast<float*>(ws);
    b.acc = reinterpret_cast<unsigned long long*>(ws + 256);
    b.env_rows = b.acc + n_acc * P;
    b.want_a = d_a != nullptr; b.want_r = d_r != nullptr; b.want_m = d_m != nullptr; b.want_env = d_env != nullptr;
    const hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(ws + 256, 0, (size_t)P * n_acc * 8 + (size_t)n_wg * n_env * 8, st) != hipSuccess) return MATPBR_PATH_ERR_LAUNCH;
    hipLaunchKernelGGL(path_bwd_scale_kernel, dim3(1), dim3(1024), 0, st, d_out, 3 * P, reinterpret_cast<float*>(ws));
    if (hipGetLastError() != hipSuccess) return MATPBR_PATH_ERR_LAUNCH;
    for (int s0 = 0; s0 < spp; s0 += spp_per_launch) {
        const int s1 = std::min(spp, s0 + spp_per_launch);
        if (nrm) hipLaunchKernelGGL(path_bwd_kernel<BwdNormals>, grid, dim3(kTileX, kTileY), (size_t)n_env * 8, st, q, b, s0, s1,
                                    BwdNormals{nrm, d_n != nullptr});
        else hipLaunchKernelGGL(path_bwd_kernel<>, grid, dim3(kTileX, kTileY), (size_t)n_env * 8, st, q, b, s0, s1);
        if (hipGetLastError() != hipSuccess) return MATPBR_PATH_ERR_LAUNCH;
    }
    if (d_a || d_r || d_m) {
        const dim3 mg((unsigned)((P + 255) / 256));
        if (nrm) hipLaunchKernelGGL(path_bwd_maps_kernel<8>, mg, dim3(256), 0, st, (const unsigned long long*)b.acc, b.scale, P, spp, d_a, d_r, d_m);
        else hipLaunchKernelGGL(path_bwd_maps_kernel<5>, mg, dim3(256), 0, st, (const unsigned long long*)b.acc, b.scale, P, spp, d_a, d_r, d_m);
        if (hipGetLastError() != hipSuccess) return MATPBR_PATH_ERR_LAUNCH;
    }
    if (d_n) {
        hipLaunchKernelGGL(path_bwd_normal_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, (const unsigned long long*)b.acc, b.scale, P,
                           spp, d_n);
        if (hipGetLastError() != hipSuccess) return MATPBR_PATH_ERR_LAUNCH;
    }
    if (d_env) {
        hipLaunchKernelGGL(path_bwd_env_kernel, dim3((unsigned)((n_env + 255) / 256)), dim3(256), 0, st, (const unsigned long long*)b.env_rows, b.scale,
                           n_env, n_wg, spp, d_env);
        if (hipGetLastError() != hipSuccess) return MATPBR_PATH_ERR_LAUNCH;
    }
    return MATPBR_PATH_OK;
}

}  // extern "C"

// =================================================================================================================================
// Denoiser ("Denoiser"): first-hit features and a variance-guided edge-avoiding a-trous filter
// =================================================================================================================================
// The spatial part of SVGF (Schied et al. 2017) over the a-trous wavelet of Dammertz et al. 2010, the variance from two half
// buffers (Rousselle et al. 2012), the guides noise-free features of the camera ray through the pixel centre.  Forward only, no
// atomics: the bits are the same from run to run.  The per-pixel bodies are __host__ __device__: the *_host entry points run what
// the kernels run (the device takes its exponentials and reciprocals from the hardware's approximations, the CPU from libm).
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

// index of the object whose range holds triangle `id`, -1: the depth mesh (object_of's lookup, returning the index the id feature
// needs; __host__ __device__ for the CPU entry point)
__host__ __device__ inline int object_index(const ObjTable& ot, int id) {
    int idx = -1;
    if (id < ot.min_id) return idx;
    for (int k = 0; k < MATPBR_PATH_MAX_OBJECTS; ++k) {
        const MatpbrPathObject& ob = ot.o[k];
        if (k < ot.n && id >= ob.first_tri && id - ob.first_tri < ob.n_tri) idx = k;
    }
    return idx;
}

// ---- the feature ray's traversal ---------------------------------------------------------------------------------------------------
// The depth mesh's vertices lie on the rays through the pixel centres ("Camera"), so a feature ray meets the
// mesh in a vertex, where rounding decides which of the triangles around it wins.  `trace` rounds differently on the device (fused
// multiply-adds) and on the CPU (none), and the two would name different triangles there.  The feature ray therefore walks the BVH
// with `trace`'s closest-hit statements restated under `fp contract(off)`: every product and sum is rounded on its own, divisions
// and square roots are correctly rounded on both sides, and the device takes the decisions the CPU takes, which are `trace`'s own
// on the CPU (matpbr_path_trace_host).  The render kernels keep `trace`.
__host__ __device__ inline float dot3s(const float a[3], const float b[3]) {
#pragma clang fp contract(off)
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}
__host__ __device__ inline void cross3s(const float a[3], const float b[3], float c[3]) {
#pragma clang fp contract(off)
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}
__host__ __device__ inline bool box_hit_s(float lx, float ly, float lz, float hx, float hy, float hz, const float inv[3], const float oi[3],
                                          float tmin, float tmax, float& tn) {
#pragma clang fp contract(off)
    const float ax = lx * inv[0] - oi[0], bx = hx * inv[0] - oi[0];
    const float ay = ly * inv[1] - oi[1], by = hy * inv[1] - oi[1];
    const float az = lz * inv[2] - oi[2], bz = hz * inv[2] - oi[2];
    const float t0 = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), tmin));
    const float t1 = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fminf(fmaxf(az, bz), tmax)) * 1.0000004f;
    tn = t0;
    return t0 <= t1;
}
__host__ __device__ inline void tri_test_s(const float4* tris, int k, const float o[3], const float d[3], float tmin, float& t, int& hit) {
#pragma clang fp contract(off)
    const float4 A = tris[3 * k], B = tris[3 * k + 1], C = tris[3 * k + 2];
    const float e1[3] = {B.x, B.y, B.z}, e2[3] = {C.x, C.y, C.z};
    float pv[3];
    cross3s(d, e2, pv);
    const float det = dot3s(e1, pv);
    if (det == 0.0f) return;
    const float idet = 1.0f / det;
    const float tv[3] = {o[0] - A.x, o[1] - A.y, o[2] - A.z};
    const float u = dot3s(tv, pv) * idet;
    if (!(u >= 0.0f && u <= 1.0f)) return;
    float qv[3];
    cross3s(tv, e1, qv);
    const float v = dot3s(d, qv) * idet;
    if (!(v >= 0.0f && u + v <= 1.0f)) return;
    const float tt = dot3s(e2, qv) * idet;
    if (tt > tmin && tt < t) { t = tt; hit = k; }
}
template <class Stack>
__host__ __device__ inline int trace_strict(const float4* __restrict__ nodes, const float4* __restrict__ tris, const float o[3], const float d[3],
                                            float tmin, float& t, Stack& stk) {
#pragma clang fp contract(off)
    float inv[3], oi[3];
    for (int c = 0; c < 3; ++c) {
        const float dc = fabsf(d[c]) < 1e-30f ? copysignf(1e-30f, d[c]) : d[c];
        inv[c] = 1.0f / dc;
        oi[c] = o[c] * inv[c];
    }
    int hit = -1, node = 0, sp = 0;
    while (true) {
        const float4* np = nodes + 4 * node;
        const float4 q0 = np[0], q1 = np[1], q2 = np[2], q3f = np[3];
        const int4 q3 = *reinterpret_cast<const int4*>(&q3f);
        float tn0, tn1;
        bool h0 = box_hit_s(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, inv, oi, tmin, t, tn0);
        bool h1 = box_hit_s(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, inv, oi, tmin, t, tn1);
        if (h0 && q3.z >= 0) {
            for (int k = q3.x, e = q3.x + q3.z; k < e; ++k) tri_test_s(tris, k, o, d, tmin, t, hit);
            h0 = false;
        }
        if (h1 && q3.w >= 0) {
            for (int k = q3.y, e = q3.y + q3.w; k < e; ++k) tri_test_s(tris, k, o, d, tmin, t, hit);
            h1 = false;
        }
        if (h0 && h1) {
            const bool first0 = tn0 <= tn1;
            node = first0 ? q3.x : q3.y;
            if (sp < kStack) stk[sp++] = first0 ? q3.y : q3.x;
        } else if (h0) {
            node = q3.x;
        } else if (h1) {
            node = q3.y;
        } else {
            if (sp == 0) break;
            node = stk[--sp];
        }
    }
    return hit;
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
__host__ __device__ inline float4 dn_level_pixel(const float4* __restrict__ cv, const float4* __restrict__ geom, const float* __restrict__ alb, int H,
                                                 int W, int i, int j, int s, const MatpbrPathDenoise& prm) {
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const long p = (long)i * W + j;
    const float4 cp = cv[p], xp = geom[2 * p], np_ = geom[2 * p + 1];
    const float ap[3] = {alb[3 * p], alb[3 * p + 1], alb[3 * p + 2]};
    const float lp = dn_lum(cp.x, cp.y, cp.z);
    const bool geo = np_.w != -1.0f;   // a pixel that hit nothing has no normal and no position to compare
    const float inv_c = 1.0f / (prm.sigma_c * sqrtf(fmaxf(cp.w, 0.0f)) + 1e-3f * lp + 1e-30f);
    const float inv_a = 1.0f / (prm.sigma_a * prm.sigma_a);
    const float xs = prm.sigma_x * xp.w * (float)s;
    const float w0 = h[2] * h[2];
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
            const float w = in && nq.w == np_.w ? (h[di + 2] * h[dj + 2]) * wn * dn_exp(-e) : 0.0f;
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

bool denoise_params_valid(const MatpbrPathDenoise* prm) {
    if (!prm || prm->levels < 1 || prm->levels > kDnMaxLevels) return false;
    for (float s : {prm->sigma_n, prm->sigma_x, prm->sigma_a, prm->sigma_c})
        if (!(s > 0.0f && std::isfinite(s))) return false;
    return true;
}
bool denoise_size_valid(int H, int W) { return H > 0 && W > 0 && (long)H * W <= INT32_MAX / 8; }
dim3 denoise_grid(int H, int W) { return dim3((unsigned)((W + kDnTileX - 1) / kDnTileX), (unsigned)((H + kDnTileY - 1) / kDnTileY)); }

// the arguments both feature entry points share, checked and packed
bool features_args(const void* nodes, const void* tris, int H, int W, float fov_x_deg, const MatpbrPathObject* objects, int n_objects,
                   const float* obj_nrm, long n_scene_tri, const float* nrm_map, float* geom, FeatArgs& q, ObjTable& ot) {
    int n_smooth = 0, n_pbr = 0;   // an object of kind 3 is valid here: the features read its kind and its flag, never its record
    if (!nodes || !tris || !geom || !denoise_size_valid(H, W) || !(fov_x_deg > 0.0f && fov_x_deg < 180.0f) || n_scene_tri < 0 ||
        n_scene_tri > INT32_MAX || !object_table(objects, n_objects, ot, &n_smooth, &n_pbr) || (n_smooth > 0 && !obj_nrm))
        return false;
    for (int k = 0; k < n_objects; ++k)
        if (objects[k].first_tri < n_scene_tri) return false;
    q.nodes = static_cast<const float4*>(nodes);
    q.tris = static_cast<const float4*>(tris);
    q.obj_nrm = obj_nrm;
    q.nrm_map = nrm_map;
    q.geom = reinterpret_cast<float4*>(geom);
    q.H = H; q.W = W;
    q.n_scene_tri = (int32_t)n_scene_tri;
    const double th = std::tan(0.5 * (double)fov_x_deg * 3.14159265358979323846 / 180.0);   // render_common's camera
    q.f_pix = (float)((0.5 * W) / th);
    q.cx = 0.5f * (float)(W - 1);
    q.cy = 0.5f * (float)(H - 1);
    q.f_ndc = (float)(1.0 / th);
    q.aspect = (float)W / (float)H;
    q.rho_scale = (float)(2.0 * th / W);
    return true;
}

}  // namespace

extern "C" {

int matpbr_path_features(const void* nodes, const void* tris, int H, int W, float fov_x_deg, const MatpbrPathObject* objects, int n_objects,
                         const float* obj_nrm, long n_scene_tri, const float* nrm_map, float* geom, void* stream) {
    FeatArgs q{};
    ObjTable ot{};
    if (!features_args(nodes, tris, H, W, fov_x_deg, objects, n_objects, obj_nrm, n_scene_tri, nrm_map, geom, q, ot)) return MATPBR_PATH_ERR_INVALID_ARG;
    const dim3 grid((unsigned)((W + kTileX - 1) / kTileX), (unsigned)((H + kTileY - 1) / kTileY));
    hipLaunchKernelGGL(features_kernel, grid, dim3(kTileX, kTileY), 0, (hipStream_t)stream, q, ot);
    return hipGetLastError() == hipSuccess ? MATPBR_PATH_OK : MATPBR_PATH_ERR_LAUNCH;
}

int matpbr_path_features_host(const void* nodes, const void* tris, int H, int W, float fov_x_deg, const MatpbrPathObject* objects, int n_objects,
                              const float* obj_nrm, long n_scene_tri, const float* nrm_map, float* geom) {
    FeatArgs q{};
    ObjTable ot{};
    if (!features_args(nodes, tris, H, W, fov_x_deg, objects, n_objects, obj_nrm, n_scene_tri, nrm_map, geom, q, ot)) return MATPBR_PATH_ERR_INVALID_ARG;
    for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j) {
            HostStack stk;
            float4 g0, g1;
            features_pixel(q, ot, i, j, stk, g0, g1);
            q.geom[2 * ((long)i * W + j)] = g0;
            q.geom[2 * ((long)i * W + j) + 1] = g1;
        }
    return MATPBR_PATH_OK;
}

int matpbr_path_denoise_prepare(const float* A, const float* B, const float* geom, int H, int W, float* cv0, void* stream) {
    if (!A || !B || !geom || !cv0 || !denoise_size_valid(H, W)) return MATPBR_PATH_ERR_INVALID_ARG;
    hipLaunchKernelGGL(denoise_prepare_kernel, denoise_grid(H, W), dim3(kDnTileX, kDnTileY), 0, (hipStream_t)stream, A, B,
                       reinterpret_cast<const float4*>(geom), H, W, reinterpret_cast<float4*>(cv0));
    return hipGetLastError() == hipSuccess ? MATPBR_PATH_OK : MATPBR_PATH_ERR_LAUNCH;
}

int matpbr_path_denoise_prepare_host(const float* A, const float* B, const float* geom, int H, int W, float* cv0) {
    if (!A || !B || !geom || !cv0 || !denoise_size_valid(H, W)) return MATPBR_PATH_ERR_INVALID_ARG;
    for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j)
            reinterpret_cast<float4*>(cv0)[(long)i * W + j] = dn_prepare_pixel(A, B, reinterpret_cast<const float4*>(geom), H, W, i, j);
    return MATPBR_PATH_OK;
}

int matpbr_path_denoise_level(const float* cv_in, const float* geom, const float* alb, int H, int W, const MatpbrPathDenoise* prm, int level,
                              float* cv_out, void* stream) {
    if (!cv_in || !geom || !alb || !cv_out || cv_in == cv_out || !denoise_size_valid(H, W) || !denoise_params_valid(prm) || level < 0 ||
        level >= kDnMaxLevels)
        return MATPBR_PATH_ERR_INVALID_ARG;
    hipLaunchKernelGGL(denoise_level_kernel, denoise_grid(H, W), dim3(kDnTileX, kDnTileY), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(cv_in), reinterpret_cast<const float4*>(geom), alb, H, W, 1 << level, *prm,
                       reinterpret_cast<float4*>(cv_out), (float*)nullptr, 0);
    return hipGetLastError() == hipSuccess ? MATPBR_PATH_OK : MATPBR_PATH_ERR_LAUNCH;
}

int matpbr_path_denoise_level_host(const float* cv_in, const float* geom, const float* alb, int H, int W, const MatpbrPathDenoise* prm, int level,
                                   float* cv_out) {
    if (!cv_in || !geom || !alb || !cv_out || cv_in == cv_out || !denoise_size_valid(H, W) || !denoise_params_valid(prm) || level < 0 ||
        level >= kDnMaxLevels)
        return MATPBR_PATH_ERR_INVALID_ARG;
    for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j)
            reinterpret_cast<float4*>(cv_out)[(long)i * W + j] =
                dn_level_pixel(reinterpret_cast<const float4*>(cv_in), reinterpret_cast<const float4*>(geom), alb, H, W, i, j, 1 << level, *prm);
    return MATPBR_PATH_OK;
}

size_t matpbr_path_denoise_workspace_bytes(int H, int W) {
    return denoise_size_valid(H, W) ? 2 * (size_t)H * (size_t)W * sizeof(float4) : 0;
}

int matpbr_path_denoise(const float* A, const float* B, const float* geom, const float* alb, int H, int W, const MatpbrPathDenoise* prm, float* out,
                        void* workspace, size_t workspace_bytes, void* stream) {
    if (!A || !B || !geom || !alb || !out || !workspace || !denoise_size_valid(H, W) || !denoise_params_valid(prm) ||
        workspace_bytes < matpbr_path_denoise_workspace_bytes(H, W) || ((uintptr_t)workspace & 15))
        return MATPBR_PATH_ERR_INVALID_ARG;
    const MatpbrPathDenoise pr = *prm;
    float4* ws[2] = {static_cast<float4*>(workspace), static_cast<float4*>(workspace) + (size_t)H * W};
    const float4* g = reinterpret_cast<const float4*>(geom);
    hipLaunchKernelGGL(denoise_prepare_kernel, denoise_grid(H, W), dim3(kDnTileX, kDnTileY), 0, (hipStream_t)stream, A, B, g, H, W, ws[0]);
    if (hipGetLastError() != hipSuccess) return MATPBR_PATH_ERR_LAUNCH;
    for (int l = 0; l < pr.levels; ++l) {
        const int last = l + 1 == pr.levels ? 1 : 0;
        hipLaunchKernelGGL(denoise_level_kernel, denoise_grid(H, W), dim3(kDnTileX, kDnTileY), 0, (hipStream_t)stream, (const float4*)ws[l & 1], g,
                           alb, H, W, 1 << l, pr, ws[(l + 1) & 1], out, last);
        if (hipGetLastError() != hipSuccess) return MATPBR_PATH_ERR_LAUNCH;
    }
    return MATPBR_PATH_OK;
}

}  // extern "C"
