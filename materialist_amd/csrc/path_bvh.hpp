// path_bvh.hpp -- the BVH of libmatpbr_path.so (matpbr_path.hip includes it; one translation unit): node and triangle layout, the
// closest-hit / any-hit traversal `trace` and its `fp contract(off)` twin `trace_strict`, the traversal stacks, the host builder.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/matpbr_path.h"

namespace {
constexpr int kMaxBvhDepth = MATPBR_PATH_MAX_BVH_DEPTH;
constexpr int kStack = kMaxBvhDepth;   // at most one pushed sibling per inner level of the path from the root
constexpr int kLeafMax = 4;            // triangles per leaf the builder aims for
constexpr int kBins = 16;              // SAH bins per axis
constexpr int kTileX = 16, kTileY = 8; // one workgroup = a 16 x 8 pixel tile (a wave = 16 x 4): neighbouring rays share nodes
constexpr int kBlock = kTileX * kTileY;

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

// the id a triangle carries in tris[3 k].w: its index in the input mesh
__host__ __device__ inline int tri_id(const float4& A) { return __builtin_bit_cast(int, A.w); }

// Moller-Trumbore on (v0, e1, e2); updates t / k where tmin < t' < t.  FILTER: a triangle whose id is id_limit or more is skipped
// before its test (the differential render's walk without the inserted objects, which follow the scene's triangles in the input mesh).
template <bool FILTER = false>
__host__ __device__ inline void tri_test(const float4* tris, int k, const float o[3], const float d[3], float tmin, float& t, int& hit,
                                         int id_limit = 0) {
    if (FILTER && tri_id(tris[3 * k]) >= id_limit) return;
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
// array on the host.  Pushes beyond kStack are dropped: only a BVH deeper than the builder makes could reach that.  FILTER: tri_test's;
// without it id_limit is not read and the routine is the one it was.
template <bool ANY, bool FILTER = false, class Stack>
__host__ __device__ inline int trace(const float4* __restrict__ nodes, const float4* __restrict__ tris, const float o[3], const float d[3],
                                     float tmin, float& t, Stack& stk, int id_limit = 0) {
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
            for (int k = q3.x, e = q3.x + q3.z; k < e; ++k) tri_test<FILTER>(tris, k, o, d, tmin, t, hit, id_limit);
            h0 = false;
            if (ANY && hit >= 0) return hit;
        }
        if (h1 && q3.w >= 0) {
            for (int k = q3.y, e = q3.y + q3.w; k < e; ++k) tri_test<FILTER>(tris, k, o, d, tmin, t, hit, id_limit);
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
    int level_cap = kMaxBvhDepth;           // the deepest level a slot may have: a range that reaches it becomes a leaf whatever its size
    std::vector<int32_t>* levels = nullptr; // when set: the level of every node but the root, in node order (the grafted build's refit walks by it)

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
            if (it.e - it.b <= kLeafMax || it.level >= level_cap) {
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
            if (levels) levels->push_back(it.level);
            const int m = split(it.b, it.e);
            work.push_back({q, 1, m, it.e, it.level + 1});
            work.push_back({q, 0, it.b, m, it.level + 1});
        }
        return true;
    }
};

// scene scale: the largest coordinate magnitude; boxes are padded by 1e-6 of it so that fp32 rounding of (v0, e1, e2) stays inside
inline double mesh_scale(const double* vert, long n_vert) {
    double S = 0.0;
    for (long k = 0; k < 3 * n_vert; ++k) S = std::max(S, std::fabs(vert[k]));
    return S;
}

// the builder's input: padded box and centroid of triangles [first, first + N) of the mesh, as its triangles 0 .. N - 1
inline void builder_load(Builder& bld, const double* vert, const int32_t* tri, long first, int N, float pad) {
    bld.tb.resize(N);
    bld.cen.resize(3 * (size_t)N);
    bld.idx.resize(N);
    for (int t = 0; t < N; ++t) {
        const int32_t* ix = tri + 3 * (first + t);
        Box b;
        for (int c = 0; c < 3; ++c) {
            double lo = DBL_MAX, hi = -DBL_MAX;
            for (int v = 0; v < 3; ++v) { lo = std::min(lo, vert[3 * (long)ix[v] + c]); hi = std::max(hi, vert[3 * (long)ix[v] + c]); }
            b.lo[c] = (float)lo - pad;
            b.hi[c] = (float)hi + pad;
            bld.cen[3 * t + c] = (float)(0.5 * (lo + hi));
        }
        bld.tb[t] = b;
        bld.idx[t] = t;
    }
}

// the record (v0, id) (e1, 0) (e2, 0) of triangle t of the mesh: v0, e1, e2 formed in fp64, stored fp32
inline void tri_record(const double* vert, const int32_t* tri, long t, long n_scene_tri, float4* out) {
    const double* v0 = vert + 3 * (long)tri[3 * t];
    const double* v1 = vert + 3 * (long)tri[3 * t + 1];
    const double* v2 = vert + 3 * (long)tri[3 * t + 2];
    double e1[3], e2[3];
    for (int c = 0; c < 3; ++c) { e1[c] = v1[c] - v0[c]; e2[c] = v2[c] - v0[c]; }
    const double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
    // depth mesh: e1 x e2 faces the camera at the origin; an inserted mesh keeps its winding (e1 x e2 = its outward normal)
    if (t < n_scene_tri && nx * v0[0] + ny * v0[1] + nz * v0[2] > 0.0) std::swap(e1, e2);
    const int32_t id = (int32_t)t;
    float idf;
    std::memcpy(&idf, &id, 4);
    out[0] = make_float4((float)v0[0], (float)v0[1], (float)v0[2], idf);
    out[1] = make_float4((float)e1[0], (float)e1[1], (float)e1[2], 0.0f);
    out[2] = make_float4((float)e2[0], (float)e2[1], (float)e2[2], 0.0f);
}
}  // namespace
