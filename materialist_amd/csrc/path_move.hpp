// path_move.hpp -- moving inserted objects ("Moving inserted objects"; matpbr_path.hip includes it): the grafted
// BVH's host build, the per-object similarity and its checks, the move of the object triangles, corner normals and light records from
// their rest pose, and the bottom-up refit of the object nodes' boxes.  The per-triangle and per-slot routines are __host__ __device__
// under `fp contract(off)` (every product and sum rounded on its own, as trace_strict's): matpbr_path_objects_move_host runs what
// the kernels run and gives the same bits.  The render kernels are not touched: nodes, triangles, corner normals and light records
// keep their layouts.
#pragma once
#include "path_lights.hpp"

namespace {
constexpr int kRefitBlock = 1024;             // the refit's one workgroup
constexpr double kXformOrtho = 1e-5;          // |R_i . R_j - delta_ij| at most this

// ---- the similarity p' = R (s (p - c)) + c + t ----------------------------------------------------------------------------------
// The corner normals are turned by R alone and not renormalised.  That relies on kXformOrtho: a row product within 1e-5 of the
// identity's keeps |R n| within 2e-5 of 1 (three row errors of 1e-5 at most), which shading_normal's own normalisation of the
// interpolated normal absorbs; every consumer of obj_nrm normalises after interpolating and none assumes unit corners.
inline bool xform_ok(const MatpbrPathXform& x) {
    const float* f = x.R;
    for (int k = 0; k < 9; ++k)
        if (!std::isfinite(f[k])) return false;
    if (!std::isfinite(x.s) || !(x.s > 0.0f)) return false;
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(x.t[k]) || !std::isfinite(x.c[k])) return false;
    const double R[9] = {f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8]};
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j) {
            const double d = R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1] + R[3 * i + 2] * R[3 * j + 2];
            if (!(std::fabs(d - (i == j ? 1.0 : 0.0)) <= kXformOrtho)) return false;
        }
    const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
    return det > 0.0;   // a mirror (det = -1) would flip every winding
}
// exactly the identity: the object is left at rest, its records are copied (p - c + c is not p in floating point)
inline bool xform_rest(const MatpbrPathXform& x) {
    static const float I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int k = 0; k < 9; ++k)
        if (x.R[k] != I[k]) return false;
    return x.s == 1.0f && x.t[0] == 0.0f && x.t[1] == 0.0f && x.t[2] == 0.0f;
}

// What the move kernel takes by value: per object its range of triangle ids, its similarity, whether it is smooth, whether it is left
// at rest; per light the object it is and its range of light records.
struct MoveTable {
    MatpbrPathXform x[MATPBR_PATH_MAX_OBJECTS];
    int32_t first[MATPBR_PATH_MAX_OBJECTS], n_tri[MATPBR_PATH_MAX_OBJECTS];
    int32_t smooth[MATPBR_PATH_MAX_OBJECTS], rest[MATPBR_PATH_MAX_OBJECTS];
    int32_t n;
    int32_t light_object[MATPBR_PATH_MAX_OBJECTS], light_first[MATPBR_PATH_MAX_OBJECTS], light_n[MATPBR_PATH_MAX_OBJECTS];
    int32_t n_lights;
};

// The transform runs in fp64 on the fp32 inputs and is rounded once: the kernels are bound by their 96 bytes of traffic per triangle,
// not by some fifty fp64 operations, fp64 sums and products are IEEE on both sides (the same bits on the CPU and on the device under
// `fp contract(off)`), and a coordinate comes out within half an ulp of the exact transform plus 2^-50 of the largest term.
__host__ __device__ inline void xform_point(const MatpbrPathXform& x, float px, float py, float pz, float out[3]) {
#pragma clang fp contract(off)
    const double s = x.s;
    const double q0 = s * ((double)px - (double)x.c[0]), q1 = s * ((double)py - (double)x.c[1]), q2 = s * ((double)pz - (double)x.c[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double r = ((double)x.R[3 * i] * q0 + (double)x.R[3 * i + 1] * q1) + (double)x.R[3 * i + 2] * q2;
        out[i] = (float)(r + ((double)x.c[i] + (double)x.t[i]));
    }
}
// R (s e): an edge (s = x.s) or a normal (s = 1)
__host__ __device__ inline void xform_vector(const MatpbrPathXform& x, double s, float ex, float ey, float ez, float out[3]) {
#pragma clang fp contract(off)
    const double q0 = s * (double)ex, q1 = s * (double)ey, q2 = s * (double)ez;
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = (float)(((double)x.R[3 * i] * q0 + (double)x.R[3 * i + 1] * q1) + (double)x.R[3 * i + 2] * q2);
}
// the record (v0, w) (e1, 0) (e2, 0) moved; w (the id, or a light record's 0) is kept
__host__ __device__ inline void move_record(const MatpbrPathXform& x, const float4* in, float4* out) {
    const float4 A = in[0], B = in[1], C = in[2];
    float v[3], e1[3], e2[3];
    xform_point(x, A.x, A.y, A.z, v);
    xform_vector(x, (double)x.s, B.x, B.y, B.z, e1);
    xform_vector(x, (double)x.s, C.x, C.y, C.z, e2);
    out[0] = make_float4(v[0], v[1], v[2], A.w);
    out[1] = make_float4(e1[0], e1[1], e1[2], B.w);
    out[2] = make_float4(e2[0], e2[1], e2[2], C.w);
}
__host__ __device__ inline void copy_record(const float4* in, float4* out) {
    const float4 A = in[0], B = in[1], C = in[2];
    out[0] = A; out[1] = B; out[2] = C;
}

// Object triangle k (leaf order): tris[n_scene_tri + k] from rest_tris[k], and the nine corner normals of a smooth object's triangle
// (input order: indexed by id - n_scene_tri).  A triangle in no object's range, or in the range of an object at rest, is copied.
__host__ __device__ inline void move_triangle(const MoveTable& mt, long k, const float4* rest_tris, float4* tris, long n_scene_tri, long n_object_tri,
                                              const float* rest_nrm, float* obj_nrm) {
    const float4* in = rest_tris + 3 * k;
    float4* out = tris + 3 * (n_scene_tri + k);
    const int id = tri_id(in[0]);
    const long j = (long)id - n_scene_tri;
    int ob = -1;
    for (int o = 0; o < mt.n; ++o)
        if (id >= mt.first[o] && id - mt.first[o] < mt.n_tri[o]) ob = o;
    const bool normals = ob >= 0 && mt.smooth[ob] && rest_nrm && obj_nrm && j >= 0 && j < n_object_tri;
    if (ob < 0 || mt.rest[ob]) {
        copy_record(in, out);
        if (normals)
            for (int c = 0; c < 9; ++c) obj_nrm[9 * j + c] = rest_nrm[9 * j + c];
        return;
    }
    const MatpbrPathXform& x = mt.x[ob];
    move_record(x, in, out);
    if (normals)
        for (int c = 0; c < 3; ++c) {
            const float* n = rest_nrm + 9 * j + 3 * c;
            xform_vector(x, 1.0, n[0], n[1], n[2], obj_nrm + 9 * j + 3 * c);
        }
}
// Light record r: light_tris[r] from rest_light_tris[r] under its object's similarity: move_record's arithmetic on the records the
// light tables hold, which are the BVH's (v0, e1, e2), so the moved record equals the moved triangle of the same id bit for bit.
__host__ __device__ inline void move_light_record(const MoveTable& mt, long r, const float4* rest_light_tris, float4* light_tris) {
    int ob = -1;
    for (int l = 0; l < mt.n_lights; ++l)
        if (r >= mt.light_first[l] && r - mt.light_first[l] < mt.light_n[l]) ob = mt.light_object[l];
    if (ob < 0 || mt.rest[ob]) copy_record(rest_light_tris + 3 * r, light_tris + 3 * r);
    else move_record(mt.x[ob], rest_light_tris + 3 * r, light_tris + 3 * r);
}

// ---- the refit rule ----------------------------------------------------------------------------------------------------------------
// A leaf slot's box: min / max over its triangles of v0, fl(v0 + e1), fl(v0 + e2) in fp32, widened by pad = 1e-6 S, S the largest
// coordinate magnitude of the scene and of every announced pose.  Why pad suffices: the triangle test meets points of the exact
// triangle (v0, v0 + e1, v0 + e2).  fl(v0 + e) differs from v0 + e by half an ulp of a number of magnitude <= S, at most 2^-24 S =
// 6e-8 S; fl(lo - pad) and fl(hi + pad) round by as much again.  Together 1.2e-7 S, an eighth of pad.  Against the fp64 transform of
// the rest record (what the tests hold the boxes to), the rounding of v0' and of e' adds half an ulp each: 2.4e-7 S, a quarter of pad.
// min and max do not depend on the order of their operands, so no order of the threads changes a bit.
__host__ __device__ inline void leaf_box(const float4* tris, int first, int count, float pad, float b[6]) {
#pragma clang fp contract(off)
    if (count <= 0) {
        for (int c = 0; c < 6; ++c) b[c] = 0.0f;
        return;
    }
    float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int k = first; k < first + count; ++k) {
        const float4 A = tris[3 * k], B = tris[3 * k + 1], C = tris[3 * k + 2];
        const float v0[3] = {A.x, A.y, A.z}, e1[3] = {B.x, B.y, B.z}, e2[3] = {C.x, C.y, C.z};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float p1 = v0[c] + e1[c], p2 = v0[c] + e2[c];
            lo[c] = fminf(lo[c], fminf(v0[c], fminf(p1, p2)));
            hi[c] = fmaxf(hi[c], fmaxf(v0[c], fmaxf(p1, p2)));
        }
    }
    for (int c = 0; c < 3; ++c) { b[c] = lo[c] - pad; b[3 + c] = hi[c] + pad; }
}
// an inner slot's box: the union of its child's two boxes
__host__ __device__ inline void union_box(const BNode& child, float b[6]) {
    for (int c = 0; c < 3; ++c) {
        b[c] = fminf(child.b[c], child.b[6 + c]);
        b[3 + c] = fmaxf(child.b[3 + c], child.b[9 + c]);
    }
}
// the leaf slots of one node (any level: they read triangles alone)
__host__ __device__ inline void refit_leaf_slots(BNode* nodes, long node, const float4* tris, float pad) {
    BNode& nd = nodes[node];
    for (int s = 0; s < 2; ++s)
        if (nd.count[s] >= 0) {
            float b[6];
            leaf_box(tris, nd.child[s], nd.count[s], pad, b);
            for (int c = 0; c < 6; ++c) nd.b[6 * s + c] = b[c];
        }
}
// the inner slots of one node, once its children's boxes stand
__host__ __device__ inline void refit_inner_slots(BNode* nodes, long node) {
    BNode& nd = nodes[node];
    for (int s = 0; s < 2; ++s)
        if (nd.count[s] < 0) {
            float b[6];
            union_box(nodes[nd.child[s]], b);
            for (int c = 0; c < 6; ++c) nd.b[6 * s + c] = b[c];
        }
}
// slot 1 of node 0, last: the object side's leaf, or the union over the object subtree's root
__host__ __device__ inline void refit_graft_slot(BNode* nodes, const float4* tris, float pad) {
    float b[6];
    if (nodes[0].count[1] >= 0) leaf_box(tris, nodes[0].child[1], nodes[0].count[1], pad, b);
    else union_box(nodes[nodes[0].child[1]], b);
    for (int c = 0; c < 6; ++c) nodes[0].b[6 + c] = b[c];
}

// ---- the kernels -------------------------------------------------------------------------------------------------------------------
// One thread per object triangle, then one per light record.  Plain vector loads and stores; nothing is read that this launch writes.
__global__ void __launch_bounds__(256) objects_move_kernel(MoveTable mt, const float4* __restrict__ rest_tris, float4* __restrict__ tris, long n_scene_tri,
                                                           long n_object_tri, const float* __restrict__ rest_nrm, float* __restrict__ obj_nrm,
                                                           const float4* __restrict__ rest_light_tris, float4* __restrict__ light_tris, long n_light_tri) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_object_tri) move_triangle(mt, i, rest_tris, tris, n_scene_tri, n_object_tri, rest_nrm, obj_nrm);
    else if (i - n_object_tri < n_light_tri) move_light_record(mt, i - n_object_tri, rest_light_tris, light_tris);
}

// One workgroup walks the object nodes: every leaf slot first, then the inner slots level by level from the deepest up, a barrier
// between levels, slot 1 of node 0 last.  A node's boxes are written by one thread and read, a level later, by another thread of the
// same workgroup: __syncthreads() orders them.  It is a workgroup-scope release and acquire around the barrier (the stores are
// waited for before it, and the compiler carries no global value across it); a workgroup's waves run on one compute unit and share
// its vector L1, which a store writes through, so the later load sees the line (the memory model's workgroup scope outside
// threadgroup-split mode, which HIP does not launch in).  `nodes` is neither const nor __restrict__ here: nothing lets the compiler
// read it through the scalar cache, which vector stores do not update.  Inserted meshes are small, so one workgroup needs neither a
// grid-wide wait nor a launch per level.  The scene's nodes and triangles are never written.
__global__ void __launch_bounds__(kRefitBlock) objects_refit_kernel(BNode* nodes, const float4* tris, long first_object_node, long n_object_nodes,
                                                                    const int32_t* __restrict__ node_level, int depth, float pad) {
    for (long i = threadIdx.x; i < n_object_nodes; i += kRefitBlock) refit_leaf_slots(nodes, first_object_node + i, tris, pad);
    for (int level = depth - 1; level >= 1; --level) {
        __syncthreads();
        for (long i = threadIdx.x; i < n_object_nodes; i += kRefitBlock)
            if (node_level[i] == level) refit_inner_slots(nodes, first_object_node + i);
    }
    __syncthreads();
    if (threadIdx.x == 0) refit_graft_slot(nodes, tris, pad);
}

// the CPU twin of both kernels, with their routines in the same dependency order
inline void objects_move_host(const MoveTable& mt, BNode* nodes, float4* tris, const float4* rest_tris, long n_scene_tri, long n_object_tri,
                              long first_object_node, long n_object_nodes, const int32_t* node_level, int depth, float pad, const float* rest_nrm,
                              float* obj_nrm, const float4* rest_light_tris, float4* light_tris, long n_light_tri) {
    for (long k = 0; k < n_object_tri; ++k) move_triangle(mt, k, rest_tris, tris, n_scene_tri, n_object_tri, rest_nrm, obj_nrm);
    for (long r = 0; r < n_light_tri; ++r) move_light_record(mt, r, rest_light_tris, light_tris);
    for (long i = 0; i < n_object_nodes; ++i) refit_leaf_slots(nodes, first_object_node + i, tris, pad);
    for (int level = depth - 1; level >= 1; --level)
        for (long i = 0; i < n_object_nodes; ++i)
            if (node_level[i] == level) refit_inner_slots(nodes, first_object_node + i);
    refit_graft_slot(nodes, tris, pad);
}

// The caller's arguments -> the kernel's table; false for what matpbr_path_objects_move refuses.  `lights` NULL: no light records.
inline bool move_table(const MatpbrPathObject* objects, int n_objects, const MatpbrPathXform* xform, long n_scene_tri, long n_object_tri,
                       const float* rest_nrm, float* obj_nrm, const MatpbrPathLights* lights, long n_light_tri, MoveTable& mt) {
    if (!objects || !xform || n_objects < 1 || n_objects > MATPBR_PATH_MAX_OBJECTS) return false;
    mt = MoveTable{};
    mt.n = n_objects;
    for (int k = 0; k < n_objects; ++k) {
        const MatpbrPathObject& ob = objects[k];
        if (ob.n_tri < 1 || ob.first_tri < n_scene_tri || (long)ob.first_tri + ob.n_tri > n_scene_tri + n_object_tri) return false;
        for (int j = 0; j < k; ++j)
            if (ob.first_tri < objects[j].first_tri + objects[j].n_tri && objects[j].first_tri < ob.first_tri + ob.n_tri) return false;
        if (!xform_ok(xform[k])) return false;
        mt.x[k] = xform[k];
        mt.first[k] = ob.first_tri;
        mt.n_tri[k] = ob.n_tri;
        mt.smooth[k] = (ob.kind & MATPBR_PATH_OBJECT_SMOOTH) != 0;
        mt.rest[k] = xform_rest(xform[k]);
        if (mt.smooth[k] && (!rest_nrm || !obj_nrm)) return false;
    }
    if (!lights) return n_light_tri == 0;
    if (lights->n_lights < 0 || lights->n_lights > kMaxLights) return false;
    mt.n_lights = lights->n_lights;
    long first = 0;
    for (int l = 0; l < lights->n_lights; ++l) {
        const int ob = lights->object[l];
        if (ob < 0 || ob >= n_objects || lights->first[l] != first || lights->n_tri[l] != objects[ob].n_tri) return false;
        mt.light_object[l] = ob;
        mt.light_first[l] = lights->first[l];
        mt.light_n[l] = lights->n_tri[l];
        first += lights->n_tri[l];
    }
    return first == n_light_tri;
}
}  // namespace
