// path_lights.hpp -- emissive inserted objects ("Emissive inserted objects"; matpbr_path.hip includes it): the
// light tables the kernel takes by value, the emitter choice, the area sampler, both solid-angle pdfs, the checks of what the caller
// passes and the host builder of the tables.  The sampler and the pdfs are __host__ __device__ (plain divisions and sqrtf): the CPU
// entry points run what the kernel runs.
#pragma once
#include "path_objects.hpp"

namespace {
constexpr int kMaxLights = MATPBR_PATH_MAX_OBJECTS;
constexpr float kShadowEps = 1e-3f;           // a light's shadow ray ends at dist (1 - kShadowEps): the scale of Mitsuba's ShadowEpsilon
constexpr float kBelowOne = 0.99999994f;      // 1 - 2^-24: the re-used emitter coordinate stays below 1

// The header travels to the kernel by value; the triangle records (the BVH's layout: (v0, 0) (e1, 0) (e2, 0), input order, light after
// light) and the cumulative areas (per light, upper bounds, the last one exactly 1) are device buffers.
struct LightTable {
    const float4* tri;   // [n_light_tri, 3]
    const float* cdf;    // [n_light_tri]
    int32_t n;           // lights: the kind-4 objects in table order
    int32_t first[kMaxLights], n_tri[kMaxLights];   // light l's records: [first, first + n_tri)
    float area[kMaxLights];                         // light l's area, summed in fp64
    float rad[kMaxLights][3];                       // light l's radiance: its object's p
    float obj_area[MATPBR_PATH_MAX_OBJECTS];        // object k's area where it is a light: the hit side's lookup
};
struct LightObjects : PbrObjects {
    LightTable lt;
};
// the table of a scene with a rough dielectric object (kind 5): the light table may be empty then (lt.n = 0)
struct RoughObjects : LightObjects {};
// the table of a scene with a vertex-coloured object ("Vertex-coloured inserted objects"): the superset table
struct ColorObjects : RoughObjects {
    const float* col;   // [n_tri - n_scene_tri, 3, 3]: one linear RGB triple per corner of every inserted triangle
};

// emitter `idx` of n_e by sample reuse: idx = min(int(u n_e), n_e - 1), u' = u n_e - idx kept below 1
__host__ __device__ inline int emitter_choose(float u, int n_e, float& u_re) {
    const float x = u * (float)n_e;
    int idx = (int)x;
    if (idx > n_e - 1) idx = n_e - 1;
    u_re = fminf(x - (float)idx, kBelowOne);
    return idx;
}
// the first of n entries with cdf[t] > u (cdf[n - 1] = 1 > u): a zero-area triangle repeats its predecessor's bound and is never chosen
__host__ __device__ inline int light_triangle(const float* cdf, int n, float u) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] > u) hi = mid; else lo = mid + 1;
    }
    return lo;
}
// A point of light l seen from po: the triangle by u_tri in l's cumulative areas, y = v0 + (1 - s) e1 + s u4 e2 with s = sqrt(1 - u3);
// wl = normalize(y - po), dist = |y - po|, pdf = dist^2 / (A cos_l n_e) with cos_l = n_l . (-wl), 0 where cos_l <= 0 or dist = 0.
// Returns the record's index.  The header's fields are unrolled selects over wave-uniform reads: no indexed private array.
__host__ __device__ inline int light_sample(const LightTable& lt, int l, float u_tri, float u3, float u4, const float po[3], float n_e, float y[3],
                                            float wl[3], float& dist, float& pdf) {
    int first = 0, n = 1;
    float area = 0.0f;
#pragma unroll
    for (int k = 0; k < kMaxLights; ++k)
    {
        first = k == l ? lt.first[k] : first;
        n = k == l ? lt.n_tri[k] : n;
        area = k == l ? lt.area[k] : area;
    }
    const int t = first + light_triangle(lt.cdf + first, n, u_tri);
    const float4 A = lt.tri[3 * t], B = lt.tri[3 * t + 1], C = lt.tri[3 * t + 2];
    const float e1[3] = {B.x, B.y, B.z}, e2[3] = {C.x, C.y, C.z};
    const float s = sqrtf(fmaxf(1.0f - u3, 0.0f));
    const float b1 = 1.0f - s, b2 = s * u4;
    y[0] = A.x + b1 * e1[0] + b2 * e2[0];
    y[1] = A.y + b1 * e1[1] + b2 * e2[1];
    y[2] = A.z + b1 * e1[2] + b2 * e2[2];
    const float dv[3] = {y[0] - po[0], y[1] - po[1], y[2] - po[2]};
    const float d2 = dot3h(dv, dv);
    dist = sqrtf(d2);
    pdf = 0.0f;
    wl[0] = wl[1] = wl[2] = 0.0f;
    if (!(dist > 0.0f)) return t;
    const float id = 1.0f / dist;
    for (int c = 0; c < 3; ++c) wl[c] = dv[c] * id;
    float nl[3];
    cross3(e1, e2, nl);
    const float cos_l = -dot3h(nl, wl) / sqrtf(dot3h(nl, nl));
    if (cos_l > 0.0f) pdf = d2 / (area * cos_l * n_e);
    return t;
}
// the solid-angle pdf the sampler gives a ray that lands on a light's front after t: t^2 / (A (ng . wo) n_e)
__host__ __device__ inline float light_hit_pdf(float t, float area, float cos_o, float n_e) { return (t * t) / (area * cos_o * n_e); }

// object_lookup for the light table, returned by value: kind, p (a light's radiance), a PBR object's record as there, and the area of
// an object that is a light.  One walk for every kind.
struct LightLookup {
    int kind;
    float p0, p1, p2, a0, a1, a2, r, m, area;
};
// FLAGS: the bits a kind may carry beside its BSDF (the colour table's kinds carry MATPBR_PATH_OBJECT_COLORED as well)
template <int FLAGS = MATPBR_PATH_OBJECT_SMOOTH>
__host__ __device__ inline LightLookup light_lookup(const LightObjects& lo, int id) {
    LightLookup f{0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    object_match(lo.t, id, [&](int k, const MatpbrPathObject& ob) {
        f.kind = ob.kind;
        f.p0 = ob.p[0]; f.p1 = ob.p[1]; f.p2 = ob.p[2];
        if ((ob.kind & ~FLAGS) == MATPBR_PATH_BSDF_PBR) {
            f.a0 = lo.pbr[k].a[0]; f.a1 = lo.pbr[k].a[1]; f.a2 = lo.pbr[k].a[2];
            f.r = lo.pbr[k].r;
            f.m = lo.pbr[k].m;
        }
        if (ob.kind == MATPBR_PATH_BSDF_AREA) f.area = lo.lt.obj_area[k];
    });
    return f;
}
// light l's radiance, by the same selects
__host__ __device__ inline void light_radiance(const LightTable& lt, int l, float rad[3]) {
#pragma unroll
    for (int k = 0; k < kMaxLights; ++k)
        for (int c = 0; c < 3; ++c) rad[c] = k == l ? lt.rad[k][c] : rad[c];
}

// Moller-Trumbore's t of the ray o + t d on record k's plane, tri_test's operations without its bounds (FLT_MAX where det = 0)
__host__ __device__ inline float tri_t(const float4* tris, int k, const float o[3], const float d[3]) {
    const float4 A = tris[3 * k], B = tris[3 * k + 1], C = tris[3 * k + 2];
    const float e1[3] = {B.x, B.y, B.z}, e2[3] = {C.x, C.y, C.z};
    float pv[3], qv[3];
    cross3(d, e2, pv);
    const float det = dot3h(e1, pv);
    if (det == 0.0f) return FLT_MAX;
    const float tv[3] = {o[0] - A.x, o[1] - A.y, o[2] - A.z};
    cross3(tv, e1, qv);
    return dot3h(e2, qv) * (1.0f / det);
}

// The caller's header -> the kernel's table (tri / cdf are the caller's device or host buffers): the records of the lights follow each
// other from 0, every area is finite and positive.  With `ot`, the (checked) table: the lights are its kind-4 objects in table order,
// n_tri the object's, cdf is needed, and the radiances and the objects' areas are filled in.  Without (the CPU entry points, which have
// no table): the header is checked against itself alone.  *n_light_tri: the records it counts.
bool light_table(const MatpbrPathLights* h, const ObjTable* ot, const void* tri, const float* cdf, LightTable& lt, long* n_light_tri = nullptr) {
    if (!h || !tri || (ot && !cdf) || ((uintptr_t)tri & 15) || h->n_lights < 1 || h->n_lights > kMaxLights) return false;
    lt = LightTable{};
    lt.tri = static_cast<const float4*>(tri);
    lt.cdf = cdf;
    lt.n = h->n_lights;
    int l = 0;
    long first = 0;
    for (int k = 0; k < (ot ? ot->n : h->n_lights); ++k) {
        if (ot && ot->o[k].kind != MATPBR_PATH_BSDF_AREA) continue;
        if (l >= h->n_lights || h->first[l] != first || h->n_tri[l] < 1 || !(h->area[l] > 0.0f) || !std::isfinite(h->area[l])) return false;
        lt.first[l] = h->first[l];
        lt.n_tri[l] = h->n_tri[l];
        lt.area[l] = h->area[l];
        first += h->n_tri[l];
        if (ot) {
            if (h->object[l] != k || h->n_tri[l] != ot->o[k].n_tri || first > INT32_MAX) return false;
            lt.obj_area[k] = h->area[l];
            for (int c = 0; c < 3; ++c) lt.rad[l][c] = ot->o[k].p[c];
        }
        ++l;
    }
    if (n_light_tri) *n_light_tri = first;
    return l == h->n_lights;
}

// The host builder: per light the area (fp64), the records in input order (the BVH's rounding: v0, e1, e2 formed in fp64, stored
// fp32; an inserted mesh keeps its winding) and the cumulative areas / A (fp64 sums, stored fp32, everything from the last triangle
// of positive area on exactly 1).  tris == NULL: the header and the count alone.
int light_tables_build(const double* vert, long n_vert, const int32_t* tri, long n_tri, const ObjTable& ot, MatpbrPathLights* h, float* tris,
                       float* cdf, long capacity, long* n_light_tri) {
    *h = MatpbrPathLights{};
    long first = 0;
    for (int k = 0; k < ot.n; ++k) {
        const MatpbrPathObject& ob = ot.o[k];
        if (ob.kind != MATPBR_PATH_BSDF_AREA) continue;
        if (ob.n_tri < 1 || (long)ob.first_tri + ob.n_tri > n_tri) return MATPBR_PATH_ERR_INVALID_ARG;
        std::vector<double> a(ob.n_tri);
        double A = 0.0;
        for (int t = 0; t < ob.n_tri; ++t) {
            const int32_t* ix = tri + 3 * ((long)ob.first_tri + t);
            for (int v = 0; v < 3; ++v)
                if (ix[v] < 0 || ix[v] >= n_vert) return MATPBR_PATH_ERR_INVALID_ARG;
            const double *v0 = vert + 3 * (long)ix[0], *v1 = vert + 3 * (long)ix[1], *v2 = vert + 3 * (long)ix[2];
            double e1[3], e2[3];
            for (int c = 0; c < 3; ++c) { e1[c] = v1[c] - v0[c]; e2[c] = v2[c] - v0[c]; }
            const double nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
            a[t] = 0.5 * std::sqrt(nx * nx + ny * ny + nz * nz);
            A += a[t];
            if (tris) {
                if (first + t >= capacity) return MATPBR_PATH_ERR_CAPACITY;
                float* rec = tris + 12 * (first + t);
                for (int c = 0; c < 3; ++c) { rec[c] = (float)v0[c]; rec[4 + c] = (float)e1[c]; rec[8 + c] = (float)e2[c]; }
                rec[3] = rec[7] = rec[11] = 0.0f;
            }
        }
        if (!(A > 0.0) || !std::isfinite(A) || !((float)A > 0.0f) || !std::isfinite((float)A)) return MATPBR_PATH_ERR_INVALID_ARG;   // a light of area 0
        if (tris) {
            int last = 0;
            for (int t = 0; t < ob.n_tri; ++t)
                if (a[t] > 0.0) last = t;
            double run = 0.0;
            for (int t = 0; t < ob.n_tri; ++t) {
                run += a[t];
                cdf[first + t] = t >= last ? 1.0f : fminf((float)(run / A), 1.0f);
            }
        }
        const int l = h->n_lights++;
        h->object[l] = k;
        h->first[l] = (int32_t)first;
        h->n_tri[l] = ob.n_tri;
        h->area[l] = (float)A;
        first += ob.n_tri;
        if (first > INT32_MAX) return MATPBR_PATH_ERR_INVALID_ARG;
    }
    *n_light_tri = first;
    return MATPBR_PATH_OK;
}
}  // namespace
