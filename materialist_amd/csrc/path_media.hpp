// path_media.hpp -- homogeneous media inside inserted glass meshes (matpbr_path.hip includes it; DESIGN.md section 1.4, "Media inside
// glass"): the tables of path_kernel<MediumObjects> and of the differential family with media, the trait the kernel reads them by, the
// three routines of a segment inside a medium, and the check of a record.
#pragma once
#include "path_diff.hpp"

namespace {
// TexObjects (every object rule is on) and one MatpbrPathObjectMedium per object, by value; record k is read only where object k's
// kind carries MATPBR_PATH_OBJECT_MEDIUM.
struct MediumObjects : TexObjects {
    MatpbrPathObjectMedium med[MATPBR_PATH_MAX_OBJECTS];
};
// a table of the differential family (DiffObjects, ThroughObjects, RatioObjects, RatioThroughObjects) with the same records behind it:
// the four shapes without them stay the code they are
template <class Diff>
struct MediumDiff : Diff {
    MatpbrPathObjectMedium med[MATPBR_PATH_MAX_OBJECTS];
};
// what path_kernel reads off its table's type: the table carries medium records.  False for every other table.
template <class Objects> struct MediumTraits { static constexpr bool medium = false; };
template <> struct MediumTraits<MediumObjects> { static constexpr bool medium = true; };
template <class Diff> struct MediumTraits<MediumDiff<Diff>> { static constexpr bool medium = true; };
template <class Diff> struct DiffTraits<MediumDiff<Diff>> : DiffTraits<Diff> {};

// the free flight of a medium with sigma_s > 0: the distance to the next scattering event, sampled from sigma_s alone (u in [0, 1))
__host__ __device__ inline float medium_flight(float sigma_s, float u) { return -logf(1.0f - u) / sigma_s; }
// Beer-Lambert over `dist`: the analytic weight of a segment; sigma_a = 0 gives exactly 1
__host__ __device__ inline void medium_transmittance(const float sigma_a[3], float dist, float w[3]) {
    for (int c = 0; c < 3; ++c) w[c] = expf(-sigma_a[c] * dist);
}
// One segment of length t inside the medium `mr`; u9 = dim 9 of the depth (read only where sigma_s > 0).  -> whether the segment ends
// at a medium vertex (s < t) instead of its hit, the distance flown and the weight the throughput takes.
__host__ __device__ inline bool medium_segment(const MatpbrPathObjectMedium& mr, float t, float u9, float& dist, float w[3]) {
    bool scattered = false;
    dist = t;
    if (mr.sigma_s > 0.0f) {
        const float s = medium_flight(mr.sigma_s, u9);
        if (s < t) {
            scattered = true;
            dist = s;
        }
    }
    medium_transmittance(mr.sigma_a, dist, w);
    return scattered;
}
// Henyey-Greenstein about the propagation direction d (unit length), u0, u1 = dims 10, 11: the cosine by inversion (isotropic below
// |g| = 1e-3), kept in [-1, 1] against its own rounding; phi = 2 pi u1; the frame of Duff et al. 2017 about d, object_sample's.  The
// weight of the sample is 1: the phase function is its own density.
__host__ __device__ inline void phase_sample(float g, const float d[3], float u0, float u1, float wi[3]) {
    float ct;
    if (fabsf(g) < 1e-3f) {
        ct = 1.0f - 2.0f * u0;
    } else {
        const float q = (1.0f - g * g) / (1.0f - g + 2.0f * g * u0);
        ct = (1.0f + g * g - q * q) / (2.0f * g);
    }
    ct = fminf(fmaxf(ct, -1.0f), 1.0f);
    const float st = sqrtf(fmaxf(1.0f - ct * ct, 0.0f));
    const float ph = 6.28318530717958647692f * u1;
    const float x = st * cosf(ph), y = st * sinf(ph);
    const float sg = copysignf(1.0f, d[2]), a = -1.0f / (sg + d[2]), b = d[0] * d[1] * a;
    const float s[3] = {1.0f + sg * d[0] * d[0] * a, sg * b, -sg * d[0]}, t[3] = {b, sg + d[1] * d[1] * a, -d[1]};
    for (int c = 0; c < 3; ++c) wi[c] = s[c] * x + t[c] * y + d[c] * ct;
}

// the index of the object whose range holds triangle `id` where its kind carries the medium flag, else -1
__host__ __device__ inline int medium_index(const ObjTable& ot, int id) {
    int idx = -1;
    object_match(ot, id, [&](int k, const MatpbrPathObject& ob) {
        if (ob.kind & MATPBR_PATH_OBJECT_MEDIUM) idx = k;
    });
    return idx;
}
// record m of the table, by unrolled selects: no indexed private array
template <class Table>
__device__ __forceinline__ MatpbrPathObjectMedium medium_of(const Table& ot, int m) {
    MatpbrPathObjectMedium r{};
#pragma unroll
    for (int k = 0; k < MATPBR_PATH_MAX_OBJECTS; ++k) {
        if (k == m) {
            r.sigma_a[0] = ot.med[k].sigma_a[0]; r.sigma_a[1] = ot.med[k].sigma_a[1]; r.sigma_a[2] = ot.med[k].sigma_a[2];
            r.sigma_s = ot.med[k].sigma_s;
            r.g = ot.med[k].g;
        }
    }
    return r;
}

// a record: sigma_a and sigma_s finite and >= 0 (0 is valid), |g| <= 0.99, reserved == 0 (a NaN fails every comparison)
bool medium_valid(const MatpbrPathObjectMedium& mr) {
    for (int c = 0; c < 3; ++c)
        if (!(mr.sigma_a[c] >= 0.0f && std::isfinite(mr.sigma_a[c])) || mr.reserved[c] != 0.0f) return false;
    return mr.sigma_s >= 0.0f && std::isfinite(mr.sigma_s) && fabsf(mr.g) <= 0.99f;
}
// what a table with a flagged object needs besides the flag's place (object_table): the records, and a valid one for every flagged object
bool media_valid(const MatpbrPathObject* objects, int n_objects, const MatpbrPathObjectMedium* media) {
    if (!media) return false;
    for (int k = 0; k < n_objects; ++k)
        if ((objects[k].kind & MATPBR_PATH_OBJECT_MEDIUM) && !medium_valid(media[k])) return false;
    return true;
}
// whether some flagged object's record absorbs or scatters at all
bool media_any(const MatpbrPathObject* objects, int n_objects, const MatpbrPathObjectMedium* media) {
    for (int k = 0; k < n_objects; ++k) {
        if (!(objects[k].kind & MATPBR_PATH_OBJECT_MEDIUM)) continue;
        const MatpbrPathObjectMedium& mr = media[k];
        if (mr.sigma_a[0] > 0.0f || mr.sigma_a[1] > 0.0f || mr.sigma_a[2] > 0.0f || mr.sigma_s > 0.0f) return true;
    }
    return false;
}
}  // namespace
