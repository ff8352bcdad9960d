// path_objects.hpp -- the tables that travel to libmatpbr_path.so's kernels by value (matpbr_path.hip includes it) and everything that
// operates on them: inserted objects (flat, smooth, PBR, rough dielectric), the transparency edit, the shading-normal map; their lookups, samplers and
// the checks of what the caller passes.
#pragma once
#include "path_shading.hpp"

namespace {
// ---- inserted objects ("Inserted objects"): Mitsuba's smooth `dielectric` and `diffuse` ------------------
// The table travels to the kernel by value.  An id (the triangle's index in the input mesh) in no range is the depth mesh's.
struct ObjTable {
    MatpbrPathObject o[MATPBR_PATH_MAX_OBJECTS];
    int32_t n, min_id;   // min_id: the smallest first_tri, below which no lookup is needed
};
struct NoObjects {};   // the kernel's table when there is none
constexpr int kFlagDelta = 1, kFlagTransmitted = 2;

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

// ---- PBR inserted objects ("PBR inserted objects") --------------------------------------------------------
// An object of kind MATPBR_PATH_BSDF_PBR shades as the depth mesh does, MatDiffBSDF, on the constants of its record instead of a
// texel's.  MatpbrPathObject is frozen, so the eight records travel to the kernel by value beside the smooth table.
struct PbrObjects : SmoothObjects {
    MatpbrPathObjectPbr pbr[MATPBR_PATH_MAX_OBJECTS];
};

// ---- transparency editing ("Transparency editing"): TransBSDF (myutils/mi_plugin.py:1477-1771) -----------
// Where mask[tp] is set the depth mesh shades as a sheet of glass in front of the photograph `bg`, read at the texel a ray refracted
// twice through the sheet lands on.  The edit travels to the kernel by value, in the place of the object table.  The masked-branch
// arithmetic and the lookup are __host__ __device__ (plain divisions and sqrtf): the CPU entry points run what the kernel runs.
struct TransEdit {
    const uint8_t* mask;   // [H,W], non-zero = edited
    const float* bg;       // [H,W,3]
    float ior, spec_trans, refract_distance;
};

// ---- shading normals ("Shading normals") -------------------------------------------------------------------
// The map travels to the kernel in the table's place.  A vertex then has two normals: ng, the face normal, keeps everything geometric
// (the back-face test, the spawn offset, which side a direction leaves on); ns = nrm[tp] takes the place of MatDiffBSDF's `normal`.
struct ShadeNormals {
    const float* nrm;   // [H,W,3], unit length, used as given
};

// ---- the table lookups: one walk, three readers ----------------------------------------------------------------------------------------
// found(k, ob) for every object whose range holds triangle `id` (ranges do not overlap: at most one).  Unrolled selects over
// wave-uniform table reads: no indexed private array.
template <class F>
__host__ __device__ __forceinline__ void object_match(const ObjTable& ot, int id, F found) {
    if (id < ot.min_id) return;
#pragma unroll
    for (int k = 0; k < MATPBR_PATH_MAX_OBJECTS; ++k) {
        const MatpbrPathObject& ob = ot.o[k];
        if (k < ot.n && id >= ob.first_tri && id - ob.first_tri < ob.n_tri) found(k, ob);
    }
}
// kind and parameters of triangle `id` (0: the depth mesh)
__device__ __forceinline__ int object_of(const NoObjects&, int, float[3]) { return 0; }
__device__ __forceinline__ int object_of(const ObjTable& ot, int id, float p[3]) {
    int kind = 0;
    object_match(ot, id, [&](int, const MatpbrPathObject& ob) {
        kind = ob.kind;
        p[0] = ob.p[0]; p[1] = ob.p[1]; p[2] = ob.p[2];
    });
    return kind;
}
// object_of for the smooth table: the kind still carries the flag bit
__device__ __forceinline__ int object_of(const SmoothObjects& so, int id, float p[3]) { return object_of(so.t, id, p); }
__device__ __forceinline__ int object_of(const TransEdit&, int, float[3]) { return 0; }
__device__ __forceinline__ int object_of(const ShadeNormals&, int, float[3]) { return 0; }
// object_of for the PBR table: kind (with its flag bit) and p as above; a, r, m written where the object is of kind 3 and left alone
// elsewhere.  __host__ __device__: matpbr_path_object_lookup_host runs it.
__host__ __device__ inline int object_lookup(const ObjTable& ot, const MatpbrPathObjectPbr* pbr, int id, float p[3], float a[3], float& r, float& m) {
    int kind = 0;
    object_match(ot, id, [&](int k, const MatpbrPathObject& ob) {
        kind = ob.kind;
        p[0] = ob.p[0]; p[1] = ob.p[1]; p[2] = ob.p[2];
        if ((ob.kind & ~MATPBR_PATH_OBJECT_SMOOTH) == MATPBR_PATH_BSDF_PBR) {
            a[0] = pbr[k].a[0]; a[1] = pbr[k].a[1]; a[2] = pbr[k].a[2];
            r = pbr[k].r;
            m = pbr[k].m;
        }
    });
    return kind;
}
// index of the object whose range holds triangle `id`, -1: the depth mesh (the id feature needs it; __host__ __device__ for the CPU
// entry point)
__host__ __device__ inline int object_index(const ObjTable& ot, int id) {
    int idx = -1;
    object_match(ot, id, [&](int k, const MatpbrPathObject&) { idx = k; });
    return idx;
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
// ---- vertex-coloured inserted objects ("Vertex-coloured inserted objects") -------------------------------------
// c = clamp(c0 + u (c1 - c0) + v (c2 - c0), 0, 1) per channel for the corner colours cc = (c0, c1, c2) and tri_uv's u, v.  Differences
// and explicit fmaf, so that three equal corners give exactly their colour and the CPU and the device give the same bits for the same
// u, v; the clamp takes the rounding of u, v at an edge (and a u, v that is not a number, which gives 0).
__host__ __device__ inline void object_color(const float cc[9], float u, float v, float c[3]) {
    for (int k = 0; k < 3; ++k) c[k] = fminf(fmaxf(fmaf(v, cc[6 + k] - cc[k], fmaf(u, cc[3 + k] - cc[k], cc[k])), 0.0f), 1.0f);
}
// tri_uv without contraction (tri_test_strict's operations): the colour guide's, the same bits on the device and on the CPU
__host__ __device__ inline void tri_uv_strict(const float v0[3], const float e1[3], const float e2[3], const float o[3], const float d[3], float& u,
                                              float& v) {
#pragma clang fp contract(off)
    float pv[3], qv[3];
    cross3s(d, e2, pv);
    const float idet = 1.0f / dot3s(e1, pv);
    const float tv[3] = {o[0] - v0[0], o[1] - v0[1], o[2] - v0[2]};
    u = dot3s(tv, pv) * idet;
    cross3s(tv, e1, qv);
    v = dot3s(d, qv) * idet;
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

// ---- rough dielectric objects ("Rough dielectric objects"): Walter et al. 2007 with GGX, visible normals ---
// p = (int_ior, ext_ior, alpha).  The surface shades from both sides: n is the outward normal the BSDF shades with (the face normal,
// or the interpolated one after its three fallbacks), N = sign(n . wo) n the same normal on the viewer's side, eta_it = eta entering,
// 1 / eta leaving.  A direction w with (ng . w)(n . w) <= 0 carries nothing, in the sample and in the evaluation alike.  Plain
// divisions and sqrtf: the CPU entry points run what the kernel runs.
__host__ __device__ inline void rough_side(const float p[3], const float ng[3], const float ns_in[3], const float wo[3], float n[3], float N[3],
                                           float& eta_it, float& cos_o) {
    for (int c = 0; c < 3; ++c) n[c] = ns_in[c];
    smooth_side(ng, wo, n);
    const float no = dot3h(n, wo), eta = p[0] / p[1];
    const float s = no > 0.0f ? 1.0f : -1.0f;
    for (int c = 0; c < 3; ++c) N[c] = s * n[c];
    eta_it = no > 0.0f ? eta : 1.0f / eta;
    cos_o = fabsf(no);
}
// GGX about N at the half vector h (h . N > 0), 1 - NoH^2 from N x h (ggx_den_stable's form: the literal one loses its digits on the peak)
__host__ __device__ inline float rough_d(float alpha, const float N[3], const float h[3]) {
    float cr[3];
    cross3(N, h, cr);
    const float a2 = alpha * alpha, den = a2 + dot3h(cr, cr) * (1.0f - a2);
    return a2 * 0.31830988618379067154f / (den * den);
}
// Smith's G1 of the separable form: vn = v . N, vh = v . h; 0 where the two disagree about v's side
__host__ __device__ inline float rough_g1(float alpha, float vn, float vh) {
    if (!(vn * vh > 0.0f)) return 0.0f;
    const float c2 = vn * vn, t2 = fmaxf(1.0f - c2, 0.0f) / c2;
    return 2.0f / (1.0f + sqrtf(1.0f + (alpha * alpha) * t2));
}
// 1 - F of fresnel_dielectric(ci, eta_it, ct) in the form that does not cancel near total internal reflection:
// 1 - a_s^2 = 4 eta ci ct / (ci + eta ct)^2 and 1 - a_p^2 = 4 eta ci ct / (ct + eta ci)^2
__host__ __device__ inline float rough_transmittance(float ci, float eta_it, float ct) {
    const float a = ci + eta_it * ct, b = ct + eta_it * ci;
    return ct > 0.0f ? 2.0f * eta_it * ci * ct * (1.0f / (a * a) + 1.0f / (b * b)) : 0.0f;
}
// BSDF sample at a rough dielectric vertex; u_lobe, u0, u1 = dims 6, 7, 8.  h from the visible normals of wo (Heitz 2018), then
// u_lobe <= F reflects about h (weight G1(wi)), else refracts by Snell about h (weight G1(wi) eta_ti^2, kFlagTransmitted).  pdf is
// the solid-angle density of wi; the vertex is never delta.  weight 0: the path ends.
__host__ __device__ inline void rough_sample(const float p[3], const float ng[3], const float ns_in[3], const float wo[3], float u_lobe, float u0,
                                             float u1, float wi[3], float w[3], float& pdf, int& flags) {
    float n[3], N[3], eta_it, cos_o;
    rough_side(p, ng, ns_in, wo, n, N, eta_it, cos_o);
    const float alpha = p[2], eta_ti = 1.0f / eta_it;
    wi[0] = wi[1] = wi[2] = 0.0f;
    w[0] = w[1] = w[2] = 0.0f;
    pdf = 0.0f;
    flags = 0;
    if (!(cos_o > 0.0f)) return;
    // the frame of Duff et al. 2017 about N, wo in it
    const float sg = copysignf(1.0f, N[2]), a = -1.0f / (sg + N[2]), b = N[0] * N[1] * a;
    const float S[3] = {1.0f + sg * N[0] * N[0] * a, sg * b, -sg * N[0]}, T[3] = {b, sg + N[1] * N[1] * a, -N[1]};
    // the visible normals: the hemisphere configuration, a disk sample warped onto its projected area, back to the ellipsoid
    float V[3] = {alpha * dot3h(S, wo), alpha * dot3h(T, wo), cos_o};
    {
        const float il = 1.0f / sqrtf(dot3h(V, V));
        for (int c = 0; c < 3; ++c) V[c] *= il;
    }
    const float lensq = V[0] * V[0] + V[1] * V[1];
    const float il1 = lensq > 0.0f ? 1.0f / sqrtf(lensq) : 0.0f;
    const float T1[3] = {lensq > 0.0f ? -V[1] * il1 : 1.0f, lensq > 0.0f ? V[0] * il1 : 0.0f, 0.0f};
    const float T2[3] = {-V[2] * T1[1], V[2] * T1[0], V[0] * T1[1] - V[1] * T1[0]};
    const float r = sqrtf(fmaxf(u0, 0.0f)), ph = 6.28318530717958647692f * u1;
    const float t1 = r * cosf(ph), sm = 0.5f * (1.0f + V[2]);
    const float t2 = (1.0f - sm) * sqrtf(fmaxf(1.0f - t1 * t1, 0.0f)) + sm * (r * sinf(ph));
    const float t3 = sqrtf(fmaxf(1.0f - t1 * t1 - t2 * t2, 0.0f));
    float m[3] = {alpha * (t1 * T1[0] + t2 * T2[0] + t3 * V[0]), alpha * (t1 * T1[1] + t2 * T2[1] + t3 * V[1]), fmaxf(t2 * T2[2] + t3 * V[2], 0.0f)};
    const float ml2 = dot3h(m, m);
    if (!(ml2 > 0.0f)) return;
    const float ilm = 1.0f / sqrtf(ml2);
    float h[3];
    for (int c = 0; c < 3; ++c) h[c] = (m[0] * S[c] + m[1] * T[c] + m[2] * N[c]) * ilm;
    const float woh = dot3h(wo, h);
    if (!(woh > 0.0f)) return;
    float ct;
    const float F = fresnel_dielectric(woh, eta_it, ct);
    const float Dv = rough_g1(alpha, cos_o, woh) * woh * rough_d(alpha, N, h) / cos_o;
    float win, wih;
    if (u_lobe <= F) {
        for (int c = 0; c < 3; ++c) wi[c] = 2.0f * woh * h[c] - wo[c];
        win = dot3h(wi, N);
        wih = dot3h(wi, h);
        pdf = F * Dv / (4.0f * woh);
        w[0] = win > 0.0f ? rough_g1(alpha, win, wih) : 0.0f;
    } else {
        const float k = eta_ti * woh - ct;
        for (int c = 0; c < 3; ++c) wi[c] = k * h[c] - eta_ti * wo[c];
        win = dot3h(wi, N);
        wih = dot3h(wi, h);
        const float q = woh + eta_it * wih;
        pdf = rough_transmittance(woh, eta_it, ct) * Dv * (eta_it * eta_it) * fabsf(wih) / (q * q);
        w[0] = win < 0.0f ? rough_g1(alpha, win, wih) * (eta_ti * eta_ti) : 0.0f;
        flags = kFlagTransmitted;
    }
    if (!(dot3h(ng, wi) * dot3h(n, wi) > 0.0f) || !(pdf > 0.0f)) w[0] = 0.0f;   // the two normals disagree about wi's side
    w[1] = w[2] = w[0];
}
// The BSDF's value for the direction wl (with its cosine) and the density rough_sample gives wl: f / pdf is its weight.
__host__ __device__ inline void rough_eval(const float p[3], const float ng[3], const float ns_in[3], const float wo[3], const float wl[3], float& f,
                                           float& pdf) {
    float n[3], N[3], eta_it, cos_o;
    rough_side(p, ng, ns_in, wo, n, N, eta_it, cos_o);
    const float alpha = p[2];
    f = 0.0f;
    pdf = 0.0f;
    const float cos_l = dot3h(wl, N);
    if (!(cos_o > 0.0f) || !(dot3h(ng, wl) * dot3h(n, wl) > 0.0f)) return;
    const bool reflect = cos_l > 0.0f;
    const float kl = reflect ? 1.0f : eta_it;
    float h[3] = {wo[0] + kl * wl[0], wo[1] + kl * wl[1], wo[2] + kl * wl[2]};
    const float l2 = dot3h(h, h);
    if (!(l2 > 0.0f)) return;
    const float il = (dot3h(h, N) > 0.0f ? 1.0f : -1.0f) / sqrtf(l2);
    for (int c = 0; c < 3; ++c) h[c] *= il;
    const float woh = dot3h(wo, h), wlh = dot3h(wl, h);
    if (!(woh > 0.0f) || (!reflect && !(wlh < 0.0f))) return;   // a refraction leaves on the far side of the microfacet
    float ct;
    const float F = fresnel_dielectric(woh, eta_it, ct);
    const float D = rough_d(alpha, N, h), G1o = rough_g1(alpha, cos_o, woh), G1l = rough_g1(alpha, cos_l, wlh);
    const float Dv = G1o * woh * D / cos_o;
    if (reflect) {
        f = F * D * (G1o * G1l) / (4.0f * cos_o);
        pdf = F * Dv / (4.0f * woh);
    } else {
        const float q = woh + eta_it * wlh;
        const float Tr = rough_transmittance(woh, eta_it, ct);
        f = Tr * D * (G1o * G1l) * (woh * fabsf(wlh)) / (cos_o * (q * q));
        pdf = Tr * Dv * (eta_it * eta_it) * fabsf(wlh) / (q * q);
    }
    if (!(pdf > 0.0f)) { f = 0.0f; pdf = 0.0f; }
}

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
// a rough dielectric's p: both indices finite and > 0, their ratio and its inverse finite fp32 numbers at least 0.01 away from 1,
// alpha in [0.02, 1]
bool rough_valid(const float p[3]) {
    if (!(p[0] > 0.0f && p[1] > 0.0f && std::isfinite(p[0]) && std::isfinite(p[1]))) return false;
    const float eta = p[0] / p[1];
    return eta > 0.0f && std::isfinite(eta) && std::isfinite(1.0f / eta) && fabsf(eta - 1.0f) >= 0.01f && p[2] >= 0.02f && p[2] <= 1.0f;
}
// What a table may hold besides the plain kinds 1 and 2, as object_table's accept mask: kAcceptSmooth a kind that carries
// MATPBR_PATH_OBJECT_SMOOTH; kAcceptPbr kind MATPBR_PATH_BSDF_PBR (its p[] is ignored; its record is checked where `pbr` is given);
// kAcceptLight kind MATPBR_PATH_BSDF_AREA (never with the smooth flag; p = radiance, finite and >= 0); kAcceptRough kind
// MATPBR_PATH_BSDF_ROUGH_DIELECTRIC (rough_valid); kAcceptColor a kind 2 or 3 that carries MATPBR_PATH_OBJECT_COLORED (on another kind
// the flag is refused); kAcceptTexture the same for MATPBR_PATH_OBJECT_TEXTURED (its record is path_textures.hpp's to check); kAcceptMedium
// a kind 1 or 5 that carries MATPBR_PATH_OBJECT_MEDIUM (on another kind the flag is refused; its record is path_media.hpp's to check);
// kAcceptPhoto a kind 2, 3 or 5 that carries MATPBR_PATH_OBJECT_PHOTO (on another kind the flag is refused).
// A kind outside the mask is an unknown kind.  kAcceptAll is what the entries before the colour flag admit.
enum : unsigned { kAcceptSmooth = 1u, kAcceptPbr = 2u, kAcceptLight = 4u, kAcceptRough = 8u, kAcceptAll = 15u, kAcceptColor = 16u, kAcceptTexture = 32u,
                  kAcceptMedium = 64u, kAcceptPhoto = 128u };
// how many objects of a checked table are smooth, of kind 3, of kind 4, of kind 5, coloured, textured, filled with a medium, flagged to
// keep the see-through chain
struct ObjCounts {
    int smooth = 0, pbr = 0, light = 0, rough = 0, color = 0, tex = 0, medium = 0, photo = 0;
};
bool object_table(const MatpbrPathObject* objects, int n_objects, unsigned accept, const MatpbrPathObjectPbr* pbr, ObjTable& ot,
                  ObjCounts* counts = nullptr) {
    if (n_objects < 0 || n_objects > MATPBR_PATH_MAX_OBJECTS || (n_objects > 0 && !objects)) return false;
    ot.n = n_objects;
    ot.min_id = INT32_MAX;
    ObjCounts c;
    for (int k = 0; k < n_objects; ++k) {
        MatpbrPathObject plain = objects[k];
        bool range_alone = false;   // kinds 3, 4, 5 are checked as a diffuse object of reflectance 0: the range alone
        if ((accept & kAcceptPhoto) && (plain.kind & MATPBR_PATH_OBJECT_PHOTO)) {
            const int base = plain.kind & ~(MATPBR_PATH_OBJECT_PHOTO | MATPBR_PATH_OBJECT_MEDIUM | MATPBR_PATH_OBJECT_TEXTURED | MATPBR_PATH_OBJECT_COLORED |
                                            MATPBR_PATH_OBJECT_SMOOTH);
            if (base != MATPBR_PATH_BSDF_DIFFUSE && base != MATPBR_PATH_BSDF_PBR && base != MATPBR_PATH_BSDF_ROUGH_DIELECTRIC) return false;
            plain.kind &= ~MATPBR_PATH_OBJECT_PHOTO;
            ++c.photo;
        }
        if ((accept & kAcceptTexture) && (plain.kind & MATPBR_PATH_OBJECT_TEXTURED)) {
            const int base = plain.kind & ~(MATPBR_PATH_OBJECT_TEXTURED | MATPBR_PATH_OBJECT_COLORED | MATPBR_PATH_OBJECT_SMOOTH);
            if (base != MATPBR_PATH_BSDF_DIFFUSE && base != MATPBR_PATH_BSDF_PBR) return false;
            plain.kind &= ~MATPBR_PATH_OBJECT_TEXTURED;
            ++c.tex;
        }
        if ((accept & kAcceptColor) && (plain.kind & MATPBR_PATH_OBJECT_COLORED)) {
            const int base = plain.kind & ~(MATPBR_PATH_OBJECT_COLORED | MATPBR_PATH_OBJECT_SMOOTH);
            if (base != MATPBR_PATH_BSDF_DIFFUSE && base != MATPBR_PATH_BSDF_PBR) return false;
            plain.kind &= ~MATPBR_PATH_OBJECT_COLORED;
            ++c.color;
        }
        if ((accept & kAcceptMedium) && (plain.kind & MATPBR_PATH_OBJECT_MEDIUM)) {
            const int base = plain.kind & ~(MATPBR_PATH_OBJECT_MEDIUM | MATPBR_PATH_OBJECT_SMOOTH);
            if (base != MATPBR_PATH_BSDF_DIELECTRIC && base != MATPBR_PATH_BSDF_ROUGH_DIELECTRIC) return false;
            plain.kind &= ~MATPBR_PATH_OBJECT_MEDIUM;
            ++c.medium;
        }
        if ((accept & kAcceptLight) && plain.kind == MATPBR_PATH_BSDF_AREA) {
            for (int j = 0; j < 3; ++j)
                if (!(plain.p[j] >= 0.0f) || !std::isfinite(plain.p[j])) return false;
            range_alone = true;
            ++c.light;
        }
        if ((accept & kAcceptSmooth) && (plain.kind & MATPBR_PATH_OBJECT_SMOOTH)) {
            plain.kind &= ~MATPBR_PATH_OBJECT_SMOOTH;
            ++c.smooth;
        }
        if ((accept & kAcceptRough) && plain.kind == MATPBR_PATH_BSDF_ROUGH_DIELECTRIC) {
            if (!rough_valid(plain.p)) return false;
            range_alone = true;
            ++c.rough;
        }
        if ((accept & kAcceptPbr) && plain.kind == MATPBR_PATH_BSDF_PBR) {
            if (pbr && !pbr_valid(pbr[k])) return false;
            range_alone = true;
            ++c.pbr;
        }
        if (range_alone) {
            plain.kind = MATPBR_PATH_BSDF_DIFFUSE;
            plain.p[0] = plain.p[1] = plain.p[2] = 0.0f;
        }
        if (!object_valid(plain)) return false;
        for (int j = 0; j < k; ++j)   // ranges may not overlap
            if (objects[k].first_tri < objects[j].first_tri + objects[j].n_tri && objects[j].first_tri < objects[k].first_tri + objects[k].n_tri)
                return false;
        ot.o[k] = objects[k];
        ot.min_id = std::min(ot.min_id, objects[k].first_tri);
    }
    if (counts) *counts = c;
    return true;
}
bool trans_edit_valid(const MatpbrPathTransEdit* e) {
    return e && e->ior > 0.0f && std::isfinite(e->ior) && e->spec_trans >= 0.0f && e->spec_trans <= 1.0f && e->refract_distance >= 0.0f &&
           std::isfinite(e->refract_distance);
}
}  // namespace
