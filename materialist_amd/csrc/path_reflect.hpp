// path_reflect.hpp -- the photograph reflected in inserted objects (matpbr_path.hip includes it; DESIGN.md section 1.4, "Reflected in
// inserted objects"): the tables of the four see-through shapes whose chain passes objects that carry MATPBR_PATH_OBJECT_PHOTO, and the
// trait the kernel reads them by.
#pragma once
#include "path_media.hpp"

namespace {
// a see-through table (ThroughObjects, RatioThroughObjects, MediumDiff<> of either) some of whose objects carry the flag: the same
// members, another type, so that the four shapes without the flag stay the code they are
template <class Through>
struct Reflect : Through {};
// what path_kernel reads off its table's type: a vertex on a flagged object keeps the camera chain alive.  False for every other table.
template <class Objects> struct ReflectTraits { static constexpr bool reflect = false; };
template <class Through> struct ReflectTraits<Reflect<Through>> { static constexpr bool reflect = true; };
template <class Through> struct DiffTraits<Reflect<Through>> : DiffTraits<Through> {};
template <class Through> struct MediumTraits<Reflect<Through>> : MediumTraits<Through> {};

// path_sample for the CPU twin of the chain (matpbr_path_reflect_chain_host) at a vertex of kind 3.  matpbr_device.hpp's functions are
// device code (hardware reciprocals, square roots and sincosf), so the CPU restates frame, to_world, path_sample_st, path_lane and
// brdf_core with plain divisions, sqrtf, sinf and cosf, operation for operation otherwise, as cosine_grads_host does for the normal's
// gradient.  -> wi, weight = f / (pdf + 1e-6) where pdf > 1e-6 else 0, pdf.
inline void path_sample_host(float sample1, float u0, float u1, const float wo[3], const float n[3], const float a[3], float r, float m, float wi[3],
                             float w[3], float& pdf_out) {
    const float kPiF = 3.14159265358979323846f, kInvPiF = 0.31830988618379067154f;
    const float sign = n[2] >= 0.0f ? 1.0f : -1.0f, fa = -1.0f / (sign + n[2]), fb = n[0] * n[1] * fa;
    const float s[3] = {fmaf(sign * n[0] * n[0], fa, 1.0f), sign * fb, -sign * n[0]}, t[3] = {fb, fmaf(n[1] * n[1], fa, sign), -n[1]};
    const float sp = sinf(2.0f * kPiF * u1), cp = cosf(2.0f * kPiF * u1);
    const float alpha2 = (r * r) * (r * r), am1 = alpha2 - 1.0f;
    float sin2_h = -1.0f, cos_h = 0.0f;
    if (sample1 > 0.5f) {
        const float st = sqrtf(fmaxf(u0, 0.0f)), ct = sqrtf(fmaxf(1.0f - u0, 0.0f));
        for (int c = 0; c < 3; ++c) wi[c] = fmaf(n[c], ct, fmaf(t[c], st * sp, s[c] * (st * cp)));
    } else {
        const float q = 1.0f / fmaf(u0, am1, 1.0f);
        const float ct = sqrtf(fmaxf((1.0f - u0) * q, 0.0f)), st = sqrtf(fmaxf(u0 * alpha2 * q, 0.0f));
        float wh[3];
        for (int c = 0; c < 3; ++c) wh[c] = fmaf(n[c], ct, fmaf(t[c], st * sp, s[c] * (st * cp)));
        const float d = 2.0f * fmaf(wo[2], wh[2], fmaf(wo[1], wh[1], wo[0] * wh[0]));
        for (int c = 0; c < 3; ++c) wi[c] = fmaf(d, wh[c], -wo[c]);
        const float il = 1.0f / sqrtf(fmaf(wi[2], wi[2], fmaf(wi[1], wi[1], wi[0] * wi[0])));
        for (int c = 0; c < 3; ++c) wi[c] *= il;
        if (d > 0.0f) { sin2_h = u0 * alpha2 * q; cos_h = ct; }
    }
    auto dot = [](const float* x, const float* y) { return fmaf(x[2], y[2], fmaf(x[1], y[1], x[0] * y[0])); };
    float h[3] = {wi[0] + wo[0], wi[1] + wo[1], wi[2] + wo[2]};
    const float ilh = 1.0f / sqrtf(dot(h, h));
    for (int c = 0; c < 3; ++c) h[c] *= ilh;
    const float NoV = fmaxf(dot(n, wo), 0.0f), NoL = fmaxf(dot(n, wi), 0.0f), VoH = fmaxf(dot(wo, h), 0.0f), nh_raw = dot(n, h);
    float NoH = fmaxf(nh_raw, 0.0f), den;
    if (sin2_h >= 0.0f) {
        NoH = cos_h;
        den = fmaf(sin2_h, -am1, alpha2) + 1e-6f;
    } else if (fabsf(dot(n, n) - 1.0f) < 1e-5f && nh_raw > 0.0f) {
        const float cx = n[1] * h[2] - n[2] * h[1], cy = n[2] * h[0] - n[0] * h[2], cz = n[0] * h[1] - n[1] * h[0];
        den = fmaf(fmaf(cx, cx, fmaf(cy, cy, cz * cz)), -am1, alpha2) + 1e-6f;
    } else {
        den = fmaf(NoH * NoH, am1, 1.0f) + 1e-6f;
    }
    const float iden = 1.0f / den, D = (alpha2 * kInvPiF) * (iden * iden);
    const float p = fmaf(0.125f * (D * NoH), 1.0f / fmaxf(VoH, 1e-6f), (0.5f * kInvPiF) * NoL);
    const float FDm1 = fmaf((2.0f * r) * VoH, VoH, -0.5f);
    auto pow5 = [](float x) { const float x2 = x * x; return x2 * x2 * x; };
    const float Fi = fmaf(FDm1, pow5(1.0f - NoL), 1.0f), Fo = fmaf(FDm1, pow5(1.0f - NoV), 1.0f);
    const float rp1 = r + 1.0f, k = (rp1 * rp1) * 0.125f, omk = 1.0f - k, kpe = k + 1e-6f;
    const float G = (1.0f / fmaf(NoL, omk, kpe)) * (1.0f / fmaf(NoV, omk, kpe));
    const float x5 = pow5(1.0f - VoH), dsc = Fo * Fi * NoL, ssc = 0.25f * (D * G) * NoL;
    const float ip = p > 1e-6f ? 1.0f / (p + 1e-6f) : 0.0f, omm = 1.0f - m;
    for (int c = 0; c < 3; ++c) {
        const float C0 = fmaf(m, a[c], omm * 0.04f);
        w[c] = fmaf(ssc, fmaf(x5, 1.0f - C0, C0), ((a[c] * omm) * kInvPiF) * dsc) * ip;
    }
    pdf_out = p > 0.0f ? p : 0.0f;
}
}  // namespace
