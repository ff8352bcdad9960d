// path_diff.hpp -- the differential render of libmatpbr_path.so (matpbr_path.hip includes it; DESIGN.md section 1.4, "Differential
// render"): the tables of path_kernel<DiffObjects> and its kin, the traits the kernel reads them by, and the composites into the
// photograph.
#pragma once
#include "path_textures.hpp"

namespace {
// TexObjects (every object rule is on) and the sums the kernel keeps per pixel.  A sample is walked in the merged scene; where that
// walk met an inserted triangle and the camera ray did not land on one, it is walked again with every triangle of id >= n_scene_tri
// skipped and the envmap as the only emitter.  fg: radiance of the samples whose camera ray lands on an object; alpha: their share;
// delta: radiance with minus radiance without the objects of the other samples that were walked twice.
struct DiffObjects : TexObjects {
    float* fg;            // [H,W,3]
    float* delta;         // [H,W,3]
    float* alpha;         // [H,W]
    uint32_t* rewalked;   // [H,W], nullable: second walks per pixel, added to
};
// DiffObjects with the photograph behind inserted glass ("Seen through glass").  A sample whose camera ray
// lands on an object and leaves it through dielectric vertices alone lands on the depth mesh's front at depth k: there it adds
// thr_k photo[screen_texel(p)] to `through`, and, where its walk met an inserted triangle after that landing (or the table holds a
// light) and k + 1 < max_depth, it is walked again with the inserted triangles skipped from depth k on and the envmap as the only
// emitter; fg then takes the difference of the two walks.
struct ThroughObjects : DiffObjects {
    const float* photo;   // [H,W,3], finite and >= 0
    float* through;       // [H,W,3]
};
// Either table with one more sum ("Ratio shadow transfer"): base = (1 - c_s) L_without,s, the radiance without
// the objects of every sample whose camera ray misses them: the second walk's where there was one, else the first's, which met no
// object and so is the same arithmetic.  The other sums are computed as they are without it.
struct RatioObjects : DiffObjects {
    float* base;          // [H,W,3]
};
struct RatioThroughObjects : ThroughObjects {
    float* base;          // [H,W,3]
};
// what path_kernel reads off its table's type: `diff`: the table carries the differential render's sums and a sample takes up to two
// trips; `through`: it carries the photograph as well; `base`: and the ratio's sum.  All false for every other table.
template <class Objects> struct DiffTraits { static constexpr bool diff = false, through = false, base = false; };
template <> struct DiffTraits<DiffObjects> { static constexpr bool diff = true, through = false, base = false; };
template <> struct DiffTraits<ThroughObjects> { static constexpr bool diff = true, through = true, base = false; };
template <> struct DiffTraits<RatioObjects> { static constexpr bool diff = true, through = false, base = true; };
template <> struct DiffTraits<RatioThroughObjects> { static constexpr bool diff = true, through = true, base = true; };

// out = max(0, (fg + delta) scale + (1 - alpha scale) photo) of one channel: every product and sum rounded on its own, so the device
// and the CPU give the same bits
__host__ __device__ inline float composite_value(float fg, float delta, float alpha, float photo, float scale) {
#pragma clang fp contract(off)
    const float d = (fg + delta) * scale;
    const float keep = 1.0f - alpha * scale;
    const float bg = keep * photo;
    return fmaxf(0.0f, d + bg);
}
__host__ __device__ inline void composite_pixel(const float* fg, const float* delta, const float* alpha, const float* photo, long p, float scale,
                                                float* out) {
    const float al = alpha[p];
    for (int c = 0; c < 3; ++c) out[3 * p + c] = composite_value(fg[3 * p + c], delta[3 * p + c], al, photo[3 * p + c], scale);
}
__global__ __launch_bounds__(256) void composite_kernel(const float* fg, const float* delta, const float* alpha, const float* photo, long P,
                                                        float scale, float* out) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p < P) composite_pixel(fg, delta, alpha, photo, p, scale, out);
}
// The composite with the shadows transferred as a ratio ("Ratio shadow transfer"), one channel.  Where the
// objects darken it (delta < 0 < base) the photograph behind the objects is multiplied by g = max(0, B + D) / B in [0, 1], B = base
// scale, D = delta scale: the model's albedo cancels and the result cannot go below fg.  Elsewhere it is composite_value, statement
// for statement: light the scene did not have is additive, and its ratio has no bound where the model's base is dark.  Every
// operation is rounded on its own and the division is the correctly rounded one on both sides.
__host__ __device__ inline float composite_ratio_value(float fg, float delta, float base, float alpha, float photo, float scale) {
#pragma clang fp contract(off)
    if (delta < 0.0f && base > 0.0f) {
        const float B = base * scale;
        const float D = delta * scale;
        const float g = fmaxf(0.0f, B + D) / B;
        const float keep = 1.0f - alpha * scale;
        const float bg = keep * photo;
        const float f = fg * scale;
        return fmaxf(0.0f, f + bg * g);
    }
    return composite_value(fg, delta, alpha, photo, scale);
}
__host__ __device__ inline void composite_ratio_pixel(const float* fg, const float* delta, const float* base, const float* alpha, const float* photo,
                                                      long p, float scale, float* out) {
    const float al = alpha[p];
    for (int c = 0; c < 3; ++c)
        out[3 * p + c] = composite_ratio_value(fg[3 * p + c], delta[3 * p + c], base[3 * p + c], al, photo[3 * p + c], scale);
}
__global__ __launch_bounds__(256) void composite_ratio_kernel(const float* fg, const float* delta, const float* base, const float* alpha,
                                                              const float* photo, long P, float scale, float* out) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p < P) composite_ratio_pixel(fg, delta, base, alpha, photo, p, scale, out);
}
inline bool composite_args_valid(const float* fg, const float* delta, const float* alpha, const float* photo, int H, int W, float scale,
                                 const float* out) {
    return fg && delta && alpha && photo && out && H > 0 && W > 0 && std::isfinite(scale) && scale > 0.0f;
}
}  // namespace
