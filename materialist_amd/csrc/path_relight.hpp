// path_relight.hpp -- relighting in the photograph (matpbr_path.hip includes it; DESIGN.md section 1.4, "Relighting in the
// photograph"): the table of the path_kernel whose one walk carries the radiance under two environments, the trait the kernel reads
// it by, and the quotient composite into the photograph.
#pragma once
#include "path_mapedit.hpp"

namespace {
// `Base` (NoObjects, or ShadeNormals with its map) and a second environment beside the one of PathArgs, with its own size and tables.
// No decision of the walk over the depth mesh reads the envmap, so one walk serves both: the closest hits, the texels and the BSDF
// samples are computed once, and at every vertex the emitter sample (the same dims 2-5, its own shadow ray) and at an escape the lookup
// run once per environment.  The radiance under PathArgs' environment goes to PathArgs' `out`, which the entry point sets to `base`;
// the radiance under this one to `relit`.  Both sums, the launch split and the final division are the render's own.
template <class Base>
struct Relight : Base {
    const float *env_b, *row_cdf_b, *col_cdf_b, *env_pdf_b;   // [He_b,We_b,3], [He_b+1], [He_b,We_b+1], [He_b,We_b]
    int He_b, We_b;
    float* relit;   // [H,W,3]
};
// what path_kernel reads off its table's type: the table carries a second environment and a sample carries two radiances.  False for
// every other table.
template <class Objects> struct RelightTraits { static constexpr bool relight = false; };
template <class Base> struct RelightTraits<Relight<Base>> { static constexpr bool relight = true; };

// The quotient image, one channel: the photograph times the model's radiance under the new light over its radiance under the fitted
// one, B0 = base scale, B1 = relit scale, g = (B1 + floor) / (B0 + floor), out = max(0, photo g).  The fit's albedo cancels in g to
// first order; floor > 0 bounds it where the model is dark, g <= (B1 + floor) / floor.  Every operation is rounded on its own and the
// division is the correctly rounded one on both sides, so the device and the CPU give the same bits; where relit has base's bits g is
// exactly 1 and the photograph comes through bit for bit.
__host__ __device__ inline float composite_relight_value(float base, float relit, float photo, float scale, float floor) {
#pragma clang fp contract(off)
    const float B0 = base * scale;
    const float B1 = relit * scale;
    const float g = (B1 + floor) / (B0 + floor);
    return fmaxf(0.0f, photo * g);
}
__host__ __device__ inline void composite_relight_pixel(const float* base, const float* relit, const float* photo, long p, float scale, float floor,
                                                        float* out) {
    for (int c = 0; c < 3; ++c) out[3 * p + c] = composite_relight_value(base[3 * p + c], relit[3 * p + c], photo[3 * p + c], scale, floor);
}
__global__ __launch_bounds__(256) void composite_relight_kernel(const float* base, const float* relit, const float* photo, long P, float scale,
                                                                float floor, float* out) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p < P) composite_relight_pixel(base, relit, photo, p, scale, floor, out);
}
inline bool composite_relight_args_valid(const float* base, const float* relit, const float* photo, int H, int W, float scale, float floor,
                                         const float* out) {
    return base && relit && photo && out && H > 0 && W > 0 && std::isfinite(scale) && scale > 0.0f && std::isfinite(floor) && floor > 0.0f;
}
}  // namespace
