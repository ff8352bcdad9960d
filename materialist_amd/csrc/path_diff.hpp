// path_diff.hpp -- the differential render of libmatpbr_path.so (matpbr_path.hip includes it; DESIGN.md section 1.4, "Differential
// render"): the table of path_kernel<DiffObjects> and the composite into the photograph.
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
inline bool composite_args_valid(const float* fg, const float* delta, const float* alpha, const float* photo, int H, int W, float scale,
                                 const float* out) {
    return fg && delta && alpha && photo && out && H > 0 && W > 0 && std::isfinite(scale) && scale > 0.0f;
}
}  // namespace
