// matpbr_path.hip -- libmatpbr_path.so: the path-traced re-render of the depth mesh (include/matpbr_path.h).
//
//   * host: a binned-SAH BVH2 over the mesh's triangles (every node holds both children's boxes, so one 64-byte node read tests
//     two boxes), triangles stored in leaf order as precomputed (v0, e1, e2); the envmap's importance-sampling tables (fp64 -> fp32);
//   * device: one thread per pixel loops over its samples in order and accumulates them in a fixed order (no atomics: the image is
//     bit-reproducible, and so is every split of a frame into launches); the traversal stack lives in LDS, one column per lane;
//   * the closest-hit routine and the emitter sampler are __host__ __device__: the CPU entry points run the same code as the kernel;
//   * backward (matpbr_path_render_bwd): path replay with the sampling detached, 64-bit fixed-point sums (see "backward pass" below).
// The BRDF arithmetic is matpbr_device.hpp's (pixel_const, brdf_core, ggx_den_stable, frame, to_world), unchanged.
// One translation unit: this file holds PathArgs, the forward kernel, the backward kernels and the C ABI; path_bvh.hpp the BVH, its
// traversals and the host builder; path_shading.hpp the RNG, the envmap sampler and the BSDF wrappers; path_objects.hpp the tables the
// kernels take by value, their lookups, samplers and checks; path_lights.hpp the emissive objects' tables, sampler and pdfs;
// path_textures.hpp the image textures of inserted objects; path_denoise.hpp the denoiser; path_diff.hpp the differential render's table
// and the composite; path_media.hpp the media inside glass objects; path_move.hpp the grafted BVH's move and refit of the inserted objects;
// path_reflect.hpp the see-through tables whose chain passes flagged objects; path_mapedit.hpp the table of the walk over edited maps;
// path_relight.hpp the table of the walk under two environments and the quotient composite.
#include <type_traits>

#include "path_denoise.hpp"
#include "path_diff.hpp"
#include "path_mapedit.hpp"
#include "path_media.hpp"
#include "path_move.hpp"
#include "path_reflect.hpp"
#include "path_relight.hpp"

namespace {

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
__host__ __device__ __forceinline__ float spawn_eps(const float p[3]) { return 1e-5f * (1.0f + fmaxf(fmaxf(fabsf(p[0]), fabsf(p[1])), fabsf(p[2]))); }

// (DiffObjects) the id from which the traversals skip triangles: none in a sample's first trip, the inserted ones in its second
template <class Objects> __device__ __forceinline__ int id_limit_of(const Objects&, bool) { return 0; }
__device__ __forceinline__ int id_limit_of(const DiffObjects& ot, bool second) { return second ? ot.n_scene_tri : INT32_MAX; }
__device__ __forceinline__ int id_limit_of(const RatioObjects& ot, bool second) { return id_limit_of(static_cast<const DiffObjects&>(ot), second); }
template <class Diff> __device__ __forceinline__ int id_limit_of(const MediumDiff<Diff>& ot, bool second) {
    return id_limit_of(static_cast<const DiffObjects&>(ot), second);
}
// (ThroughObjects) the second trip of a see-through sample replays its chain over every triangle and skips the inserted ones from its
// landing depth `land` on; land = -1 (not see-through) skips them from the camera ray on, DiffObjects' rule
__device__ __forceinline__ int id_limit_at(const ThroughObjects& ot, bool second, int depth, int land) {
    return second && depth >= land ? ot.n_scene_tri : INT32_MAX;
}

// samples [s0, s1) of every pixel added to out (first: start from 0; last: divide by spp).  OBJ: the BVH holds inserted objects
// (Objects = ObjTable, passed by value); EDIT: transparency editing (Objects = TransEdit, by value in the table's place).  With
// NoObjects every `if (OBJ ...)`, `if (EDIT ...)` and `if (NRM ...)` below folds away and the walk is the depth mesh's alone, the code
// the kernel had before there were objects; with ObjTable every `if (EDIT ...)` folds away.  NRM: shading normals (Objects =
// ShadeNormals): `n` stays the face normal ng and `ns` is the map's.  SMOOTH: smooth inserted objects (Objects = SmoothObjects): OBJ
// with `ns` the interpolated corner normal at the vertices of a flagged object; every `if (SMOOTH ...)` folds away in the other four.
// PBR: SMOOTH with objects of kind 3 (Objects = PbrObjects), whose vertices run the depth mesh's branch about `ns` on the constants of
// their record; every `if (PBR ...)` folds away in the other five.  LIGHT: PBR with objects of kind 4 (Objects = LightObjects), area
// lights: one emitter of n_e (the envmap, the lights) is sampled per vertex, and a ray that lands on a light adds its emission and
// ends; every `if (LIGHT ...)` folds away in the other six.  ROUGH: LIGHT with objects of kind 5 (Objects = RoughObjects), rough
// dielectrics: a non-delta vertex that shades from both sides, whose emitter sample may arrive on either side of the face and whose
// light table may be empty; every `if (ROUGH ...)` folds away in the other seven.  COLOR: ROUGH with vertex-coloured objects (Objects =
// ColorObjects): at a vertex of a flagged object of kind 2 or 3 the reflectance or the albedo is multiplied by the colour interpolated
// from the triangle's corners; every `if (COLOR ...)` folds away in the other eight.  TEX: COLOR with UV-textured objects (Objects =
// TexObjects): at a vertex of a flagged object the reflectance or the albedo is multiplied by a base-colour image, a PBR object's
// roughness and metallic by an orm image, at the coordinate interpolated from the triangle's corners; every `if (TEX ...)` folds away in
// the other nine.  DIFF: TEX as the differential render walks it (Objects = DiffObjects; DESIGN.md section 1.4, "Differential render"):
// a sample takes up to two trips through the sample loop's body, the same statements.  Trip 0 is TEX's walk; it records whether the camera
// ray landed on an inserted triangle (`cov`) and whether any trace returned one (`touched`; a light in the table touches every
// sample).  Trip 1 runs where touched && !cov: the same sample from the camera ray on, with every triangle of id >= n_scene_tri skipped
// and the envmap as the only emitter.  The sums live in the table's buffers between samples, not in registers.  Every `if (DIFF ...)`
// folds away in the other ten.  THROUGH: DIFF with the photograph behind inserted glass (Objects = ThroughObjects; DESIGN.md section 1.4,
// "Seen through glass").  Trip 0 follows the camera chain (`chain`: every vertex so far was a dielectric one); where it lands on the
// depth mesh's front at depth >= 1 it adds thr photo[texel] to `through`, records the depth in `land` and starts `touched` afresh.  Trip 1
// of such a sample runs where touched && land + 1 < max_depth: the same sample from the camera ray on, so the same chain, with the
// inserted triangles skipped from depth `land` on and the envmap as the only emitter; fg takes trip 0 minus trip 1.  Every
// `if (THROUGH ...)` folds away in the other eleven.  BASE: DIFF or THROUGH with one more sum (Objects = RatioObjects,
// RatioThroughObjects; DESIGN.md section 1.4, "Ratio shadow transfer"): a sample with cov false adds the radiance of its last trip, the
// walk without the objects, to `base`.  DIFF, THROUGH and BASE are read off the table's type (DiffTraits), so the twelve kernels
// without `base` are the code they were; every `if (BASE ...)` folds away in them.  MEDIUM: TEX or a table of the DIFF family with media
// inside glass objects (Objects = MediumObjects, MediumDiff<...>; DESIGN.md section 1.4, "Media inside glass"): the path carries `med`,
// the object whose medium the ray is in, and a segment with med >= 0 is attenuated and may end at a medium vertex.  Read off the
// table's type (MediumTraits); every `if (MEDIUM ...)` folds away in the sixteen kernels without media.  REFLECT: THROUGH whose chain also
// passes the vertices of objects that carry MATPBR_PATH_OBJECT_PHOTO (Objects = Reflect<...> of the four see-through shapes; DESIGN.md
// section 1.4, "Reflected in inserted objects").  Such a vertex is not delta: its emitter sample stays in the sample's radiance.  At the
// landing trip 0 commits the radiance gathered so far, the chain's, to fg and starts L afresh, so that Lw is the tail's as it is along
// a dielectric chain; trip 1 replays the chain without emitter samples below `land`, so that its L is the tail's as well.  Read off the
// table's type (ReflectTraits); every `if (REFLECT ...)` folds away in the twenty kernels without it.  MAPEDIT: the depth mesh's walk, or
// NRM's, over edited maps (Objects = MapEdit<NoObjects>, MapEdit<ShadeNormals>; DESIGN.md section 1.4, "Material edits in the
// photograph"), with DIFF's two trips and none of its tables.  Trip 0 reads the edited maps where the texel a vertex reads is masked and
// records the first such read in `touched`; trip 1 runs where touched: the same sample from the camera ray on, on the fitted maps
// alone.  delta takes trip 0 minus trip 1; the radiance on the fitted maps, trip 1's or the only trip's, takes the render's own sum
// (`acc`, q.out).  Nothing of trip 0 but Lw and touched reaches trip 1.  Read off the table's type (MapEditTraits); every
// `if (MAPEDIT ...)` folds away in every kernel without it.  RELIGHT: the depth mesh's walk, or NRM's, under two environments (Objects =
// Relight<NoObjects>, Relight<ShadeNormals>; DESIGN.md section 1.4, "Relighting in the photograph"): one trip per sample, as the
// render's.  No decision of that walk reads the envmap, so the closest hit, the texel, the BSDF sample, the throughput and the stop
// rules are computed once; the statements that do read it, the emitter sample at a vertex and the lookup at an escape, are the
// depth mesh's alone (no object, light or edit rule applies) and stand in blocks of their own: one body run twice (`e` = 0: PathArgs'
// environment into L; 1: the table's into L1), a loop that is not unrolled with the pointers, the sizes and the sum chosen by
// wave-uniform selects, so both environments get the same instructions and L1 has L's bits where the environments are equal.  L goes
// to the render's own sum (`acc`, q.out), L1 to a second register sum (`racc`, relit).  Read off the table's type (RelightTraits);
// every `if (RELIGHT ...)` folds away in every kernel without it, whose statements are untouched.
template <class Objects>
__global__ __launch_bounds__(kBlock) void path_kernel(const PathArgs q, int s0, int s1, int first, int last, const Objects ot) {
    constexpr bool THROUGH = DiffTraits<Objects>::through;
    constexpr bool DIFF = DiffTraits<Objects>::diff;
    constexpr bool BASE = DiffTraits<Objects>::base;
    constexpr bool MEDIUM = MediumTraits<Objects>::medium;
    constexpr bool REFLECT = ReflectTraits<Objects>::reflect;
    constexpr bool MAPEDIT = MapEditTraits<Objects>::mapedit;
    constexpr bool RELIGHT = RelightTraits<Objects>::relight;
    constexpr bool TEX = std::is_same<Objects, TexObjects>::value || DIFF || MEDIUM;
    constexpr bool COLOR = std::is_same<Objects, ColorObjects>::value || TEX;
    constexpr bool ROUGH = std::is_same<Objects, RoughObjects>::value || COLOR;
    constexpr bool LIGHT = std::is_same<Objects, LightObjects>::value || ROUGH;
    constexpr bool PBR = std::is_same<Objects, PbrObjects>::value || LIGHT;
    constexpr bool SMOOTH = std::is_same<Objects, SmoothObjects>::value || PBR;
    constexpr bool OBJ = std::is_same<Objects, ObjTable>::value || SMOOTH;
    constexpr bool EDIT = std::is_same<Objects, TransEdit>::value;
    constexpr bool NRM = std::is_same<Objects, ShadeNormals>::value || std::is_same<Objects, MapEdit<ShadeNormals>>::value ||
                         std::is_same<Objects, Relight<ShadeNormals>>::value;
    __shared__ int s_stack[kStack * kBlock];
    const int tid = threadIdx.y * kTileX + threadIdx.x;
    const int j = blockIdx.x * kTileX + threadIdx.x, i = blockIdx.y * kTileY + threadIdx.y;
    if (i >= q.H || j >= q.W) return;   // no barriers below: each lane's stack column is its own
    LdsStack stk{s_stack + tid};
    const long pix = (long)i * q.W + j;
    const bool have_tab = q.row_cdf[q.He] > 0.0f;   // an envmap of zero luminance has no emitter sampling
    bool have_tab_b = false;                        // (RELIGHT) the same of the table's environment
    if constexpr (RELIGHT) have_tab_b = ot.row_cdf_b[ot.He_b] > 0.0f;
    int n_e = 1;   // (LIGHT) the emitters: the envmap where it has tables, then the lights
    if constexpr (LIGHT) n_e = (have_tab ? 1 : 0) + ot.lt.n;
    float n_ef = (float)n_e;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    float dacc[3] = {0.0f, 0.0f, 0.0f};   // (MAPEDIT) delta's sum, in registers within a launch as acc is
    uint32_t n_second = 0;                // (MAPEDIT) second walks of this launch
    float racc[3] = {0.0f, 0.0f, 0.0f};   // (RELIGHT) relit's sum, in registers within a launch as acc is
    if constexpr (RELIGHT) {
        if (!first) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                acc[c] = q.out[3 * pix + c];
                racc[c] = ot.relit[3 * pix + c];
            }
        }
    } else if constexpr (MAPEDIT) {
        if (!first) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                acc[c] = q.out[3 * pix + c];
                dacc[c] = ot.delta[3 * pix + c];
            }
        }
    } else if constexpr (DIFF) {
        if (first) {
#pragma unroll
            for (int c = 0; c < 3; ++c) ot.fg[3 * pix + c] = ot.delta[3 * pix + c] = 0.0f;
            ot.alpha[pix] = 0.0f;
            if constexpr (THROUGH) {
#pragma unroll
                for (int c = 0; c < 3; ++c) ot.through[3 * pix + c] = 0.0f;
            }
            if constexpr (BASE) {
#pragma unroll
                for (int c = 0; c < 3; ++c) ot.base[3 * pix + c] = 0.0f;
            }
        }
    } else if (!first) {
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] = q.out[3 * pix + c];
    }
    const uint32_t pix_hash = pcg_hash(q.seed_hash + (uint32_t)pix);
    uint32_t n_rays = 0;
    // (DIFF) a sample takes up to two trips through the loop's body: trip 1 (`second`) repeats the iteration of `s` that trip 0 asked it for
    bool second = false;
    bool cov = false, touched = false;      // trip 0's record
    float Lw[3] = {0.0f, 0.0f, 0.0f};       // trip 0's radiance, kept across trip 1
    bool chain = false;                     // (THROUGH) trip 0: every vertex so far was a dielectric one
    int land = -1;                          // (THROUGH) trip 0's record: the depth at which the chain landed on the depth mesh's front
    for (int s = s0; s < s1; ++s) {
        const uint32_t base = pcg_hash(pix_hash + (uint32_t)s);
        if constexpr (DIFF) {
            if (!second) {
                cov = false;
                touched = ot.lt.n > 0;   // a light changes n_e, and through it every emitter sample
                if constexpr (THROUGH) {
                    chain = true;
                    land = -1;
                }
            }
            n_e = (have_tab ? 1 : 0) + (second ? 0 : ot.lt.n);   // trip 1: the envmap alone
            n_ef = (float)n_e;
        }
        if constexpr (MAPEDIT) {
            if (!second) touched = false;
        }
        float L[3] = {0.0f, 0.0f, 0.0f}, thr[3] = {1.0f, 1.0f, 1.0f};
        float L1[3] = {0.0f, 0.0f, 0.0f};   // (RELIGHT) the sample's radiance under the table's environment
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
        int med = -1;              // (MEDIUM) the object whose medium the ray is in; -1: none, as at the camera
        for (int depth = 0;; ++depth) {
            float t = FLT_MAX;
            ++n_rays;
            // (DIFF) the traversals skip the triangles from an id on: none in trip 0, the inserted ones in trip 1
            int id_limit = id_limit_of(ot, second);
            if constexpr (THROUGH) id_limit = id_limit_at(ot, second, depth, land);   // (THROUGH) a function of the depth
            const int k = trace<false, DIFF>(q.nodes, q.tris, o, d, 0.0f, t, stk, id_limit);
            int med_seg = -1;   // (MEDIUM) the medium of this segment: a traversal that skips the inserted triangles is in none
            if constexpr (MEDIUM) {
                med_seg = DIFF && id_limit != INT32_MAX ? -1 : med;
                // a ray that escapes inside a medium (an open mesh) drops it without attenuation; else the trace gave t: the flight is
                // sampled from sigma_s alone and the absorption over the distance flown is an analytic weight
                if (med_seg >= 0 && k >= 0) {
                    const MatpbrPathObjectMedium mr = medium_of(ot, med_seg);
                    float dist, tw[3];
                    const bool scattered = medium_segment(mr, t, mr.sigma_s > 0.0f ? rng_u(base, depth, 9) : 0.0f, dist, tw);
#pragma unroll
                    for (int c = 0; c < 3; ++c) thr[c] *= tw[c];
                    if (scattered) {   // a medium vertex at o + s d: no emitter sample (the boundary is a dielectric), no spawn offset
                        if constexpr (THROUGH) {
                            if (!second) chain = false;
                        }
                        if (depth + 1 >= q.max_depth) break;
                        float wi[3];
                        phase_sample(mr.g, d, rng_u(base, depth, 10), rng_u(base, depth, 11), wi);
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            o[c] = fmaf(dist, d[c], o[c]);
                            d[c] = wi[c];
                        }
                        prev_delta = true;   // whatever the ray meets next takes MIS weight 1
                        continue;
                    }
                }
            }
            if constexpr (DIFF) {
                if (k >= 0 && tri_id(q.tris[3 * k]) >= ot.n_scene_tri) {   // trip 0 alone can meet one ((THROUGH) and trip 1's chain)
                    touched = true;
                    if (depth == 0) cov = true;
                }
            }
            if constexpr (THROUGH) {
                // the chain lands on the depth mesh: on its front the photograph at the point's texel is what arrives from there, added
                // before the max_depth test as a light's emission is; `touched` then records what the objects change after the landing
                if (!second && chain && depth >= 1 && k >= 0 && tri_id(q.tris[3 * k]) < ot.n_scene_tri) {
                    chain = false;
                    const float4 B = q.tris[3 * k + 1], C = q.tris[3 * k + 2];
                    const float e1[3] = {B.x, B.y, B.z}, e2[3] = {C.x, C.y, C.z};
                    float n[3];
                    cross3(e1, e2, n);
                    if (-dot3(n, d) * rsq(dot3(n, n)) > 0.0f) {
                        float p[3];
#pragma unroll
                        for (int c = 0; c < 3; ++c) p[c] = fmaf(t, d[c], o[c]);
                        const long tq = screen_texel(p, q.f_ndc, q.aspect, q.H, q.W);
#pragma unroll
                        for (int c = 0; c < 3; ++c) ot.through[3 * pix + c] += thr[c] * ot.photo[3 * tq + c];
                        if constexpr (REFLECT) {   // the chain's own light goes to fg here: from now on L is the tail's
#pragma unroll
                            for (int c = 0; c < 3; ++c) {
                                ot.fg[3 * pix + c] += L[c];
                                L[c] = 0.0f;
                            }
                        }
                        land = depth;
                        touched = ot.lt.n > 0;
                    }
                }
            }
            if constexpr (DIFF && MEDIUM) {   // a mesh that pokes through the scene: the segment reached the scene inside a medium
                if (med_seg >= 0 && k >= 0 && tri_id(q.tris[3 * k]) < ot.n_scene_tri) touched = true;
            }
            if (k < 0) {   // escaped: the envmap, MIS-weighted against emitter sampling after a BSDF sample
                if constexpr (RELIGHT) {   // each environment at its own texel, with its own weight against the shared prev_pdf
#pragma nounroll
                    for (int e = 0; e < 2; ++e) {
                        const float* const env = e ? ot.env_b : q.env;
                        const float* const env_pdf = e ? ot.env_pdf_b : q.env_pdf;
                        const int tx = env_texel(d, e ? ot.He_b : q.He, e ? ot.We_b : q.We);
                        const float w = depth == 0 ? 1.0f : mis_weight(prev_pdf, (e ? have_tab_b : have_tab) ? env_pdf[tx] : 0.0f);
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            float Ls = e ? L1[c] : L[c];   // this environment's sum
                            Ls += thr[c] * (env[3 * tx + c] * w);
                            L[c] = e ? L[c] : Ls;
                            L1[c] = e ? Ls : L1[c];
                        }
                    }
                    break;
                }
                const int tx = env_texel(d, q.He, q.We);
                const float w = depth == 0 || (OBJ && prev_delta)
                                    ? 1.0f
                                    : mis_weight(prev_pdf, have_tab ? (LIGHT ? q.env_pdf[tx] / n_ef : q.env_pdf[tx]) : 0.0f);
#pragma unroll
                for (int c = 0; c < 3; ++c) L[c] += thr[c] * (q.env[3 * tx + c] * w);
                break;
            }
            int kind = 0;          // (OBJ) 0: the depth mesh; else the inserted object's BSDF and its parameters
            float op[3] = {0.0f, 0.0f, 0.0f};
            float oa[3] = {0.0f, 0.0f, 0.0f}, o_r = 0.0f, o_m = 0.0f;   // (PBR) the record of an object of kind 3
            bool colored = false;         // (COLOR) the object's reflectance or albedo is multiplied by its interpolated corner colours
            bool textured = false;        // (TEX) the object's images are read at its interpolated corner coordinates
            float bu = 0.0f, bv = 0.0f;   // (COLOR) u, v of the winning triangle, formed once for the texture, the colour and the smooth normal
            if constexpr (LIGHT) {   // the table lookup moves ahead of the max_depth test: a light's emission is added as the envmap's escape term is
                const LightLookup f = light_lookup<(REFLECT ? MATPBR_PATH_OBJECT_PHOTO : 0) |
                                                   (TEX     ? MATPBR_PATH_OBJECT_SMOOTH | MATPBR_PATH_OBJECT_COLORED | MATPBR_PATH_OBJECT_TEXTURED :
                                                    COLOR ? MATPBR_PATH_OBJECT_SMOOTH | MATPBR_PATH_OBJECT_COLORED : MATPBR_PATH_OBJECT_SMOOTH)>(
                    ot, __float_as_int(q.tris[3 * k].w));
                kind = f.kind;
                op[0] = f.p0; op[1] = f.p1; op[2] = f.p2;
                oa[0] = f.a0; oa[1] = f.a1; oa[2] = f.a2;
                o_r = f.r; o_m = f.m;
                const float area = f.area;
                if (kind == MATPBR_PATH_BSDF_AREA) {
                    const float4 B = q.tris[3 * k + 1], C = q.tris[3 * k + 2];
                    const float e1[3] = {B.x, B.y, B.z}, e2[3] = {C.x, C.y, C.z};
                    float n[3];
                    cross3(e1, e2, n);
                    const float cos_o = -dot3(n, d) * rsq(dot3(n, n));
                    if (cos_o > 0.0f) {   // one-sided: the back ends the path with nothing added
                        const float w = depth == 0 || prev_delta ? 1.0f : mis_weight(prev_pdf, light_hit_pdf(t, area, cos_o, n_ef));
#pragma unroll
                        for (int c = 0; c < 3; ++c) L[c] += thr[c] * (op[c] * w);
                    }
                    break;
                }
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
            if constexpr (LIGHT) {
            } else if constexpr (PBR) kind = object_lookup(ot.t, ot.pbr, __float_as_int(q.tris[3 * k].w), op, oa, o_r, o_m);
            else if (OBJ) kind = object_of(ot, __float_as_int(q.tris[3 * k].w), op);
            bool smooth = false;   // (SMOOTH) the object shades with its interpolated corner normals, `ns` below
            if constexpr (SMOOTH) {
                smooth = (kind & MATPBR_PATH_OBJECT_SMOOTH) != 0;
                kind &= ~MATPBR_PATH_OBJECT_SMOOTH;
            }
            if constexpr (COLOR) {
                colored = (kind & MATPBR_PATH_OBJECT_COLORED) != 0;
                kind &= ~MATPBR_PATH_OBJECT_COLORED;
            }
            if constexpr (TEX) {
                textured = (kind & MATPBR_PATH_OBJECT_TEXTURED) != 0;
                kind &= ~MATPBR_PATH_OBJECT_TEXTURED;
            }
            int med_obj = -1;   // (MEDIUM) the vertex lies on this object, whose kind carries the medium flag
            if constexpr (MEDIUM) {
                if (kind & MATPBR_PATH_OBJECT_MEDIUM) med_obj = medium_index(ot.t, __float_as_int(q.tris[3 * k].w));
                kind &= ~MATPBR_PATH_OBJECT_MEDIUM;
            }
            bool photo_obj = false;   // (REFLECT) the vertex lies on an object that carries the photo flag
            if constexpr (REFLECT) {
                photo_obj = (kind & MATPBR_PATH_OBJECT_PHOTO) != 0;
                kind &= ~MATPBR_PATH_OBJECT_PHOTO;
            }
            if constexpr (THROUGH) {
                // rough glass and every other kind end the chain; (REFLECT) a flagged object of any kind keeps it
                if (!second) chain = chain && (kind == MATPBR_PATH_BSDF_DIELECTRIC || (REFLECT && photo_obj));
            }
            // a hit on the back of a triangle ends the path (glass shades from both sides)
            const bool rough = ROUGH && kind == MATPBR_PATH_BSDF_ROUGH_DIELECTRIC;   // (ROUGH) shades from both sides, like glass
            if (!(OBJ && kind == MATPBR_PATH_BSDF_DIELECTRIC) && !rough && !(dot3(n, wo) > 0.0f)) break;
            float p[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) p[c] = fmaf(t, d[c], o[c]);
            // material: the texel the hit point projects to by the inverse of the camera above (one focal length for both axes; a6
            // world_to_screen when H = W), floor, clamped to the image (MatDiffBSDF)
            const float ndc0 = q.f_ndc * (-p[0]) / p[2], ndc1 = (q.f_ndc * q.aspect) * p[1] / p[2];
            const float sx = (ndc0 + 1.0f) * 0.5f * (float)q.W, sy = (ndc1 + 1.0f) * 0.5f * (float)q.H;
            const int tx = (int)fminf(fmaxf(floorf(sx), 0.0f), (float)(q.W - 1)), ty = (int)fminf(fmaxf(floorf(sy), 0.0f), (float)(q.H - 1));
            const long tp = OBJ && kind != 0 ? 0 : (long)ty * q.W + tx;   // an object reads no texel
            float av[3] = {0.0f, 0.0f, 0.0f}, rv = 0.0f, mv = 0.0f;
            if constexpr (MAPEDIT) {   // trip 0 reads the edited maps at a masked texel; the first such read asks for trip 1
                const bool edited = !second && ot.mask[tp] != 0;
                touched = touched || edited;
                const float *pa = edited ? ot.a_e : q.a, *pr = edited ? ot.r_e : q.r, *pm = edited ? ot.m_e : q.m;
                av[0] = pa[3 * tp]; av[1] = pa[3 * tp + 1]; av[2] = pa[3 * tp + 2];
                rv = pr[tp]; mv = pm[tp];
            } else {
                av[0] = q.a[3 * tp]; av[1] = q.a[3 * tp + 1]; av[2] = q.a[3 * tp + 2];
                rv = q.r[tp]; mv = q.m[tp];
            }
            const bool pbr = PBR && kind == MATPBR_PATH_BSDF_PBR;   // (PBR) the depth mesh's branch on the object's constants
            if constexpr (PBR) {
                if (pbr) { av[0] = oa[0]; av[1] = oa[1]; av[2] = oa[2]; rv = o_r; mv = o_m; }
            }
            if constexpr (COLOR) {
                if (smooth || colored || (TEX && textured)) {
                    const float4 A = q.tris[3 * k];
                    const float v0[3] = {A.x, A.y, A.z};
                    tri_uv(v0, e1, e2, o, d, bu, bv);
                }
                if (colored) {   // its nine corner colours, consumed at once
                    const float* cp = ot.col + 9 * (long)(__float_as_int(q.tris[3 * k].w) - ot.n_scene_tri);
                    float cc[9], cv[3];
#pragma unroll
                    for (int c = 0; c < 9; ++c) cc[c] = cp[c];
                    object_color(cc, bu, bv, cv);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        av[c] *= cv[c];
                        op[c] *= cv[c];
                    }
                }
            }
            if constexpr (TEX) {
                if (textured) {   // its six corner coordinates, consumed at once; the orm fetch follows the base fetch
                    const int id = __float_as_int(q.tris[3 * k].w);
                    const MatpbrPathObjectTex tr = tex_lookup(ot.t, ot.tex, id);
                    const float* up = ot.uv + 6 * (long)(id - ot.n_scene_tri);
                    float cs[6], ts, tt, cb[3];
#pragma unroll
                    for (int c = 0; c < 6; ++c) cs[c] = up[c];
                    object_st(cs, bu, bv, ts, tt);
                    if (tr.base_w > 0) {
                        texture_fetch(ot.texels + (long)tr.base_first, tr.base_w, tr.base_h, ts, tt, cb);
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            av[c] *= cb[c];
                            op[c] *= cb[c];
                        }
                    }
                    if (tr.orm_w > 0) {   // kind 3 only: the record check refuses it elsewhere
                        texture_fetch(ot.texels + (long)tr.orm_first, tr.orm_w, tr.orm_h, ts, tt, cb);
                        orm_apply(cb, rv, mv);
                    }
                }
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
                    float cn[9], su, sv;
#pragma unroll
                    for (int c = 0; c < 9; ++c) cn[c] = cp[c];
                    if constexpr (COLOR) { su = bu; sv = bv; }
                    else tri_uv(v0, e1, e2, o, d, su, sv);
                    smooth_normal(cn, su, sv, n, ns);
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
            // (REFLECT) trip 1 takes none below the landing: the chain's own light is not the tail's
            // (RELIGHT) one per environment that has tables, from the same dims 2-5, each with its own shadow ray and MIS weight
            if constexpr (RELIGHT) {
#pragma nounroll
                for (int e = 0; e < 2; ++e) {
                    if (!(e ? have_tab_b : have_tab)) continue;
                    const float* const env = e ? ot.env_b : q.env;
                    float wl[3], pdf_e;
                    const int te = env_sample(e ? ot.row_cdf_b : q.row_cdf, e ? ot.col_cdf_b : q.col_cdf, e ? ot.env_pdf_b : q.env_pdf,
                                              e ? ot.He_b : q.He, e ? ot.We_b : q.We, rng_u(base, depth, 2), rng_u(base, depth, 3),
                                              rng_u(base, depth, 4), rng_u(base, depth, 5), wl, pdf_e);
                    if (pdf_e > 0.0f && dot3(n, wl) > 0.0f) {
                        float f[3], pdf_b;
                        path_eval(wl, wo, NRM ? ns : n, av, rv, mv, f, pdf_b);
                        if (f[0] > 0.0f || f[1] > 0.0f || f[2] > 0.0f) {
                            float ts = FLT_MAX;
                            ++n_rays;
                            if (trace<true, false>(q.nodes, q.tris, po, wl, 0.0f, ts, stk, id_limit) < 0) {   // no occluder
                                const float w = mis_weight(pdf_e, pdf_b) / pdf_e;
#pragma unroll
                                for (int c = 0; c < 3; ++c) {
                                    float Ls = e ? L1[c] : L[c];   // this environment's sum
                                    Ls += thr[c] * (f[c] * (env[3 * te + c] * w));
                                    L[c] = e ? L[c] : Ls;
                                    L1[c] = e ? Ls : L1[c];
                                }
                            }
                        }
                    }
                }
            } else if (((ROUGH ? n_e > 0 : LIGHT) || have_tab) && !(OBJ && kind == MATPBR_PATH_BSDF_DIELECTRIC) && !(REFLECT && second && depth < land)) {
                float wl[3], pdf_e;
                int te = 0;
                float Le[3] = {0.0f, 0.0f, 0.0f}, ts_max = FLT_MAX;   // (LIGHT) the chosen emitter's radiance, the shadow ray's reach
                if constexpr (LIGHT) {   // one emitter of n_e by sample reuse of dim 2; pdf_e carries the 1 / n_e
                    float u_re;
                    const int idx = emitter_choose(rng_u(base, depth, 2), n_e, u_re);
                    if (have_tab && idx == 0) {
                        te = env_sample(q.row_cdf, q.col_cdf, q.env_pdf, q.He, q.We, u_re, rng_u(base, depth, 3), rng_u(base, depth, 4),
                                        rng_u(base, depth, 5), wl, pdf_e);
                        pdf_e = pdf_e / n_ef;
#pragma unroll
                        for (int c = 0; c < 3; ++c) Le[c] = q.env[3 * te + c];
                    } else {   // dim 5 is unused for a light
                        const int l = idx - (have_tab ? 1 : 0);
                        float y[3], dist;
                        light_sample(ot.lt, l, u_re, rng_u(base, depth, 3), rng_u(base, depth, 4), po, n_ef, y, wl, dist, pdf_e);
                        light_radiance(ot.lt, l, Le);
                        ts_max = dist * (1.0f - kShadowEps);
                    }
                } else {
                    te = env_sample(q.row_cdf, q.col_cdf, q.env_pdf, q.He, q.We, rng_u(base, depth, 2), rng_u(base, depth, 3),
                                    rng_u(base, depth, 4), rng_u(base, depth, 5), wl, pdf_e);
                }
                if (pdf_e > 0.0f && (rough || dot3(n, wl) > 0.0f)) {   // (ROUGH) a rough dielectric takes the sample on either side of its face
                    float f[3], pdf_b;
                    if constexpr (ROUGH) {
                        if (rough) {   // the shadow ray starts on wl's side of the face
                            const float side = dot3(n, wl) > 0.0f ? eps : -eps;
#pragma unroll
                            for (int c = 0; c < 3; ++c) po[c] = fmaf(side, n[c], p[c]);
                        }
                    }
                    if (rough) {
                        rough_eval(op, n, ns, wo, wl, f[0], pdf_b);
                        f[1] = f[2] = f[0];
                    } else if (OBJ && kind == MATPBR_PATH_BSDF_DIFFUSE) {   // f cos = rho / pi max(n . wi, 0), pdf = cos / pi
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
                        float ts = LIGHT ? ts_max : FLT_MAX;
                        ++n_rays;
                        const int ks = trace<true, DIFF>(q.nodes, q.tris, po, wl, 0.0f, ts, stk, id_limit);   // the occluder
                        if constexpr (DIFF) {
                            if (ks >= 0 && tri_id(q.tris[3 * ks]) >= ot.n_scene_tri) touched = true;
                        }
                        if (ks < 0) {
                            const float w = mis_weight(pdf_e, pdf_b) / pdf_e;
#pragma unroll
                            for (int c = 0; c < 3; ++c) L[c] += thr[c] * (f[c] * ((LIGHT ? Le[c] : q.env[3 * te + c]) * w));
                        }
                    }
                }
            }
            // BSDF sample: the next ray
            float wi[3], wgt[3], pdf_s;
            if (OBJ && kind != 0 && !pbr) {
                int flags;
                if (rough)
                    rough_sample(op, n, ns, wo, rng_u(base, depth, 6), rng_u(base, depth, 7), rng_u(base, depth, 8), wi, wgt, pdf_s, flags);
                else if (SMOOTH && smooth)
                    object_sample_shading(kind, op, n, ns, wo, rng_u(base, depth, 6), rng_u(base, depth, 7), rng_u(base, depth, 8), wi, wgt, pdf_s, flags);
                else
                    object_sample(kind, op, n, wo, rng_u(base, depth, 6), rng_u(base, depth, 7), rng_u(base, depth, 8), wi, wgt, pdf_s, flags);
                prev_delta = (flags & kFlagDelta) != 0;
                if constexpr (MEDIUM) {   // the side the ray leaves on decides: into the object, its medium; out of it, none
                    if (med_obj >= 0) med = dot3(n, wi) < 0.0f ? med_obj : -1;
                }
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
        if constexpr (DIFF) {
            if (!second) {
#pragma unroll
                for (int c = 0; c < 3; ++c) Lw[c] = L[c];
                if constexpr (THROUGH) {
                    if (touched && (!cov || (land >= 0 && land + 1 < q.max_depth))) {   // the same s once more; (cov) the landing's tail
                        second = true;
                        --s;
                        continue;
                    }
                } else if (touched && !cov) {   // the same s once more
                    second = true;
                    --s;
                    continue;
                }
            }
            if (cov) {
                if (THROUGH && second) {   // a see-through sample walked twice: what the objects change in the landing's light
#pragma unroll
                    for (int c = 0; c < 3; ++c) ot.fg[3 * pix + c] += Lw[c] - L[c];
                    if (ot.rewalked) ot.rewalked[pix] += 1u;
                } else if (THROUGH && land >= 0) {
                    // a see-through sample with an untouched tail: both tails are the same arithmetic, so it adds exactly nothing to fg
                    // (a tail that max_depth cuts has Lw = 0: nothing is added along a dielectric chain)
                } else {
#pragma unroll
                    for (int c = 0; c < 3; ++c) ot.fg[3 * pix + c] += Lw[c];
                }
                ot.alpha[pix] += 1.0f;
            } else if (second) {   // an untouched sample adds nothing: no subtraction
#pragma unroll
                for (int c = 0; c < 3; ++c) ot.delta[3 * pix + c] += Lw[c] - L[c];
                if (ot.rewalked) ot.rewalked[pix] += 1u;
            }
            if constexpr (BASE) {
                // the walk without the objects of a sample that misses them: trip 1's L, or trip 0's where it met none (then L is Lw)
                if (!cov) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) ot.base[3 * pix + c] += L[c];
                }
            }
            second = false;
        } else if constexpr (MAPEDIT) {
            if (!second && touched) {   // the same s once more, on the fitted maps
#pragma unroll
                for (int c = 0; c < 3; ++c) Lw[c] = L[c];
                second = true;
                --s;
                continue;
            }
            if (second) {   // an untouched sample adds nothing: no subtraction
#pragma unroll
                for (int c = 0; c < 3; ++c) dacc[c] += Lw[c] - L[c];
                ++n_second;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += L[c];   // the fitted maps' radiance: trip 1's, or the only trip's, which read no edited texel
            second = false;
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += L[c];
            if constexpr (RELIGHT) {
#pragma unroll
                for (int c = 0; c < 3; ++c) racc[c] += L1[c];
            }
        }
    }
    const float sc = last ? 1.0f / (float)q.spp : 1.0f;
    if constexpr (DIFF) {
        if (last) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                ot.fg[3 * pix + c] *= sc;
                ot.delta[3 * pix + c] *= sc;
                if constexpr (THROUGH) ot.through[3 * pix + c] *= sc;
                if constexpr (BASE) ot.base[3 * pix + c] *= sc;
            }
            ot.alpha[pix] *= sc;
        }
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) q.out[3 * pix + c] = last ? acc[c] * sc : acc[c];
    }
    if constexpr (MAPEDIT) {
#pragma unroll
        for (int c = 0; c < 3; ++c) ot.delta[3 * pix + c] = last ? dacc[c] * sc : dacc[c];
        if (ot.rewalked) ot.rewalked[pix] += n_second;
    }
    if constexpr (RELIGHT) {
#pragma unroll
        for (int c = 0; c < 3; ++c) ot.relit[3 * pix + c] = last ? racc[c] * sc : racc[c];
    }
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
        const long tp = screen_texel(p, q.f_ndc, q.aspect, q.H, q.W);
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

// =================================================================================================================================
// C ABI
// =================================================================================================================================
// the camera of a frame: rays ((x - cx)/f_pix, -(y - cy)/f_pix, -1), texels ndc0 = f_ndc x/(-z), ndc1 = f_ndc aspect y/z
struct Camera {
    double th;             // tan(fov_x / 2)
    float f_pix, cx, cy;   // f = (W/2)/tan(fov/2), c = (W-1)/2, (H-1)/2
    float f_ndc, aspect;   // perspective_projection_matrix (mi_plugin.py:585-595): 1/tan(fov_x/2), W/H
};
Camera camera(int H, int W, float fov_x_deg) {
    const double th = std::tan(0.5 * (double)fov_x_deg * 3.14159265358979323846 / 180.0);
    return {th, (float)((0.5 * W) / th), 0.5f * (float)(W - 1), 0.5f * (float)(H - 1), (float)(1.0 / th), (float)W / (float)H};
}
bool fov_valid(float fov_x_deg) { return fov_x_deg > 0.0f && fov_x_deg < 180.0f; }
dim3 tile_grid(int H, int W) { return dim3((unsigned)((W + kTileX - 1) / kTileX), (unsigned)((H + kTileY - 1) / kTileY)); }

// the common arguments of a render or a backward pass, as the C ABI receives them and in its order
struct Frame {
    const void *nodes, *tris;
    const float *a, *r, *m;
    int H, W;
    float fov_x_deg;
    const float *env, *row_cdf, *col_cdf, *env_pdf;
    int He, We, spp, max_depth;
    uint32_t seed;
    int spp_per_launch;
    float* out;   // the render's image; null in a backward pass
    uint32_t* rays;
    void* stream;
};
// the checks a render and a backward pass share, and the kernels' arguments (`out` and the backward pass's own are the caller's to check)
bool frame_args(const Frame& f, PathArgs& q) {
    if (!f.nodes || !f.tris || !f.a || !f.r || !f.m || !f.env || !f.row_cdf || !f.col_cdf || !f.env_pdf || f.H <= 0 || f.W <= 0 || f.He <= 0 ||
        f.We <= 0 || f.spp <= 0 || f.spp_per_launch <= 0 || f.max_depth < 1 || f.max_depth > MATPBR_PATH_MAX_MAX_DEPTH || !fov_valid(f.fov_x_deg))
        return false;
    q.nodes = static_cast<const float4*>(f.nodes);
    q.tris = static_cast<const float4*>(f.tris);
    q.a = f.a; q.r = f.r; q.m = f.m;
    q.env = f.env; q.row_cdf = f.row_cdf; q.col_cdf = f.col_cdf; q.env_pdf = f.env_pdf;
    q.out = f.out;
    q.rays = f.rays;
    q.H = f.H; q.W = f.W; q.He = f.He; q.We = f.We; q.spp = f.spp; q.max_depth = f.max_depth;
    const Camera c = camera(f.H, f.W, f.fov_x_deg);
    q.f_pix = c.f_pix; q.cx = c.cx; q.cy = c.cy;
    q.f_ndc = c.f_ndc; q.aspect = c.aspect;
    q.seed_hash = pcg_hash(f.seed);
    return true;
}

// the path_kernel instantiation a render launches; it also says which members of `Scene` the launch reads
enum class Kernel { NoObjects, ObjTable, SmoothObjects, PbrObjects, LightObjects, RoughObjects, ColorObjects, TexObjects, MediumObjects, TransEdit, ShadeNormals };
// what a render hands its kernel besides the frame, checked
struct Scene {
    Kernel kernel = Kernel::NoObjects;
    ObjTable ot{};
    const float* obj_nrm = nullptr;             // set where some object is smooth
    int32_t n_scene_tri = 0;
    const MatpbrPathObjectPbr* pbr = nullptr;   // set where some object is of kind 3
    LightTable lt{};                            // empty (n = 0) where no object is a light
    const float* obj_col = nullptr;             // set where some object is coloured
    const float* obj_uv = nullptr;              // set where some object is textured, with its records and the texels
    const MatpbrPathObjectTex* tex = nullptr;
    const float4* texels = nullptr;
    const MatpbrPathObjectMedium* media = nullptr;   // set where some object holds a medium
    int n_photo = 0;                                 // how many objects carry MATPBR_PATH_OBJECT_PHOTO
    TransEdit edit{};
    const float* nrm = nullptr;
};

template <class Table>
int launch_frame(const Frame& f, const PathArgs& q, const Table& table) {
    const dim3 grid = tile_grid(f.H, f.W), block(kTileX, kTileY);
    for (int s0 = 0; s0 < f.spp; s0 += f.spp_per_launch) {
        const int s1 = std::min(f.spp, s0 + f.spp_per_launch);
        const int first = s0 == 0 ? 1 : 0, last = s1 == f.spp ? 1 : 0;
        hipLaunchKernelGGL(path_kernel<Table>, grid, block, 0, (hipStream_t)f.stream, q, s0, s1, first, last, table);
        if (hipGetLastError() != hipSuccess) return MATPBR_PATH_ERR_LAUNCH;
    }
    return MATPBR_PATH_OK;
}

// the widest table over what `s` holds: a member the scene does not have stays zero, and a kernel that takes a narrower table is
// handed its part
TexObjects tex_objects(const Scene& s) {
    TexObjects ro{};
    ro.t = s.ot;
    ro.nrm = s.obj_nrm;
    ro.n_scene_tri = s.n_scene_tri;
    for (int k = 0; s.pbr && k < s.ot.n; ++k) ro.pbr[k] = s.pbr[k];
    ro.lt = s.lt;
    ro.col = s.obj_col;
    ro.uv = s.obj_uv;
    ro.texels = s.texels;
    for (int k = 0; s.tex && k < s.ot.n; ++k)   // a record is copied where its object carries the flag: the others stay zero
        if (s.ot.o[k].kind & MATPBR_PATH_OBJECT_TEXTURED) ro.tex[k] = s.tex[k];
    return ro;
}
// the medium records of `s` into a table that carries them: a record is copied where its object carries the flag, the others stay zero
template <class Table>
void media_into(const Scene& s, Table& t) {
    for (int k = 0; s.media && k < s.ot.n; ++k)
        if (s.ot.o[k].kind & MATPBR_PATH_OBJECT_MEDIUM) t.med[k] = s.media[k];
}

int render_common(const Frame& f, const Scene& s) {
    PathArgs q{};
    if (!f.out || !frame_args(f, q)) return MATPBR_PATH_ERR_INVALID_ARG;
    switch (s.kernel) {
        case Kernel::NoObjects: return launch_frame(f, q, NoObjects{});
        case Kernel::ObjTable: return launch_frame(f, q, s.ot);
        case Kernel::SmoothObjects: return launch_frame(f, q, SmoothObjects{s.ot, s.obj_nrm, s.n_scene_tri});
        case Kernel::TransEdit: return launch_frame(f, q, s.edit);
        case Kernel::ShadeNormals: return launch_frame(f, q, ShadeNormals{s.nrm});
        default: break;
    }
    const TexObjects ro = tex_objects(s);   // the five kernels whose tables extend one another
    if (s.kernel == Kernel::PbrObjects) return launch_frame<PbrObjects>(f, q, ro);
    if (s.kernel == Kernel::TexObjects) return launch_frame(f, q, ro);
    if (s.kernel == Kernel::MediumObjects) {
        MediumObjects mo{};
        static_cast<TexObjects&>(mo) = ro;
        media_into(s, mo);
        return launch_frame(f, q, mo);
    }
    return s.kernel == Kernel::LightObjects ? launch_frame<LightObjects>(f, q, ro) :
           s.kernel == Kernel::RoughObjects ? launch_frame<RoughObjects>(f, q, ro) : launch_frame<ColorObjects>(f, q, ro);
}

// what a table with a textured object needs besides the flag's place (object_table): the three buffers, texels aligned for float4
// loads, and a valid record for every flagged object
bool textures_valid(const MatpbrPathObject* objects, int n_objects, const float* obj_uv, const MatpbrPathObjectTex* tex, const void* texels,
                    long n_texels) {
    if (!obj_uv || !tex || !texels || ((uintptr_t)texels & 15) || n_texels < 1) return false;
    for (int k = 0; k < n_objects; ++k) {
        if (!(objects[k].kind & MATPBR_PATH_OBJECT_TEXTURED)) continue;
        const int base = objects[k].kind & ~(MATPBR_PATH_OBJECT_TEXTURED | MATPBR_PATH_OBJECT_COLORED | MATPBR_PATH_OBJECT_SMOOTH | MATPBR_PATH_OBJECT_PHOTO);
        if (!tex_valid(tex[k], base == MATPBR_PATH_BSDF_PBR, n_texels)) return false;
    }
    return true;
}

// n_scene_tri against a checked table: an int32 >= 0, and no range starts below it
bool ranges_above(const MatpbrPathObject* objects, int n_objects, long n_scene_tri) {
    if (n_scene_tri < 0 || n_scene_tri > INT32_MAX) return false;
    for (int k = 0; k < n_objects; ++k)
        if (objects[k].first_tri < n_scene_tri) return false;
    return true;
}
// The table of an entry point that knows n_scene_tri, with the rules those entries share: n_scene_tri as `ranges_above` has it, and
// corner normals are given where an object is smooth.
bool scene_table(const MatpbrPathObject* objects, int n_objects, unsigned accept, const float* obj_nrm, long n_scene_tri,
                 const MatpbrPathObjectPbr* pbr, ObjTable& ot, ObjCounts& n) {
    return object_table(objects, n_objects, accept, pbr, ot, &n) && ranges_above(objects, n_objects, n_scene_tri) && !(n.smooth > 0 && !obj_nrm);
}

// the object arguments of an entry point, as the C ABI receives them and in its order: an entry leaves what it does not have null / 0
struct ObjectArgs {
    const MatpbrPathObject* objects;
    int n_objects;
    const float* obj_nrm = nullptr;
    long n_scene_tri = 0;
    const MatpbrPathObjectPbr* pbr = nullptr;
    const MatpbrPathLights* lights = nullptr;
    const void* light_tris = nullptr;
    const float* light_cdf = nullptr;
    const float* obj_col = nullptr;
    const float* obj_uv = nullptr;
    const MatpbrPathObjectTex* tex = nullptr;
    const void* texels = nullptr;
    long n_texels = 0;
    const MatpbrPathObjectMedium* media = nullptr;
};

// The nine object entries are the nine levels of this one rule (the table in DESIGN.md section 1.4, "The object entries"): level 1
// admits kinds 1 and 2, level 2 the smooth flag on them, level 3 kind 3, level 4 kind 4, level 5 kind 5, level 6 the colour flag on
// kinds 2 and 3 (obj_col is consulted where an object carries it), level 7 the texture flag on them (obj_uv, tex and texels are consulted
// where an object carries it, and its record is checked against n_texels), level 8 the medium flag on kinds 1 and 5 (media is consulted
// where an object carries it, and its record is checked; its kernel is chosen first), level 9 the photo flag on kinds 2, 3 and 5 (it
// chooses no kernel here: matpbr_path_render_objects_reflect reads n_photo).  An entry passes null / 0 for
// the arguments it does not have; level 1's n_scene_tri = 0 lies below every range.  An argument is consulted only where the table needs
// it: obj_nrm where an object is smooth, pbr where one is of kind 3, the light header and buffers where one is of kind 4.  The counts
// alone choose the kernel.
bool objects_scene(int level, const ObjectArgs& o, Scene& s) {
    const auto [objects, n_objects, obj_nrm, n_scene_tri, pbr, lights, light_tris, light_cdf, obj_col, obj_uv, tex, texels, n_texels, media] = o;
    const unsigned accept = (level >= 2 ? kAcceptSmooth : 0u) | (level >= 3 ? kAcceptPbr : 0u) | (level >= 4 ? kAcceptLight : 0u) |
                            (level >= 5 ? kAcceptRough : 0u) | (level >= 6 ? kAcceptColor : 0u) | (level >= 7 ? kAcceptTexture : 0u) |
                            (level >= 8 ? kAcceptMedium : 0u) | (level >= 9 ? kAcceptPhoto : 0u);
    ObjCounts n;
    if (!scene_table(objects, n_objects, accept, obj_nrm, n_scene_tri, pbr, s.ot, n) || (n.pbr > 0 && !pbr) || (n.color > 0 && !obj_col) ||
        (n.light > 0 && !light_table(lights, &s.ot, light_tris, light_cdf, s.lt)) ||
        (n.tex > 0 && !textures_valid(objects, n_objects, obj_uv, tex, texels, n_texels)) ||
        (n.medium > 0 && !media_valid(objects, n_objects, media)))
        return false;
    // records without a coefficient anywhere are no medium: the table goes on without the flag, to the kernel it had without it
    if (n.medium > 0 && !media_any(objects, n_objects, media)) {
        for (int k = 0; k < n_objects; ++k) s.ot.o[k].kind &= ~MATPBR_PATH_OBJECT_MEDIUM;
        n.medium = 0;
    }
    s.media = n.medium > 0 ? media : nullptr;
    s.n_photo = n.photo;
    s.kernel = n.medium > 0 ? Kernel::MediumObjects : n.tex > 0 ? Kernel::TexObjects : n.color > 0 ? Kernel::ColorObjects : n.rough > 0 ? Kernel::RoughObjects : n.light > 0 ? Kernel::LightObjects : n.pbr > 0 ? Kernel::PbrObjects :
               n.smooth > 0 ? Kernel::SmoothObjects : n_objects > 0 ? Kernel::ObjTable : Kernel::NoObjects;
    s.obj_nrm = n.smooth > 0 ? obj_nrm : nullptr;
    s.n_scene_tri = (int32_t)n_scene_tri;
    s.pbr = n.pbr > 0 ? pbr : nullptr;
    s.obj_col = n.color > 0 ? obj_col : nullptr;
    if (n.tex > 0) {
        s.obj_uv = obj_uv;
        s.tex = tex;
        s.texels = static_cast<const float4*>(texels);
    }
    return true;
}
int render_objects(const Frame& f, int level, const ObjectArgs& o) {
    Scene s;
    return objects_scene(level, o, s) ? render_common(f, s) : MATPBR_PATH_ERR_INVALID_ARG;
}

// the outputs of a differential entry, and the photograph it may read: an entry leaves what it does not have null
struct DiffOut {
    float *fg, *delta, *alpha;
    uint32_t* rewalked;
    const float* photo = nullptr;
    float *through = nullptr, *base = nullptr;
};
// The five differential entries are this one function (the second table in DESIGN.md section 1.4, "The object entries"): fg, delta and
// alpha always, photo and through both or neither (`need_photo`: both), base where `need_base`, at least one object.  (photo, base)
// choose the table; it is launched with the medium records behind it where `objects_scene` left them, and, at level 9 where an object
// carries the photo flag, as the table of the kernel whose chain passes it.
int render_diff(const Frame& f, int level, const ObjectArgs& o, const DiffOut& d, bool need_photo, bool need_base) {
    PathArgs q{};
    Scene s;
    if (!d.fg || !d.delta || !d.alpha || (need_photo && !d.photo) || (d.photo == nullptr) != (d.through == nullptr) || (need_base && !d.base) ||
        o.n_objects <= 0 || !frame_args(f, q) || !objects_scene(level, o, s))
        return MATPBR_PATH_ERR_INVALID_ARG;
    auto launch_as = [&](const auto& table) {
        using Table = std::decay_t<decltype(table)>;
        if constexpr (DiffTraits<Table>::through)
            if (level >= 9 && s.n_photo > 0) {
                Reflect<Table> rt{};
                static_cast<Table&>(rt) = table;
                return launch_frame(f, q, rt);
            }
        return launch_frame(f, q, table);
    };
    auto launch = [&](auto table) {
        using Table = decltype(table);
        static_cast<TexObjects&>(table) = tex_objects(s);
        table.fg = d.fg; table.delta = d.delta; table.alpha = d.alpha; table.rewalked = d.rewalked;
        if constexpr (DiffTraits<Table>::through) { table.photo = d.photo; table.through = d.through; }
        if constexpr (DiffTraits<Table>::base) table.base = d.base;
        if (!s.media) return launch_as(table);
        MediumDiff<Table> mt{};
        static_cast<Table&>(mt) = table;
        media_into(s, mt);
        return launch_as(mt);
    };
    if (d.base) return d.photo ? launch(RatioThroughObjects{}) : launch(RatioObjects{});
    return d.photo ? launch(ThroughObjects{}) : launch(DiffObjects{});
}

// the arguments both feature entry points share, checked and packed: `q` arrives with the caller's pointers and sizes
bool features_args(const MatpbrPathObject* objects, int n_objects, long n_scene_tri, float fov_x_deg, FeatArgs& q, ObjTable& ot) {
    // an object of kind 3, 4 or 5 is valid here: the features read its kind and its flag, never its record or its light tables
    ObjCounts n;
    if (!q.nodes || !q.tris || !q.geom || !denoise_size_valid(q.H, q.W) || !fov_valid(fov_x_deg) ||
        !scene_table(objects, n_objects, kAcceptAll, q.obj_nrm, n_scene_tri, nullptr, ot, n))
        return false;
    q.n_scene_tri = (int32_t)n_scene_tri;
    const Camera c = camera(q.H, q.W, fov_x_deg);   // the render's
    q.f_pix = c.f_pix; q.cx = c.cx; q.cy = c.cy;
    q.f_ndc = c.f_ndc; q.aspect = c.aspect;
    q.rho_scale = (float)(2.0 * c.th / q.W);
    return true;
}

// the arguments both colour-guide entry points share, checked and packed: the table may hold every kind and both flags
// (`accept`: the tint guide's table may hold the texture flag as well; it returns the number of textured objects in *n_tex)
bool feature_colors_args(const MatpbrPathObject* objects, int n_objects, long n_scene_tri, float fov_x_deg, FeatColorArgs& q, ObjTable& ot,
                         unsigned accept = kAcceptAll | kAcceptColor, int* n_tex = nullptr) {
    ObjCounts n;
    if (!q.nodes || !q.tris || !q.out || !denoise_size_valid(q.H, q.W) || !fov_valid(fov_x_deg) ||
        !object_table(objects, n_objects, accept, nullptr, ot, &n) || !ranges_above(objects, n_objects, n_scene_tri) || (n.color > 0 && !q.obj_col))
        return false;
    q.n_scene_tri = (int32_t)n_scene_tri;
    const Camera c = camera(q.H, q.W, fov_x_deg);   // the render's
    q.f_pix = c.f_pix; q.cx = c.cx; q.cy = c.cy;
    if (n_tex) *n_tex = n.tex;
    return true;
}
// the tint guide's arguments: the colour guide's, and the textures checked and packed where an object carries the flag
bool feature_tints_args(const MatpbrPathObject* objects, int n_objects, long n_scene_tri, float fov_x_deg, const float* obj_uv,
                        const MatpbrPathObjectTex* tex, const void* texels, long n_texels, FeatColorArgs& q, ObjTable& ot, FeatTextures& tx) {
    int n_tex = 0;
    if (!feature_colors_args(objects, n_objects, n_scene_tri, fov_x_deg, q, ot, kAcceptAll | kAcceptColor | kAcceptTexture, &n_tex) ||
        (n_tex > 0 && !textures_valid(objects, n_objects, obj_uv, tex, texels, n_texels)))
        return false;
    tx = FeatTextures{};
    if (n_tex > 0) {
        tx.uv = obj_uv;
        tx.texels = static_cast<const float4*>(texels);
        for (int k = 0; k < n_objects; ++k)
            if (objects[k].kind & MATPBR_PATH_OBJECT_TEXTURED) tx.tex[k] = tex[k];
    }
    return true;
}

// the Frame of a render entry point, from the names every one of them gives its first 21 parameters
#define RENDER_FRAME Frame{nodes, tris, a, r, m, H, W, fov_x_deg, env, row_cdf, col_cdf, env_pdf, He, We, spp, max_depth, seed, spp_per_launch, out, rays, stream}
// the ObjectArgs of an entry point from level 7 up, from the names every one of them gives the thirteen; `media` is the entry's to add
#define OBJECT_ARGS ObjectArgs{objects, n_objects, obj_nrm, n_scene_tri, pbr, lights, light_tris, light_cdf, obj_col, obj_uv, tex, texels, n_texels}

}  // namespace

extern "C" {

int matpbr_path_version(void) { return MATPBR_PATH_VERSION; }

const char* matpbr_path_strerror(int code) {
    switch (code) {
        case MATPBR_PATH_OK: return "ok";
        case MATPBR_PATH_ERR_INVALID_ARG: return "invalid argument (null pointer, non-positive size, index out of range, max_depth outside 1..16, "
                                                  "a workspace too small, an envmap of more than 1024 texels with d_env, a bad object table, a smooth object without corner normals, a coloured object without corner colours, a textured object without coordinates, texels or a valid record, or a bad transparency edit)";
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
    const float pad = (float)(1e-6 * mesh_scale(vert, n_vert));
    Builder bld;
    bld.nodes = static_cast<BNode*>(nodes);
    bld.max_nodes = max_nodes;
    builder_load(bld, vert, tri, 0, N, pad);
    if (!bld.build(N)) return MATPBR_PATH_ERR_CAPACITY;
    float4* T = static_cast<float4*>(tris);
    for (int k = 0; k < N; ++k) tri_record(vert, tri, bld.idx[k], n_scene_tri, T + 3 * k);
    *n_nodes = bld.n_nodes;
    *depth = bld.depth;
    *n_leaves = bld.n_leaves;
    return MATPBR_PATH_OK;
}

// ---- moving inserted objects ("Moving inserted objects") ----------------------------------------------------
int matpbr_path_bvh_build_grafted(const double* vert, long n_vert, long n_scene_vert, const int32_t* tri, long n_tri, long n_scene_tri, double reach,
                                  void* nodes, long max_nodes, void* tris, void* rest_tris, int32_t* node_level, long* n_nodes, int* depth, long* n_leaves,
                                  long* first_object_node, int* object_depth, float* pad) {
    if (!vert || !tri || !nodes || !tris || !rest_tris || !node_level || !n_nodes || !depth || !n_leaves || !first_object_node || !object_depth ||
        !pad || n_vert <= 0 || n_scene_vert < 1 || n_scene_vert > n_vert || n_tri < 2 || n_tri > INT32_MAX / 3 || n_scene_tri < 1 || n_scene_tri >= n_tri || !(reach >= 0.0) || !std::isfinite(reach))
        return MATPBR_PATH_ERR_INVALID_ARG;
    const long n_object_tri = n_tri - n_scene_tri;
    if (max_nodes < 1 + std::max(1L, n_scene_tri) + std::max(1L, n_object_tri)) return MATPBR_PATH_ERR_CAPACITY;
    for (long k = 0; k < 3 * n_tri; ++k)
        if (tri[k] < 0 || tri[k] >= n_vert) return MATPBR_PATH_ERR_INVALID_ARG;
    // the scene side is padded as matpbr_path_bvh_build pads the scene alone: by the scale of the scene's own vertices, the first
    // n_scene_vert of the merged mesh, which are all a scene triangle may name; the object side by the scale of everything, every
    // announced pose included
    for (long k = 0; k < 3 * n_scene_tri; ++k)
        if (tri[k] >= n_scene_vert) return MATPBR_PATH_ERR_INVALID_ARG;
    const float scene_pad = (float)(1e-6 * mesh_scale(vert, n_scene_vert));
    *pad = (float)(1e-6 * std::max(mesh_scale(vert, n_vert), reach));
    BNode* out = static_cast<BNode*>(nodes);
    float4 *T = static_cast<float4*>(tris), *rest = static_cast<float4*>(rest_tris);
    std::memset(&out[0], 0, sizeof(BNode));
    long used = 1, leaves = 0;
    int deepest = 1;
    // one side: a sub-build capped one level below the whole tree's cap, renumbered behind node 0; slot `slot` of node 0 is its root, or
    // its leaf when it holds kLeafMax triangles or fewer
    auto side = [&](int slot, long first, long count, float side_pad, std::vector<int32_t>* levels, int* side_depth) -> bool {
        std::vector<BNode> sub((size_t)std::max(1L, count));
        Builder bld;
        bld.nodes = sub.data();
        bld.max_nodes = (long)sub.size();
        bld.level_cap = kMaxBvhDepth - 1;
        bld.levels = levels;
        builder_load(bld, vert, tri, first, (int)count, side_pad);
        if (!bld.build((int)count)) return false;
        for (long k = 0; k < count; ++k) tri_record(vert, tri, first + bld.idx[k], n_scene_tri, T + 3 * (first + k));
        BNode& root = out[0];
        if (count <= kLeafMax) {   // the sub-build's root holds the one leaf in its slot 0
            for (int c = 0; c < 6; ++c) root.b[6 * slot + c] = sub[0].b[c];
            root.child[slot] = (int32_t)first;
            root.count[slot] = (int32_t)count;
            leaves += 1;
            *side_depth = 1;
            return true;
        }
        const long base = used;
        for (long q = 0; q < bld.n_nodes; ++q) {
            BNode nd = sub[q];
            for (int s = 0; s < 2; ++s) nd.child[s] += (int32_t)(nd.count[s] < 0 ? base : first);
            out[base + q] = nd;
        }
        float b[6];
        union_box(sub[0], b);
        for (int c = 0; c < 6; ++c) root.b[6 * slot + c] = b[c];
        root.child[slot] = (int32_t)base;
        root.count[slot] = -1;
        used += bld.n_nodes;
        leaves += bld.n_leaves;
        *side_depth = bld.depth + 1;
        return true;
    };
    int scene_depth = 1;
    std::vector<int32_t> levels;
    if (!side(0, 0, n_scene_tri, scene_pad, nullptr, &scene_depth)) return MATPBR_PATH_ERR_CAPACITY;
    *first_object_node = used;
    if (!side(1, n_scene_tri, n_object_tri, *pad, &levels, object_depth)) return MATPBR_PATH_ERR_CAPACITY;
    const long n_object_nodes = used - *first_object_node;
    if (n_object_nodes > 0) {
        node_level[0] = 1;   // the object subtree's root; the builder recorded its other nodes' levels below it
        for (long q = 1; q < n_object_nodes; ++q) node_level[q] = levels[q - 1] + 1;
    }
    deepest = std::max(scene_depth, *object_depth);
    std::memcpy(rest, T + 3 * n_scene_tri, (size_t)n_object_tri * 3 * sizeof(float4));
    // the object boxes are the refit rule's: the build ends with the refit of the rest pose, so that a move by the identity reproduces it
    for (long i = 0; i < n_object_nodes; ++i) refit_leaf_slots(out, *first_object_node + i, T, *pad);
    for (int level = *object_depth - 1; level >= 1; --level)
        for (long i = 0; i < n_object_nodes; ++i)
            if (node_level[i] == level) refit_inner_slots(out, *first_object_node + i);
    refit_graft_slot(out, T, *pad);
    *n_nodes = used;
    *depth = deepest;
    *n_leaves = leaves;
    return MATPBR_PATH_OK;
}

int matpbr_path_xform_check_host(const MatpbrPathXform* xform, int n_objects) {
    if (!xform || n_objects < 1 || n_objects > MATPBR_PATH_MAX_OBJECTS) return MATPBR_PATH_ERR_INVALID_ARG;
    for (int k = 0; k < n_objects; ++k)
        if (!xform_ok(xform[k])) return MATPBR_PATH_ERR_INVALID_ARG;
    return MATPBR_PATH_OK;
}

namespace {
bool move_args_valid(const void* nodes, const void* tris, const void* rest_tris, long n_scene_tri, long n_object_tri, long first_object_node,
                     long n_object_nodes, const int32_t* node_level, int object_depth, float pad, const void* rest_light_tris, const void* light_tris,
                     long n_light_tri) {
    return nodes && tris && rest_tris && !((uintptr_t)nodes & 15) && !((uintptr_t)tris & 15) && !((uintptr_t)rest_tris & 15) && n_scene_tri >= 0 &&
           n_object_tri >= 1 && n_scene_tri + n_object_tri <= INT32_MAX / 3 && first_object_node >= 1 && n_object_nodes >= 0 &&
           first_object_node + n_object_nodes <= INT32_MAX && (n_object_nodes == 0 || node_level) && object_depth >= 1 &&
           object_depth <= kMaxBvhDepth && pad >= 0.0f && std::isfinite(pad) && n_light_tri >= 0 && n_light_tri <= INT32_MAX / 3 &&
           (n_light_tri == 0 || (rest_light_tris && light_tris && !((uintptr_t)rest_light_tris & 15) && !((uintptr_t)light_tris & 15)));
}
}  // namespace

int matpbr_path_objects_move(void* nodes, void* tris, const void* rest_tris, long n_scene_tri, long n_object_tri, long first_object_node,
                             long n_object_nodes, const int32_t* node_level, int object_depth, const MatpbrPathObject* objects, int n_objects,
                             const MatpbrPathXform* xform, float pad, const float* rest_nrm, float* obj_nrm, const void* rest_light_tris,
                             void* light_tris, long n_light_tri, const MatpbrPathLights* lights, void* stream) {
    MoveTable mt;
    if (!move_args_valid(nodes, tris, rest_tris, n_scene_tri, n_object_tri, first_object_node, n_object_nodes, node_level, object_depth, pad,
                         rest_light_tris, light_tris, n_light_tri) ||
        !move_table(objects, n_objects, xform, n_scene_tri, n_object_tri, rest_nrm, obj_nrm, lights, n_light_tri, mt))
        return MATPBR_PATH_ERR_INVALID_ARG;
    const long n = n_object_tri + n_light_tri;
    hipLaunchKernelGGL(objects_move_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, mt,
                       static_cast<const float4*>(rest_tris), static_cast<float4*>(tris), n_scene_tri, n_object_tri, rest_nrm, obj_nrm,
                       static_cast<const float4*>(rest_light_tris), static_cast<float4*>(light_tris), n_light_tri);
    if (hipGetLastError() != hipSuccess) return MATPBR_PATH_ERR_LAUNCH;
    hipLaunchKernelGGL(objects_refit_kernel, dim3(1), dim3(kRefitBlock), 0, (hipStream_t)stream, static_cast<BNode*>(nodes),
                       static_cast<const float4*>(tris), first_object_node, n_object_nodes, node_level, object_depth, pad);
    return hipGetLastError() == hipSuccess ? MATPBR_PATH_OK : MATPBR_PATH_ERR_LAUNCH;
}

int matpbr_path_objects_move_host(void* nodes, void* tris, const void* rest_tris, long n_scene_tri, long n_object_tri, long first_object_node,
                                  long n_object_nodes, const int32_t* node_level, int object_depth, const MatpbrPathObject* objects, int n_objects,
                                  const MatpbrPathXform* xform, float pad, const float* rest_nrm, float* obj_nrm, const void* rest_light_tris,
                                  void* light_tris, long n_light_tri, const MatpbrPathLights* lights) {
    MoveTable mt;
    if (!move_args_valid(nodes, tris, rest_tris, n_scene_tri, n_object_tri, first_object_node, n_object_nodes, node_level, object_depth, pad,
                         rest_light_tris, light_tris, n_light_tri) ||
        !move_table(objects, n_objects, xform, n_scene_tri, n_object_tri, rest_nrm, obj_nrm, lights, n_light_tri, mt))
        return MATPBR_PATH_ERR_INVALID_ARG;
    BNode* nd = static_cast<BNode*>(nodes);
    // the CPU walks the caller's nodes: every child an object node names must be an object node or an object triangle range
    if (nd[0].count[1] < 0 ? nd[0].child[1] != first_object_node : (nd[0].child[1] < n_scene_tri || (long)nd[0].child[1] + nd[0].count[1] > n_scene_tri + n_object_tri))
        return MATPBR_PATH_ERR_INVALID_ARG;
    for (long i = 0; i < n_object_nodes; ++i)
        for (int s = 0; s < 2; ++s) {
            const BNode& q = nd[first_object_node + i];
            if (q.count[s] < 0 ? (q.child[s] <= first_object_node + i || q.child[s] >= first_object_node + n_object_nodes)
                               : (q.child[s] < n_scene_tri || (long)q.child[s] + q.count[s] > n_scene_tri + n_object_tri))
                return MATPBR_PATH_ERR_INVALID_ARG;
        }
    objects_move_host(mt, nd, static_cast<float4*>(tris), static_cast<const float4*>(rest_tris), n_scene_tri, n_object_tri, first_object_node,
                      n_object_nodes, node_level, object_depth, pad, rest_nrm, obj_nrm, static_cast<const float4*>(rest_light_tris),
                      static_cast<float4*>(light_tris), n_light_tri);
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

int matpbr_path_trace_scene_host(const void* nodes, const void* tris, const float* o, const float* d, long N, float tmin, float tmax,
                                 float* t_hit, int32_t* tri_hit, long n_scene_tri, int any) {
    if (!nodes || !tris || !o || !d || !t_hit || !tri_hit || N < 0 || n_scene_tri < 0 || (any != 0 && any != 1)) return MATPBR_PATH_ERR_INVALID_ARG;
    const float4 *Nd = static_cast<const float4*>(nodes), *T = static_cast<const float4*>(tris);
    const int id_limit = (int)std::min(n_scene_tri, (long)INT32_MAX);
    for (long k = 0; k < N; ++k) {
        HostStack stk;
        float t = tmax;
        const int h = any ? trace<true, true>(Nd, T, o + 3 * k, d + 3 * k, tmin, t, stk, id_limit)
                          : trace<false, true>(Nd, T, o + 3 * k, d + 3 * k, tmin, t, stk, id_limit);
        t_hit[k] = t;
        tri_hit[k] = h >= 0 ? tri_id(T[3 * h]) : -1;
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

int matpbr_path_render_objects(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                               float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                               int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream,
                               const MatpbrPathObject* objects, int n_objects) {
    return render_objects(RENDER_FRAME, 1, {objects, n_objects});
}

int matpbr_path_render_objects_normals(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                       float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                       int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream,
                                       const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri) {
    return render_objects(RENDER_FRAME, 2, {objects, n_objects, obj_nrm, n_scene_tri});
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
    return render_objects(RENDER_FRAME, 3, {objects, n_objects, obj_nrm, n_scene_tri, pbr});
}

int matpbr_path_light_tables(const double* vert, long n_vert, const int32_t* tri, long n_tri, const MatpbrPathObject* objects, int n_objects,
                             const MatpbrPathObjectPbr* pbr, MatpbrPathLights* lights, float* light_tris, float* light_cdf, long capacity,
                             long* n_light_tri) {
    ObjTable ot{};
    if (!vert || !tri || !lights || !n_light_tri || n_vert <= 0 || n_tri < 0 || n_tri > INT32_MAX / 3 || (light_tris && (!light_cdf || capacity < 0)) ||
        !object_table(objects, n_objects, kAcceptAll, pbr, ot))
        return MATPBR_PATH_ERR_INVALID_ARG;
    return light_tables_build(vert, n_vert, tri, n_tri, ot, lights, light_tris, light_cdf, capacity, n_light_tri);
}

int matpbr_path_render_objects_lights(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                      float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                      int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream,
                                      const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                      const MatpbrPathObjectPbr* pbr, const MatpbrPathLights* lights, const void* light_tris,
                                      const float* light_cdf) {
    return render_objects(RENDER_FRAME, 4, {objects, n_objects, obj_nrm, n_scene_tri, pbr, lights, light_tris, light_cdf});
}

int matpbr_path_light_sample_host(const MatpbrPathLights* lights, const void* light_tris, const float* light_cdf, long n_light_tri, int have_env,
                                  const float* po, const float* u, long N, int32_t* emitter, float* u_re, int32_t* record, float* y, float* wl,
                                  float* dist, float* pdf) {
    LightTable lt;
    long n_rec = 0;
    if (!light_cdf || !po || !u || !emitter || !u_re || !record || !y || !wl || !dist || !pdf || N < 0 || (have_env != 0 && have_env != 1) ||
        !light_table(lights, nullptr, light_tris, light_cdf, lt, &n_rec) || n_rec != n_light_tri)
        return MATPBR_PATH_ERR_INVALID_ARG;
    const int n_e = have_env + lt.n;
    for (long k = 0; k < N; ++k) {
        emitter[k] = emitter_choose(u[4 * k], n_e, u_re[k]);
        record[k] = -1;
        y[3 * k] = y[3 * k + 1] = y[3 * k + 2] = wl[3 * k] = wl[3 * k + 1] = wl[3 * k + 2] = 0.0f;
        dist[k] = pdf[k] = 0.0f;
        if (have_env && emitter[k] == 0) continue;
        record[k] = light_sample(lt, emitter[k] - have_env, u_re[k], u[4 * k + 1], u[4 * k + 2], po + 3 * k, (float)n_e, y + 3 * k, wl + 3 * k,
                                 dist[k], pdf[k]);
    }
    return MATPBR_PATH_OK;
}

int matpbr_path_light_pdf_host(const MatpbrPathLights* lights, const void* light_tris, long n_light_tri, int have_env, const int32_t* light,
                               const int32_t* record, const float* o, const float* d, long N, float* t, float* pdf) {
    LightTable lt;
    long n_rec = 0;
    if (!light || !record || !o || !d || !t || !pdf || N < 0 || (have_env != 0 && have_env != 1) ||
        !light_table(lights, nullptr, light_tris, nullptr, lt, &n_rec) || n_rec != n_light_tri)
        return MATPBR_PATH_ERR_INVALID_ARG;
    const float n_e = (float)(have_env + lt.n);
    for (long k = 0; k < N; ++k) {
        const int l = light[k], rec = record[k];
        if (l < 0 || l >= lt.n || rec < lt.first[l] || rec - lt.first[l] >= lt.n_tri[l]) return MATPBR_PATH_ERR_INVALID_ARG;
        t[k] = tri_t(lt.tri, rec, o + 3 * k, d + 3 * k);
        const float4 B = lt.tri[3 * rec + 1], C = lt.tri[3 * rec + 2];
        const float e1[3] = {B.x, B.y, B.z}, e2[3] = {C.x, C.y, C.z};
        float n[3];
        cross3(e1, e2, n);
        const float cos_o = -dot3h(n, d + 3 * k) / sqrtf(dot3h(n, n));
        pdf[k] = t[k] > 0.0f && t[k] < FLT_MAX && cos_o > 0.0f ? light_hit_pdf(t[k], lt.area[l], cos_o, n_e) : 0.0f;
    }
    return MATPBR_PATH_OK;
}

int matpbr_path_render_objects_rough(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                     float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                     int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream,
                                     const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                     const MatpbrPathObjectPbr* pbr, const MatpbrPathLights* lights, const void* light_tris,
                                     const float* light_cdf) {
    return render_objects(RENDER_FRAME, 5, {objects, n_objects, obj_nrm, n_scene_tri, pbr, lights, light_tris, light_cdf});
}

int matpbr_path_render_objects_colors(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                      float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                      int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream,
                                      const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                      const MatpbrPathObjectPbr* pbr, const MatpbrPathLights* lights, const void* light_tris,
                                      const float* light_cdf, const float* obj_col) {
    return render_objects(RENDER_FRAME, 6, {objects, n_objects, obj_nrm, n_scene_tri, pbr, lights, light_tris, light_cdf, obj_col});
}

int matpbr_path_object_color_host(const float* tri, const float* col, const float* o, const float* d, long N, float* u, float* v, float* c) {
    if (!tri || !col || !o || !d || !u || !v || !c || N < 0) return MATPBR_PATH_ERR_INVALID_ARG;
    for (long k = 0; k < N; ++k) {
        const float *v0 = tri + 9 * k, *e1 = v0 + 3, *e2 = v0 + 6;
        tri_uv(v0, e1, e2, o + 3 * k, d + 3 * k, u[k], v[k]);
        object_color(col + 9 * k, u[k], v[k], c + 3 * k);
    }
    return MATPBR_PATH_OK;
}

int matpbr_path_render_objects_textures(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                        float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                        int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream,
                                        const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                        const MatpbrPathObjectPbr* pbr, const MatpbrPathLights* lights, const void* light_tris,
                                        const float* light_cdf, const float* obj_col, const float* obj_uv, const MatpbrPathObjectTex* tex,
                                        const void* texels, long n_texels) {
    return render_objects(RENDER_FRAME, 7, OBJECT_ARGS);
}

int matpbr_path_render_objects_diff(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                    float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                    int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, uint32_t* rays, void* stream,
                                    const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                    const MatpbrPathObjectPbr* pbr, const MatpbrPathLights* lights, const void* light_tris,
                                    const float* light_cdf, const float* obj_col, const float* obj_uv, const MatpbrPathObjectTex* tex,
                                    const void* texels, long n_texels, float* fg, float* delta, float* alpha, uint32_t* rewalked) {
    float* const out = nullptr;   // the sums go to the table's buffers
    return render_diff(RENDER_FRAME, 7, OBJECT_ARGS, {fg, delta, alpha, rewalked}, false, false);
}

int matpbr_path_render_objects_through(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                       float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                       int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, uint32_t* rays, void* stream,
                                       const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                       const MatpbrPathObjectPbr* pbr, const MatpbrPathLights* lights, const void* light_tris,
                                       const float* light_cdf, const float* obj_col, const float* obj_uv, const MatpbrPathObjectTex* tex,
                                       const void* texels, long n_texels, float* fg, float* delta, float* alpha, uint32_t* rewalked,
                                       const float* photo, float* through) {
    float* const out = nullptr;   // the sums go to the table's buffers
    return render_diff(RENDER_FRAME, 7, OBJECT_ARGS, {fg, delta, alpha, rewalked, photo, through}, true, false);
}

int matpbr_path_render_objects_ratio(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                     float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                     int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, uint32_t* rays, void* stream,
                                     const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                     const MatpbrPathObjectPbr* pbr, const MatpbrPathLights* lights, const void* light_tris,
                                     const float* light_cdf, const float* obj_col, const float* obj_uv, const MatpbrPathObjectTex* tex,
                                     const void* texels, long n_texels, float* fg, float* delta, float* alpha, uint32_t* rewalked,
                                     const float* photo, float* through, float* base) {
    float* const out = nullptr;   // the sums go to the table's buffers
    return render_diff(RENDER_FRAME, 7, OBJECT_ARGS, {fg, delta, alpha, rewalked, photo, through, base}, false, true);
}

int matpbr_path_render_objects_media(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                     float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                     int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream,
                                     const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                     const MatpbrPathObjectPbr* pbr, const MatpbrPathLights* lights, const void* light_tris,
                                     const float* light_cdf, const float* obj_col, const float* obj_uv, const MatpbrPathObjectTex* tex,
                                     const void* texels, long n_texels, const MatpbrPathObjectMedium* media) {
    ObjectArgs o = OBJECT_ARGS;
    o.media = media;
    return render_objects(RENDER_FRAME, 8, o);
}

int matpbr_path_render_objects_diff_media(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                          float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                          int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, uint32_t* rays, void* stream,
                                          const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                          const MatpbrPathObjectPbr* pbr, const MatpbrPathLights* lights, const void* light_tris,
                                          const float* light_cdf, const float* obj_col, const float* obj_uv, const MatpbrPathObjectTex* tex,
                                          const void* texels, long n_texels, float* fg, float* delta, float* alpha, uint32_t* rewalked,
                                          const float* photo, float* through, float* base, const MatpbrPathObjectMedium* media) {
    float* const out = nullptr;   // the sums go to the table's buffers
    ObjectArgs o = OBJECT_ARGS;
    o.media = media;
    return render_diff(RENDER_FRAME, 8, o, {fg, delta, alpha, rewalked, photo, through, base}, false, false);
}

int matpbr_path_render_objects_reflect(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                       float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                       int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, uint32_t* rays, void* stream,
                                       const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                       const MatpbrPathObjectPbr* pbr, const MatpbrPathLights* lights, const void* light_tris,
                                       const float* light_cdf, const float* obj_col, const float* obj_uv, const MatpbrPathObjectTex* tex,
                                       const void* texels, long n_texels, float* fg, float* delta, float* alpha, uint32_t* rewalked,
                                       const float* photo, float* through, float* base, const MatpbrPathObjectMedium* media) {
    float* const out = nullptr;   // the sums go to the table's buffers
    ObjectArgs o = OBJECT_ARGS;
    o.media = media;
    return render_diff(RENDER_FRAME, 9, o, {fg, delta, alpha, rewalked, photo, through, base}, true, false);
}

int matpbr_path_medium_segment_host(const MatpbrPathObjectMedium* medium, const float* t, const float* u9, long N, int32_t* scattered,
                                    float* dist, float* weight) {
    if (!medium || !t || !u9 || !scattered || !dist || !weight || N < 0 || !medium_valid(*medium)) return MATPBR_PATH_ERR_INVALID_ARG;
    for (long k = 0; k < N; ++k) scattered[k] = medium_segment(*medium, t[k], u9[k], dist[k], weight + 3 * k) ? 1 : 0;
    return MATPBR_PATH_OK;
}

int matpbr_path_phase_sample_host(float g, const float* d, const float* u, long N, float* wi) {
    if (!d || !u || !wi || N < 0 || !(fabsf(g) <= 0.99f)) return MATPBR_PATH_ERR_INVALID_ARG;
    for (long k = 0; k < N; ++k) phase_sample(g, d + 3 * k, u[2 * k], u[2 * k + 1], wi + 3 * k);
    return MATPBR_PATH_OK;
}

// the camera chain of both CPU entries below, one body: `reflect` admits the photo flag, and a vertex on a flagged object then keeps
// the chain as the kernels of Reflect<...> keep it (its BSDF sample by dims 6, 7, 8; no emitter sample changes the chain)
static int chain_host(const void* nodes, const void* tris, int H, int W, float fov_x_deg, int max_depth, const MatpbrPathObject* objects,
                      int n_objects, const float* obj_nrm, long n_scene_tri, const MatpbrPathObjectPbr* pbr, bool reflect, const int32_t* pixel,
                      const uint32_t* seed, const int32_t* sample, long N, int32_t* depth, int32_t* texel, float* thr, float* o, float* d) {
    ObjTable ot{};
    ObjCounts cnt;
    if (!nodes || !tris || !pixel || !seed || !sample || !depth || !texel || !thr || !o || !d || N < 0 || H <= 0 || W <= 0 ||
        !fov_valid(fov_x_deg) || max_depth < 1 || max_depth > MATPBR_PATH_MAX_MAX_DEPTH || n_objects <= 0 ||
        !scene_table(objects, n_objects, kAcceptAll | kAcceptColor | kAcceptTexture | (reflect ? kAcceptPhoto : 0u), obj_nrm, n_scene_tri, pbr, ot, cnt))
        return MATPBR_PATH_ERR_INVALID_ARG;
    for (int k = 0; k < n_objects; ++k) {   // a flagged object: its record where it is of kind 3; no colour or image multiplies its weight here
        if (!(objects[k].kind & MATPBR_PATH_OBJECT_PHOTO)) continue;
        if (objects[k].kind & (MATPBR_PATH_OBJECT_COLORED | MATPBR_PATH_OBJECT_TEXTURED)) return MATPBR_PATH_ERR_INVALID_ARG;
        if ((objects[k].kind & 0xff) == MATPBR_PATH_BSDF_PBR && !pbr) return MATPBR_PATH_ERR_INVALID_ARG;
    }
    for (long l = 0; l < N; ++l)
        if (pixel[l] < 0 || pixel[l] >= (long)H * W || sample[l] < 0) return MATPBR_PATH_ERR_INVALID_ARG;
    const float4 *Nd = static_cast<const float4*>(nodes), *T = static_cast<const float4*>(tris);
    const Camera cam = camera(H, W, fov_x_deg);
    const uint32_t flags = MATPBR_PATH_OBJECT_SMOOTH | MATPBR_PATH_OBJECT_COLORED | MATPBR_PATH_OBJECT_TEXTURED;
    for (long l = 0; l < N; ++l) {
        const int i = pixel[l] / W, j = pixel[l] % W;
        const uint32_t base = pcg_hash(pcg_hash(pcg_hash(seed[l]) + (uint32_t)pixel[l]) + (uint32_t)sample[l]);
        const float x = (float)j - 0.5f + rng_u(base, 0, 0), y = (float)i - 0.5f + rng_u(base, 0, 1);
        float ro[3] = {0.0f, 0.0f, 0.0f}, rd[3] = {(x - cam.cx) / cam.f_pix, -(y - cam.cy) / cam.f_pix, -1.0f};
        {
            const float il = 1.0f / sqrtf(dot3h(rd, rd));
            for (int c = 0; c < 3; ++c) rd[c] *= il;
        }
        float w[3] = {1.0f, 1.0f, 1.0f};
        int found = -1;
        long tq = -1;
        for (int dp = 0;; ++dp) {
            HostStack stk;
            float t = FLT_MAX;
            const int k = trace<false>(Nd, T, ro, rd, 0.0f, t, stk);
            if (k < 0) break;   // the envmap
            const int id = tri_id(T[3 * k]);
            const float4 A = T[3 * k], B = T[3 * k + 1], C = T[3 * k + 2];
            const float v0[3] = {A.x, A.y, A.z}, e1[3] = {B.x, B.y, B.z}, e2[3] = {C.x, C.y, C.z};
            float n[3];
            cross3(e1, e2, n);
            {
                const float il = 1.0f / sqrtf(dot3h(n, n));
                for (int c = 0; c < 3; ++c) n[c] *= il;
            }
            const float wo[3] = {-rd[0], -rd[1], -rd[2]};
            float p[3];
            for (int c = 0; c < 3; ++c) p[c] = fmaf(t, rd[c], ro[c]);
            if (id < n_scene_tri) {   // the depth mesh: a landing on its front at depth >= 1, else the chain's end
                if (dp >= 1 && dot3h(n, wo) > 0.0f) {
                    found = dp;
                    tq = screen_texel(p, cam.f_ndc, cam.aspect, H, W);
                }
                break;
            }
            int kind = 0, obj = -1;
            float op[3] = {0.0f, 0.0f, 0.0f};
            object_match(ot, id, [&](int k, const MatpbrPathObject& ob) {
                kind = ob.kind;
                obj = k;
                op[0] = ob.p[0]; op[1] = ob.p[1]; op[2] = ob.p[2];
            });
            const bool smooth = (kind & MATPBR_PATH_OBJECT_SMOOTH) != 0;
            const bool photo_obj = (kind & MATPBR_PATH_OBJECT_PHOTO) != 0;   // set only where `reflect` admitted it
            kind &= ~(int)(flags | MATPBR_PATH_OBJECT_PHOTO);
            // another kind without the flag, or still on the chain at max_depth
            if (!(kind == MATPBR_PATH_BSDF_DIELECTRIC || photo_obj) || dp + 1 >= max_depth) break;
            // a flagged object of kind 2 or 3 seen from behind ends the path, as every one-sided vertex does
            if (kind != MATPBR_PATH_BSDF_DIELECTRIC && kind != MATPBR_PATH_BSDF_ROUGH_DIELECTRIC && !(dot3h(n, wo) > 0.0f)) break;
            float wi[3], wgt[3], pdf_s, ns[3] = {n[0], n[1], n[2]};
            int fl;
            if (smooth) {
                float su, sv;
                tri_uv(v0, e1, e2, ro, rd, su, sv);
                smooth_normal(obj_nrm + 9 * (long)(id - n_scene_tri), su, sv, n, ns);
                smooth_side(n, wo, ns);
            }
            const float eps = spawn_eps(p);
            float side = eps;
            if (kind == MATPBR_PATH_BSDF_PBR) {   // the depth mesh's sampler on the record's constants; the ray leaves on the face's front
                path_sample_host(rng_u(base, dp, 6), rng_u(base, dp, 7), rng_u(base, dp, 8), wo, ns, pbr[obj].a, pbr[obj].r, pbr[obj].m, wi, wgt, pdf_s);
                if (!(dot3h(n, wi) > 0.0f)) break;   // a reflection that leaves below the object's face carries nothing
            } else {
                if (kind == MATPBR_PATH_BSDF_ROUGH_DIELECTRIC)
                    rough_sample(op, n, ns, wo, rng_u(base, dp, 6), rng_u(base, dp, 7), rng_u(base, dp, 8), wi, wgt, pdf_s, fl);
                else if (smooth)
                    object_sample_shading(kind, op, n, ns, wo, rng_u(base, dp, 6), rng_u(base, dp, 7), rng_u(base, dp, 8), wi, wgt, pdf_s, fl);
                else
                    object_sample(kind, op, n, wo, rng_u(base, dp, 6), rng_u(base, dp, 7), rng_u(base, dp, 8), wi, wgt, pdf_s, fl);
                side = dot3h(n, wi) > 0.0f ? eps : -eps;   // spawn on the side the new ray leaves on
            }
            for (int c = 0; c < 3; ++c) {
                w[c] *= wgt[c];
                ro[c] = fmaf(side, n[c], p[c]);
                rd[c] = wi[c];
            }
            if (!(w[0] > 0.0f || w[1] > 0.0f || w[2] > 0.0f)) break;
        }
        depth[l] = found;
        texel[l] = (int32_t)tq;
        for (int c = 0; c < 3; ++c) {
            thr[3 * l + c] = found >= 0 ? w[c] : 0.0f;
            o[3 * l + c] = found >= 0 ? ro[c] : 0.0f;
            d[3 * l + c] = found >= 0 ? rd[c] : 0.0f;
        }
    }
    return MATPBR_PATH_OK;
}

int matpbr_path_through_chain_host(const void* nodes, const void* tris, int H, int W, float fov_x_deg, int max_depth,
                                   const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                   const int32_t* pixel, const uint32_t* seed, const int32_t* sample, long N, int32_t* depth, int32_t* texel,
                                   float* thr, float* o, float* d) {
    return chain_host(nodes, tris, H, W, fov_x_deg, max_depth, objects, n_objects, obj_nrm, n_scene_tri, nullptr, false, pixel, seed, sample, N, depth,
                      texel, thr, o, d);
}

int matpbr_path_reflect_chain_host(const void* nodes, const void* tris, int H, int W, float fov_x_deg, int max_depth,
                                   const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                   const MatpbrPathObjectPbr* pbr, const int32_t* pixel, const uint32_t* seed, const int32_t* sample, long N,
                                   int32_t* depth, int32_t* texel, float* thr, float* o, float* d) {
    return chain_host(nodes, tris, H, W, fov_x_deg, max_depth, objects, n_objects, obj_nrm, n_scene_tri, pbr, true, pixel, seed, sample, N, depth,
                      texel, thr, o, d);
}

int matpbr_path_composite(const float* fg_sum, const float* delta_sum, const float* alpha_sum, const float* photo, int H, int W, float scale,
                          float* out, void* stream) {
    if (!composite_args_valid(fg_sum, delta_sum, alpha_sum, photo, H, W, scale, out)) return MATPBR_PATH_ERR_INVALID_ARG;
    const long P = (long)H * W;
    hipLaunchKernelGGL(composite_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, fg_sum, delta_sum, alpha_sum, photo, P,
                       scale, out);
    return hipGetLastError() == hipSuccess ? MATPBR_PATH_OK : MATPBR_PATH_ERR_LAUNCH;
}

int matpbr_path_composite_host(const float* fg_sum, const float* delta_sum, const float* alpha_sum, const float* photo, int H, int W, float scale,
                               float* out) {
    if (!composite_args_valid(fg_sum, delta_sum, alpha_sum, photo, H, W, scale, out)) return MATPBR_PATH_ERR_INVALID_ARG;
    for (long p = 0; p < (long)H * W; ++p) composite_pixel(fg_sum, delta_sum, alpha_sum, photo, p, scale, out);
    return MATPBR_PATH_OK;
}

int matpbr_path_composite_ratio(const float* fg_sum, const float* delta_sum, const float* base_sum, const float* alpha_sum, const float* photo, int H,
                                int W, float scale, float* out, void* stream) {
    if (!base_sum || !composite_args_valid(fg_sum, delta_sum, alpha_sum, photo, H, W, scale, out)) return MATPBR_PATH_ERR_INVALID_ARG;
    const long P = (long)H * W;
    hipLaunchKernelGGL(composite_ratio_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, fg_sum, delta_sum, base_sum,
                       alpha_sum, photo, P, scale, out);
    return hipGetLastError() == hipSuccess ? MATPBR_PATH_OK : MATPBR_PATH_ERR_LAUNCH;
}

int matpbr_path_composite_ratio_host(const float* fg_sum, const float* delta_sum, const float* base_sum, const float* alpha_sum, const float* photo,
                                     int H, int W, float scale, float* out) {
    if (!base_sum || !composite_args_valid(fg_sum, delta_sum, alpha_sum, photo, H, W, scale, out)) return MATPBR_PATH_ERR_INVALID_ARG;
    for (long p = 0; p < (long)H * W; ++p) composite_ratio_pixel(fg_sum, delta_sum, base_sum, alpha_sum, photo, p, scale, out);
    return MATPBR_PATH_OK;
}

int matpbr_path_object_texture_host(const float* tri, const float* uv, const float* o, const float* d, long N, const MatpbrPathObjectTex* tex,
                                    const void* texels, long n_texels, float* u, float* v, float* st, float* base, float* orm) {
    if (!tri || !uv || !o || !d || !tex || !texels || ((uintptr_t)texels & 15) || !u || !v || !st || !base || !orm || N < 0 ||
        !tex_valid(*tex, true, n_texels))
        return MATPBR_PATH_ERR_INVALID_ARG;
    for (long k = 0; k < N; ++k) {
        const float *v0 = tri + 9 * k, *e1 = v0 + 3, *e2 = v0 + 6;
        tri_uv(v0, e1, e2, o + 3 * k, d + 3 * k, u[k], v[k]);
        object_st(uv + 6 * k, u[k], v[k], st[2 * k], st[2 * k + 1]);
        texture_fetch_record(*tex, static_cast<const float4*>(texels), st[2 * k], st[2 * k + 1], base + 3 * k, orm + 3 * k);
    }
    return MATPBR_PATH_OK;
}

// the object of the two CPU entry points below: kind 5, with or without the smooth flag (the caller passes both normals either way)
static bool rough_object(const MatpbrPathObject* ob) {
    return ob && (ob->kind & ~MATPBR_PATH_OBJECT_SMOOTH) == MATPBR_PATH_BSDF_ROUGH_DIELECTRIC && rough_valid(ob->p);
}

int matpbr_path_rough_sample_host(const MatpbrPathObject* object, const float* ng, const float* ns, const float* wo, const float* u, long N,
                                  float* wi, float* weight, float* pdf, int32_t* flags) {
    if (!rough_object(object) || !ng || !ns || !wo || !u || !wi || !weight || !pdf || !flags || N < 0) return MATPBR_PATH_ERR_INVALID_ARG;
    for (long k = 0; k < N; ++k) {
        int fl = 0;
        rough_sample(object->p, ng + 3 * k, ns + 3 * k, wo + 3 * k, u[3 * k], u[3 * k + 1], u[3 * k + 2], wi + 3 * k, weight + 3 * k, pdf[k], fl);
        flags[k] = fl;
    }
    return MATPBR_PATH_OK;
}

int matpbr_path_rough_eval_host(const MatpbrPathObject* object, const float* ng, const float* ns, const float* wo, const float* wl, long N,
                                float* f, float* pdf) {
    if (!rough_object(object) || !ng || !ns || !wo || !wl || !f || !pdf || N < 0) return MATPBR_PATH_ERR_INVALID_ARG;
    for (long k = 0; k < N; ++k) {
        rough_eval(object->p, ng + 3 * k, ns + 3 * k, wo + 3 * k, wl + 3 * k, f[3 * k], pdf[k]);
        f[3 * k + 1] = f[3 * k + 2] = f[3 * k];
    }
    return MATPBR_PATH_OK;
}

int matpbr_path_object_lookup_host(const MatpbrPathObject* objects, int n_objects, const MatpbrPathObjectPbr* pbr, const int32_t* ids, long N,
                                   int32_t* kind, float* a, float* r, float* m) {
    ObjTable ot{};
    ObjCounts n;
    if (!ids || !kind || !a || !r || !m || N < 0 || !object_table(objects, n_objects, kAcceptAll & ~kAcceptLight, pbr, ot, &n) || (n.pbr > 0 && !pbr))
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
    Scene s;
    s.kernel = Kernel::TransEdit;
    s.edit = TransEdit{mask, bg, edit->ior, edit->spec_trans, edit->refract_distance};
    return render_common(RENDER_FRAME, s);
}

int matpbr_path_render_normals(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                               float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                               int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream,
                               const float* nrm) {
    Scene s;
    s.kernel = nrm ? Kernel::ShadeNormals : Kernel::NoObjects;
    s.nrm = nrm;
    return render_common(RENDER_FRAME, s);
}

int matpbr_path_render_edit_diff(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                 float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                 int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, uint32_t* rays, void* stream,
                                 const float* a_e, const float* r_e, const float* m_e, const uint8_t* mask, const float* nrm, float* delta,
                                 float* base, uint32_t* rewalked) {
    float* const out = base;   // the radiance on the fitted maps is the render's own sum
    const Frame f = RENDER_FRAME;
    PathArgs q{};
    if (!a_e || !r_e || !m_e || !mask || !delta || !base || !frame_args(f, q)) return MATPBR_PATH_ERR_INVALID_ARG;
    auto launch = [&](auto base_table) {   // the edit's table over the render's own
        MapEdit<decltype(base_table)> t{};
        static_cast<decltype(base_table)&>(t) = base_table;
        t.a_e = a_e; t.r_e = r_e; t.m_e = m_e; t.mask = mask; t.delta = delta; t.rewalked = rewalked;
        return launch_frame(f, q, t);
    };
    return nrm ? launch(ShadeNormals{nrm}) : launch(NoObjects{});
}

int matpbr_path_render_relight(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                               float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                               int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, uint32_t* rays, void* stream,
                               const float* env_b, const float* row_cdf_b, const float* col_cdf_b, const float* env_pdf_b, int He_b, int We_b,
                               const float* nrm, float* base, float* relit) {
    float* const out = base;   // the radiance under the frame's own environment is the render's own sum
    const Frame f = RENDER_FRAME;
    PathArgs q{};
    if (!env_b || !row_cdf_b || !col_cdf_b || !env_pdf_b || He_b <= 0 || We_b <= 0 || !base || !relit || !frame_args(f, q))
        return MATPBR_PATH_ERR_INVALID_ARG;
    auto launch = [&](auto base_table) {   // the second environment's table over the render's own
        Relight<decltype(base_table)> t{};
        static_cast<decltype(base_table)&>(t) = base_table;
        t.env_b = env_b; t.row_cdf_b = row_cdf_b; t.col_cdf_b = col_cdf_b; t.env_pdf_b = env_pdf_b; t.He_b = He_b; t.We_b = We_b; t.relit = relit;
        return launch_frame(f, q, t);
    };
    return nrm ? launch(ShadeNormals{nrm}) : launch(NoObjects{});
}

int matpbr_path_composite_relight(const float* base_sum, const float* relit_sum, const float* photo, int H, int W, float scale, float floor,
                                  float* out, void* stream) {
    if (!composite_relight_args_valid(base_sum, relit_sum, photo, H, W, scale, floor, out)) return MATPBR_PATH_ERR_INVALID_ARG;
    const long P = (long)H * W;
    hipLaunchKernelGGL(composite_relight_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, base_sum, relit_sum, photo, P,
                       scale, floor, out);
    return hipGetLastError() == hipSuccess ? MATPBR_PATH_OK : MATPBR_PATH_ERR_LAUNCH;
}

int matpbr_path_composite_relight_host(const float* base_sum, const float* relit_sum, const float* photo, int H, int W, float scale, float floor,
                                       float* out) {
    if (!composite_relight_args_valid(base_sum, relit_sum, photo, H, W, scale, floor, out)) return MATPBR_PATH_ERR_INVALID_ARG;
    for (long p = 0; p < (long)H * W; ++p) composite_relight_pixel(base_sum, relit_sum, photo, p, scale, floor, out);
    return MATPBR_PATH_OK;
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
        !fov_valid(fov_x_deg))
        return MATPBR_PATH_ERR_INVALID_ARG;
    const Camera c = camera(H, W, fov_x_deg);   // the render's
    for (long k = 0; k < N; ++k) {
        texel[k] = (int32_t)screen_texel(p + 3 * k, c.f_ndc, c.aspect, H, W);
        texel_refracted[k] = (int32_t)trans_lookup(edit->ior, edit->refract_distance, p + 3 * k, n + 3 * k, wo + 3 * k, c.f_ndc, c.aspect, H, W);
    }
    return MATPBR_PATH_OK;
}

static size_t bwd_workspace_bytes(int H, int W, int He, int We, int n_acc) {
    if (H <= 0 || W <= 0 || He <= 0 || We <= 0) return 0;
    const dim3 grid = tile_grid(H, W);
    const size_t n_wg = (size_t)grid.x * (size_t)grid.y;
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
    const Frame f{nodes, tris, a, r, m, H, W, fov_x_deg, env, row_cdf, col_cdf, env_pdf, He, We, spp, max_depth, seed, spp_per_launch, nullptr, rays, stream};
    PathArgs q{};
    if ((!nrm && d_n) || !d_out || !workspace || !frame_args(f, q) || (d_env && (long)He * We > kBwdMaxEnvTexels) ||
        workspace_bytes < bwd_workspace_bytes(H, W, He, We, n_acc) || ((uintptr_t)workspace & 7))
        return MATPBR_PATH_ERR_INVALID_ARG;
    if (!d_a && !d_r && !d_m && !d_env && !d_n) return MATPBR_PATH_OK;
    const dim3 grid = tile_grid(H, W);
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


int matpbr_path_features(const void* nodes, const void* tris, int H, int W, float fov_x_deg, const MatpbrPathObject* objects, int n_objects,
                         const float* obj_nrm, long n_scene_tri, const float* nrm_map, float* geom, void* stream) {
    FeatArgs q{static_cast<const float4*>(nodes), static_cast<const float4*>(tris), obj_nrm, nrm_map, reinterpret_cast<float4*>(geom), H, W};
    ObjTable ot{};
    if (!features_args(objects, n_objects, n_scene_tri, fov_x_deg, q, ot)) return MATPBR_PATH_ERR_INVALID_ARG;
    hipLaunchKernelGGL(features_kernel, tile_grid(H, W), dim3(kTileX, kTileY), 0, (hipStream_t)stream, q, ot);
    return hipGetLastError() == hipSuccess ? MATPBR_PATH_OK : MATPBR_PATH_ERR_LAUNCH;
}

int matpbr_path_features_host(const void* nodes, const void* tris, int H, int W, float fov_x_deg, const MatpbrPathObject* objects, int n_objects,
                              const float* obj_nrm, long n_scene_tri, const float* nrm_map, float* geom) {
    FeatArgs q{static_cast<const float4*>(nodes), static_cast<const float4*>(tris), obj_nrm, nrm_map, reinterpret_cast<float4*>(geom), H, W};
    ObjTable ot{};
    if (!features_args(objects, n_objects, n_scene_tri, fov_x_deg, q, ot)) return MATPBR_PATH_ERR_INVALID_ARG;
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

int matpbr_path_feature_colors(const void* nodes, const void* tris, int H, int W, float fov_x_deg, const MatpbrPathObject* objects, int n_objects,
                               long n_scene_tri, const float* obj_col, float* out, void* stream) {
    FeatColorArgs q{static_cast<const float4*>(nodes), static_cast<const float4*>(tris), obj_col, out, H, W};
    ObjTable ot{};
    if (!feature_colors_args(objects, n_objects, n_scene_tri, fov_x_deg, q, ot)) return MATPBR_PATH_ERR_INVALID_ARG;
    hipLaunchKernelGGL(feature_colors_kernel, tile_grid(H, W), dim3(kTileX, kTileY), 0, (hipStream_t)stream, q, ot);
    return hipGetLastError() == hipSuccess ? MATPBR_PATH_OK : MATPBR_PATH_ERR_LAUNCH;
}

int matpbr_path_feature_colors_host(const void* nodes, const void* tris, int H, int W, float fov_x_deg, const MatpbrPathObject* objects,
                                    int n_objects, long n_scene_tri, const float* obj_col, float* out) {
    FeatColorArgs q{static_cast<const float4*>(nodes), static_cast<const float4*>(tris), obj_col, out, H, W};
    ObjTable ot{};
    if (!feature_colors_args(objects, n_objects, n_scene_tri, fov_x_deg, q, ot)) return MATPBR_PATH_ERR_INVALID_ARG;
    for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j) {
            HostStack stk;
            feature_colors_pixel(q, ot, i, j, stk, out + 3 * ((long)i * W + j));
        }
    return MATPBR_PATH_OK;
}

int matpbr_path_feature_tints(const void* nodes, const void* tris, int H, int W, float fov_x_deg, const MatpbrPathObject* objects, int n_objects,
                              long n_scene_tri, const float* obj_col, const float* obj_uv, const MatpbrPathObjectTex* tex, const void* texels,
                              long n_texels, float* out, void* stream) {
    FeatColorArgs q{static_cast<const float4*>(nodes), static_cast<const float4*>(tris), obj_col, out, H, W};
    ObjTable ot{};
    FeatTextures tx;
    if (!feature_tints_args(objects, n_objects, n_scene_tri, fov_x_deg, obj_uv, tex, texels, n_texels, q, ot, tx)) return MATPBR_PATH_ERR_INVALID_ARG;
    hipLaunchKernelGGL(feature_tints_kernel, tile_grid(H, W), dim3(kTileX, kTileY), 0, (hipStream_t)stream, q, ot, tx);
    return hipGetLastError() == hipSuccess ? MATPBR_PATH_OK : MATPBR_PATH_ERR_LAUNCH;
}

int matpbr_path_feature_tints_host(const void* nodes, const void* tris, int H, int W, float fov_x_deg, const MatpbrPathObject* objects,
                                   int n_objects, long n_scene_tri, const float* obj_col, const float* obj_uv, const MatpbrPathObjectTex* tex,
                                   const void* texels, long n_texels, float* out) {
    FeatColorArgs q{static_cast<const float4*>(nodes), static_cast<const float4*>(tris), obj_col, out, H, W};
    ObjTable ot{};
    FeatTextures tx;
    if (!feature_tints_args(objects, n_objects, n_scene_tri, fov_x_deg, obj_uv, tex, texels, n_texels, q, ot, tx)) return MATPBR_PATH_ERR_INVALID_ARG;
    for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j) {
            HostStack stk;
            feature_colors_pixel(q, ot, i, j, stk, out + 3 * ((long)i * W + j), tx);
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

// ---- the differential render's filter: the steps, their CPU twins and the chain (the twins and the chain share one walk each) ----------
static bool diff_prepare_args(const DiffHalves& x, const float* geom, int H, int W, float scale, const float* cv0, const float* cov) {
    return diff_halves_valid(x) && geom && cv0 && cov && denoise_size_valid(H, W) && diff_scale_valid(scale);
}
static bool diff_level_args(const float* cv_in, const float* cov, const float* geom, const float* alb, int H, int W, const MatpbrPathDenoise* prm,
                            int level, const float* cv_out) {
    return cv_in && cov && geom && alb && cv_out && cv_in != cv_out && denoise_size_valid(H, W) && denoise_params_valid(prm) && level >= 0 &&
           level < kDnMaxLevels;
}
static bool diff_finish_args(const float* cv, const float* cov, const DiffHalves& x, const float* geom, int H, int W, float scale, const float* fg,
                             const float* delta, const float* alpha) {
    return cv && cov && diff_halves_valid(x) && geom && fg && delta && alpha && denoise_size_valid(H, W) && diff_scale_valid(scale);
}
static void diff_prepare_host(const DiffHalves& x, const float4* geom, int H, int W, float scale, float4* cv0, float* cov) {
    for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j) cov[(long)i * W + j] = dd_prepare_pixel(x, geom, H, W, i, j, scale, cv0[(long)i * W + j]);
}
static void diff_level_host(const float4* cv, const float* cov, const float4* geom, const float* alb, int H, int W, int s,
                            const MatpbrPathDenoise& prm, float4* cv_out) {
    for (int i = 0; i < H; ++i)
        for (int j = 0; j < W; ++j) cv_out[(long)i * W + j] = dn_level_pixel<true>(cv, geom, alb, H, W, i, j, s, prm, cov);
}
static void diff_finish_host(const float4* cv, const float* cov, const DiffHalves& x, const float4* geom, int H, int W, float scale, float* fg,
                             float* delta, float* alpha) {
    for (long p = 0; p < (long)H * W; ++p) dd_finish_pixel(cv, cov, x, geom, p, scale, fg, delta, alpha);
}

int matpbr_path_denoise_diff_prepare(const float* fgA, const float* deltaA, const float* alphaA, const float* fgB, const float* deltaB,
                                     const float* alphaB, const float* geom, int H, int W, float scale, float* cv0, float* cov, void* stream) {
    const DiffHalves x{fgA, deltaA, alphaA, fgB, deltaB, alphaB};
    if (!diff_prepare_args(x, geom, H, W, scale, cv0, cov)) return MATPBR_PATH_ERR_INVALID_ARG;
    hipLaunchKernelGGL(denoise_diff_prepare_kernel, denoise_grid(H, W), dim3(kDnTileX, kDnTileY), 0, (hipStream_t)stream, x,
                       reinterpret_cast<const float4*>(geom), H, W, scale, reinterpret_cast<float4*>(cv0), cov);
    return hipGetLastError() == hipSuccess ? MATPBR_PATH_OK : MATPBR_PATH_ERR_LAUNCH;
}

int matpbr_path_denoise_diff_prepare_host(const float* fgA, const float* deltaA, const float* alphaA, const float* fgB, const float* deltaB,
                                          const float* alphaB, const float* geom, int H, int W, float scale, float* cv0, float* cov) {
    const DiffHalves x{fgA, deltaA, alphaA, fgB, deltaB, alphaB};
    if (!diff_prepare_args(x, geom, H, W, scale, cv0, cov)) return MATPBR_PATH_ERR_INVALID_ARG;
    diff_prepare_host(x, reinterpret_cast<const float4*>(geom), H, W, scale, reinterpret_cast<float4*>(cv0), cov);
    return MATPBR_PATH_OK;
}

int matpbr_path_denoise_diff_level(const float* cv_in, const float* cov, const float* geom, const float* alb, int H, int W,
                                   const MatpbrPathDenoise* prm, int level, float* cv_out, void* stream) {
    if (!diff_level_args(cv_in, cov, geom, alb, H, W, prm, level, cv_out)) return MATPBR_PATH_ERR_INVALID_ARG;
    hipLaunchKernelGGL(denoise_diff_level_kernel, denoise_grid(H, W), dim3(kDnTileX, kDnTileY), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(cv_in), cov, reinterpret_cast<const float4*>(geom), alb, H, W, 1 << level, *prm,
                       reinterpret_cast<float4*>(cv_out));
    return hipGetLastError() == hipSuccess ? MATPBR_PATH_OK : MATPBR_PATH_ERR_LAUNCH;
}

int matpbr_path_denoise_diff_level_host(const float* cv_in, const float* cov, const float* geom, const float* alb, int H, int W,
                                        const MatpbrPathDenoise* prm, int level, float* cv_out) {
    if (!diff_level_args(cv_in, cov, geom, alb, H, W, prm, level, cv_out)) return MATPBR_PATH_ERR_INVALID_ARG;
    diff_level_host(reinterpret_cast<const float4*>(cv_in), cov, reinterpret_cast<const float4*>(geom), alb, H, W, 1 << level, *prm,
                    reinterpret_cast<float4*>(cv_out));
    return MATPBR_PATH_OK;
}

int matpbr_path_denoise_diff_finish(const float* cv, const float* cov, const float* fgA, const float* deltaA, const float* alphaA, const float* fgB,
                                    const float* deltaB, const float* alphaB, const float* geom, int H, int W, float scale, float* fg, float* delta,
                                    float* alpha, void* stream) {
    const DiffHalves x{fgA, deltaA, alphaA, fgB, deltaB, alphaB};
    if (!diff_finish_args(cv, cov, x, geom, H, W, scale, fg, delta, alpha)) return MATPBR_PATH_ERR_INVALID_ARG;
    hipLaunchKernelGGL(denoise_diff_finish_kernel, denoise_grid(H, W), dim3(kDnTileX, kDnTileY), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(cv), cov, x, reinterpret_cast<const float4*>(geom), H, W, scale, fg, delta, alpha);
    return hipGetLastError() == hipSuccess ? MATPBR_PATH_OK : MATPBR_PATH_ERR_LAUNCH;
}

int matpbr_path_denoise_diff_finish_host(const float* cv, const float* cov, const float* fgA, const float* deltaA, const float* alphaA,
                                         const float* fgB, const float* deltaB, const float* alphaB, const float* geom, int H, int W, float scale,
                                         float* fg, float* delta, float* alpha) {
    const DiffHalves x{fgA, deltaA, alphaA, fgB, deltaB, alphaB};
    if (!diff_finish_args(cv, cov, x, geom, H, W, scale, fg, delta, alpha)) return MATPBR_PATH_ERR_INVALID_ARG;
    diff_finish_host(reinterpret_cast<const float4*>(cv), cov, x, reinterpret_cast<const float4*>(geom), H, W, scale, fg, delta, alpha);
    return MATPBR_PATH_OK;
}

size_t matpbr_path_denoise_diff_workspace_bytes(int H, int W) {
    return denoise_size_valid(H, W) ? (size_t)H * (size_t)W * (2 * sizeof(float4) + sizeof(float)) : 0;
}

static bool diff_chain_args(const DiffHalves& x, const float* geom, const float* alb, int H, int W, float scale, const MatpbrPathDenoise* prm,
                            const float* fg, const float* delta, const float* alpha, const void* workspace, size_t workspace_bytes) {
    return diff_halves_valid(x) && geom && alb && fg && delta && alpha && workspace && denoise_size_valid(H, W) && diff_scale_valid(scale) &&
           denoise_params_valid(prm) && workspace_bytes >= matpbr_path_denoise_diff_workspace_bytes(H, W) && !((uintptr_t)workspace & 15);
}

int matpbr_path_denoise_diff(const float* fgA, const float* deltaA, const float* alphaA, const float* fgB, const float* deltaB, const float* alphaB,
                             const float* geom, const float* alb, int H, int W, float scale, const MatpbrPathDenoise* prm, float* fg, float* delta,
                             float* alpha, void* workspace, size_t workspace_bytes, void* stream) {
    const DiffHalves x{fgA, deltaA, alphaA, fgB, deltaB, alphaB};
    if (!diff_chain_args(x, geom, alb, H, W, scale, prm, fg, delta, alpha, workspace, workspace_bytes)) return MATPBR_PATH_ERR_INVALID_ARG;
    const MatpbrPathDenoise pr = *prm;
    float4* ws[2] = {static_cast<float4*>(workspace), static_cast<float4*>(workspace) + (size_t)H * W};
    float* cov = reinterpret_cast<float*>(ws[1] + (size_t)H * W);
    const float4* g = reinterpret_cast<const float4*>(geom);
    const dim3 grid = denoise_grid(H, W), block(kDnTileX, kDnTileY);
    hipLaunchKernelGGL(denoise_diff_prepare_kernel, grid, block, 0, (hipStream_t)stream, x, g, H, W, scale, ws[0], cov);
    if (hipGetLastError() != hipSuccess) return MATPBR_PATH_ERR_LAUNCH;
    for (int l = 0; l < pr.levels; ++l) {
        hipLaunchKernelGGL(denoise_diff_level_kernel, grid, block, 0, (hipStream_t)stream, (const float4*)ws[l & 1], (const float*)cov, g, alb, H, W,
                           1 << l, pr, ws[(l + 1) & 1]);
        if (hipGetLastError() != hipSuccess) return MATPBR_PATH_ERR_LAUNCH;
    }
    hipLaunchKernelGGL(denoise_diff_finish_kernel, grid, block, 0, (hipStream_t)stream, (const float4*)ws[pr.levels & 1], (const float*)cov, x, g, H,
                       W, scale, fg, delta, alpha);
    return hipGetLastError() == hipSuccess ? MATPBR_PATH_OK : MATPBR_PATH_ERR_LAUNCH;
}

int matpbr_path_denoise_diff_host(const float* fgA, const float* deltaA, const float* alphaA, const float* fgB, const float* deltaB,
                                  const float* alphaB, const float* geom, const float* alb, int H, int W, float scale, const MatpbrPathDenoise* prm,
                                  float* fg, float* delta, float* alpha, void* workspace, size_t workspace_bytes) {
    const DiffHalves x{fgA, deltaA, alphaA, fgB, deltaB, alphaB};
    if (!diff_chain_args(x, geom, alb, H, W, scale, prm, fg, delta, alpha, workspace, workspace_bytes)) return MATPBR_PATH_ERR_INVALID_ARG;
    float4* ws[2] = {static_cast<float4*>(workspace), static_cast<float4*>(workspace) + (size_t)H * W};
    float* cov = reinterpret_cast<float*>(ws[1] + (size_t)H * W);
    const float4* g = reinterpret_cast<const float4*>(geom);
    diff_prepare_host(x, g, H, W, scale, ws[0], cov);
    for (int l = 0; l < prm->levels; ++l) diff_level_host(ws[l & 1], cov, g, alb, H, W, 1 << l, *prm, ws[(l + 1) & 1]);
    diff_finish_host(ws[prm->levels & 1], cov, x, g, H, W, scale, fg, delta, alpha);
    return MATPBR_PATH_OK;
}

}  // extern "C"
