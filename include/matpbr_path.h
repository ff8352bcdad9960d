/*
 * matpbr_path.h -- C ABI of libmatpbr_path.so: a path-traced re-render of the depth mesh and its backward pass (MI355X, gfx950).
 *
 * The integrator is Mitsuba 3's `path` as the reference configures it for its final images (render_final.py:35-96,
 * inverse_img_w_mi.py:49-52: `max_depth` 4, MatDiffBSDF on the `.ply` depth mesh, shading with the face normals or with a
 * shading-normal map (MatDiffBSDF's use_mesh_normal=False: the *_normals entry points), equirectangular envmap emitter); its
 * definition and the ways it differs from Mitsuba are DESIGN.md section 1.4.  It is a separate library so that
 * libmatpbr.so's sources (and the digest the traffic profile is tied to) stay untouched.
 *
 * Conventions (those of matpbr.h)
 *   - Host pointers are named *_host or belong to the *_host / build entry points; matpbr_path_render takes DEVICE pointers.
 *   - Maps a[H,W,3] r[H,W,1] m[H,W,1], envmap env[He,W_e,3], output out[H,W,3]: fp32, contiguous, row-major HWC.
 *   - `stream` is the caller's hipStream_t (NULL = default stream); the render only enqueues work.
 *   - Return value: 0 = MATPBR_OK, negative = error (matpbr_path_strerror); nothing throws.
 */
#ifndef MATPBR_PATH_H
#define MATPBR_PATH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MATPBR_PATH_VERSION 3
#define MATPBR_PATH_MAX_BVH_DEPTH 40 /* node levels below the root the builder may create; the kernel's traversal stack has this many entries */
#define MATPBR_PATH_MAX_MAX_DEPTH 16 /* largest `max_depth` matpbr_path_render / matpbr_path_render_bwd accept */
#define MATPBR_PATH_BWD_MAX_ENV_TEXELS 1024 /* largest He * We matpbr_path_render_bwd takes with d_env */
#define MATPBR_PATH_NODE_BYTES 64    /* one node: both children's boxes (2 x 24 B) + two child words + two counts */
#define MATPBR_PATH_TRI_BYTES 48     /* one triangle in leaf order: (v0, id) (e1, 0) (e2, 0) as float4; e1 x e2 faces the camera */
#define MATPBR_PATH_MAX_OBJECTS 8    /* inserted meshes matpbr_path_render_objects takes */

enum {
    MATPBR_PATH_OK = 0,
    MATPBR_PATH_ERR_INVALID_ARG = -1,
    MATPBR_PATH_ERR_LAUNCH = -3,
    MATPBR_PATH_ERR_CAPACITY = -4,
};

/* BSDF of an inserted mesh ("Inserted objects") */
enum {
    MATPBR_PATH_BSDF_DIELECTRIC = 1, /* smooth glass, a delta BSDF: p[0] = int_ior, p[1] = ext_ior (p[2] unused) */
    MATPBR_PATH_BSDF_DIFFUSE = 2,    /* one-sided Lambertian: p = reflectance RGB in [0, 1] */
    MATPBR_PATH_BSDF_PBR = 3,        /* MatDiffBSDF on constants, one-sided: a MatpbrPathObjectPbr record beside the table; p[] is ignored.
                                        Only matpbr_path_render_objects_pbr (and the feature entry points) take it. */
    MATPBR_PATH_BSDF_AREA = 4,       /* an area light, one-sided, no BSDF: p = radiance RGB, finite and >= 0 (0 is valid).  Never with
                                        MATPBR_PATH_OBJECT_SMOOTH.  Only matpbr_path_render_objects_lights, matpbr_path_light_tables (and
                                        the feature entry points) take it; to every other entry point it is an unknown kind. */
    MATPBR_PATH_BSDF_ROUGH_DIELECTRIC = 5, /* rough glass (Walter et al. 2007, GGX, visible normals), two-sided, never delta:
                                        p[0] = int_ior, p[1] = ext_ior, p[2] = alpha (the GGX width) in [0.02, 1]; the indices finite and
                                        > 0 with |int_ior / ext_ior - 1| >= 0.01.  MATPBR_PATH_OBJECT_SMOOTH may be OR-ed in.  Only
                                        matpbr_path_render_objects_rough, matpbr_path_light_tables, matpbr_path_object_lookup_host (and
                                        the feature entry points) take it; to every other entry point it is an unknown kind. */
};

/* OR-ed into MatpbrPathObject.kind: the object shades with interpolated corner normals ("Smooth inserted
 * objects").  Only matpbr_path_render_objects_normals takes it; to matpbr_path_render_objects it is an unknown kind. */
#define MATPBR_PATH_OBJECT_SMOOTH 0x100

/* OR-ed into MatpbrPathObject.kind beside MATPBR_PATH_OBJECT_SMOOTH: the object's reflectance (kind 2) or albedo (kind 3) is multiplied
 * by a colour interpolated from its corners ("Vertex-coloured inserted objects").  Valid on kinds 2 and 3 only.
 * Only matpbr_path_render_objects_colors and matpbr_path_feature_colors take it; to every other entry point it is an unknown kind. */
#define MATPBR_PATH_OBJECT_COLORED 0x200

/* OR-ed into MatpbrPathObject.kind beside the two flags above: the object's reflectance (kind 2) or albedo (kind 3) is multiplied by a
 * base-colour image, and a kind-3 object's roughness and metallic by an orm image, both looked up at the texture coordinate interpolated
 * from its corners ("Textured inserted objects").  Valid on kinds 2 and 3 only.  Only
 * matpbr_path_render_objects_textures and matpbr_path_feature_tints take it; to every other entry point it is an unknown kind. */
#define MATPBR_PATH_OBJECT_TEXTURED 0x400

/* OR-ed into MatpbrPathObject.kind beside MATPBR_PATH_OBJECT_SMOOTH: the volume behind the object's interface holds a homogeneous
 * medium, a MatpbrPathObjectMedium record beside the table ("Media inside glass").  Valid on kinds 1 and 5 only.
 * Only matpbr_path_render_objects_media and matpbr_path_render_objects_diff_media take it; to every other entry point it is an unknown
 * kind. */
#define MATPBR_PATH_OBJECT_MEDIUM 0x800

/* OR-ed into MatpbrPathObject.kind beside the four flags above: a vertex on the object keeps the camera chain of the see-through rule
 * alive, so that what the object reflects (or, through rough glass, transmits) of the depth mesh is the photograph (DESIGN.md section
 * 1.4, "Reflected in inserted objects").  Valid on kinds 2, 3 and 5 only: kind 4 has no BSDF, and on kind 1 the see-through rule holds
 * already.  Only matpbr_path_render_objects_reflect and matpbr_path_reflect_chain_host take it; to every other entry point it is an
 * unknown kind. */
#define MATPBR_PATH_OBJECT_PHOTO 0x1000

/* One inserted mesh: triangles [first_tri, first_tri + n_tri) of the mesh handed to matpbr_path_bvh_build_objects (ids at or
 * above its n_scene_tri), outward winding. */
typedef struct MatpbrPathObject {
    int32_t kind;
    int32_t first_tri;
    int32_t n_tri;
    float p[3];
} MatpbrPathObject;

/* The material of an object of kind MATPBR_PATH_BSDF_PBR ("PBR inserted objects"): the depth mesh's BSDF
 * on constants.  MatpbrPathObject is frozen, so the record travels beside the table, one per object (read for kind 3 only).  Valid:
 * a[c] in [0, 1], r in [0.07, 1] (the floor the project's roughness maps are clamped to), m in [0, 1], all finite. */
typedef struct MatpbrPathObjectPbr {
    float a[3];
    float r;
    float m;
    float reserved[3];
} MatpbrPathObjectPbr;

/* The images of an object that carries MATPBR_PATH_OBJECT_TEXTURED, one record per object beside the table (read for flagged objects
 * only): image x is texels [x_first, x_first + x_w x_h) of the texel buffer, row-major, row 0 the top row; x_w == 0: no such image.
 * Valid: at least one image; orm on kind 3 only; w, h in [1, 8192]; first >= 0; first + w h <= n_texels; reserved == 0. */
typedef struct MatpbrPathObjectTex {
    int32_t base_first, base_w, base_h; /* base colour: linear r, g, b */
    int32_t orm_first, orm_w, orm_h;    /* glTF's occlusion (ignored), roughness, metallic */
    int32_t reserved[2];
} MatpbrPathObjectTex;

/* The medium inside an object that carries MATPBR_PATH_OBJECT_MEDIUM, one record per object beside the table (read for flagged objects
 * only): absorption per channel and grey scattering, both per scene unit, and the Henyey-Greenstein asymmetry.  Valid: sigma_a[c] and
 * sigma_s finite and >= 0 (all zero is valid: the medium multiplies by exactly 1), |g| <= 0.99, reserved == 0. */
typedef struct MatpbrPathObjectMedium {
    float sigma_a[3];
    float sigma_s;
    float g;
    float reserved[3];
} MatpbrPathObjectMedium;

/* Transparency editing ("Transparency editing"): the reference's TransBSDF where the mask is set. */
typedef struct MatpbrPathTransEdit {
    float ior;              /* index of refraction of the glass, > 0 (trans_edit.py --ior, default 1.2) */
    float spec_trans;       /* specTrans in [0, 1] (default 0.4) */
    float refract_distance; /* the sheet's thickness scale D >= 0: the lookup walks 0.3 D into the glass and D out of it (100) */
    float reserved;
} MatpbrPathTransEdit;

int matpbr_path_version(void);
const char* matpbr_path_strerror(int code);

/* Upper bounds of the BVH buffers for `n_tri` triangles: *max_nodes nodes of MATPBR_PATH_NODE_BYTES, n_tri triangles of
 * MATPBR_PATH_TRI_BYTES. */
int matpbr_path_bvh_size(long n_tri, long* max_nodes);

/* Binned-SAH BVH2 over triangles tri[n_tri,3] (int32 indices into vert[n_vert,3], float64) -> nodes (node 0 = root), triangles in
 * leaf order.  Host only; `nodes` holds `max_nodes` nodes (matpbr_path_bvh_size), `tris` n_tri triangles.  Writes the node count,
 * the deepest node level (<= MATPBR_PATH_MAX_BVH_DEPTH) and the number of leaves.  Triangles with an index outside the vertex
 * array are an error. */
int matpbr_path_bvh_build(const double* vert, long n_vert, const int32_t* tri, long n_tri, void* nodes, long max_nodes, void* tris,
                          long* n_nodes, int* depth, long* n_leaves);

/* matpbr_path_bvh_build for a depth mesh with inserted meshes appended: triangles [0, n_scene_tri) are turned to the camera side
 * as above; triangles [n_scene_tri, n_tri) keep their winding, so that e1 x e2 is the mesh's outward normal.  With n_scene_tri ==
 * n_tri the output is matpbr_path_bvh_build's, byte for byte. */
int matpbr_path_bvh_build_objects(const double* vert, long n_vert, const int32_t* tri, long n_tri, long n_scene_tri, void* nodes,
                                  long max_nodes, void* tris, long* n_nodes, int* depth, long* n_leaves);

/* Closest hit of N rays (origin o[N,3], direction d[N,3], hits with tmin < t < tmax) on the CPU, with the routine the kernel runs:
 * t_hit[N] (tmax where there is no hit), tri_hit[N] = triangle index of the input mesh or -1. */
int matpbr_path_trace_host(const void* nodes, const void* tris, const float* o, const float* d, long N, float tmin, float tmax,
                           float* t_hit, int32_t* tri_hit);

/* Importance-sampling tables of an equirectangular envmap env[He,We,3] (host, built in fp64, stored fp32): row_cdf[He+1] (marginal
 * over rows of luminance x texel solid angle), col_cdf[He,We+1] (conditional over the columns of each row), pdf[He,We] = the
 * solid-angle density of a direction in each texel's cell.  An envmap of zero luminance gets all-zero tables (no emitter
 * sampling).  *total = sum of luminance x solid angle. */
int matpbr_path_env_tables(const float* env, int He, int We, float* row_cdf, float* col_cdf, float* pdf, double* total);

/* The render's emitter sampler on the CPU: u[N,4] -> dir[N,3], pdf_out[N], texel[N] (row * We + col; -1 without tables). */
int matpbr_path_env_sample_host(const float* row_cdf, const float* col_cdf, const float* pdf, int He, int We, const float* u, long N,
                                float* dir, float* pdf_out, int32_t* texel);

/* The render: `spp` samples per pixel, accumulated in a fixed order per pixel (no atomics) and enqueued as launches of at most
 * `spp_per_launch` samples; every split gives the same bits.  out[H,W,3] = linear radiance (mean over samples).  `max_depth` is
 * Mitsuba's (1 = emission only, 2 = direct light with shadows, 4 = up to three surface vertices).  `nodes`/`tris` are the
 * builder's output copied to the device; env + its three tables as matpbr_path_env_tables made them.  `rays` (nullable, [H,W]):
 * the number of rays each pixel traced (camera, bounce and shadow rays) is ADDED to it. */
int matpbr_path_render(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W, float fov_x_deg,
                       const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He, int We, int spp,
                       int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream);

/* matpbr_path_render over a BVH made by matpbr_path_bvh_build_objects, forward only.  objects[n_objects] (HOST memory, copied
 * before the call returns; n_objects <= MATPBR_PATH_MAX_OBJECTS) gives the BSDF of each range of triangle ids; ids in no range
 * are the depth mesh and shade as in matpbr_path_render.  A dielectric vertex is a delta vertex: no emitter sample, reflection or
 * refraction chosen by dim 6 against the exact Fresnel reflectance, and the envmap seen by its ray is added unweighted.  Ranges
 * must not overlap; an unknown kind, an index of refraction <= 0 or a reflectance outside [0, 1] is an invalid argument.  With
 * n_objects == 0 this is matpbr_path_render, bit for bit.  The camera is assumed to be outside every object. */
int matpbr_path_render_objects(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                               float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                               int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream,
                               const MatpbrPathObject* objects, int n_objects);

/* The BSDF sampler of an inserted object on the CPU, with the routine the kernel runs: face normal n[3] (outward), N directions
 * wo[N,3] towards the viewer, u[N,3] = dims 6, 7, 8 of a vertex -> wi[N,3], weight[N,3] (BSDF x cosine / pdf; 0 = the path ends),
 * pdf[N] (solid angle; for the dielectric the probability of the chosen event), flags[N] (bit 0: delta, bit 1: transmitted). */
int matpbr_path_object_sample_host(const MatpbrPathObject* object, const float* n, const float* wo, const float* u, long N, float* wi,
                                   float* weight, float* pdf, int32_t* flags);

/* matpbr_path_render_objects where an object whose kind carries MATPBR_PATH_OBJECT_SMOOTH shades with its vertex normals.  obj_nrm
 * (DEVICE, fp32, [n_tri - n_scene_tri, 3, 3]): one normal per corner of every inserted triangle, in input order, indexed by
 * id - n_scene_tri, outward, any length; the triangles of objects without the flag are never read.  At a hit on a smooth object
 * u, v are Moller-Trumbore's (u the second input vertex's, v the third's), ns = normalize((1 - u - v) n0 + u n1 + v n2), and
 * ns = ng, the face normal, where ns is not finite or of zero length, where ns . ng <= 0, or where (ns . wo)(ng . wo) <= 0.  The
 * BSDF shades with ns, ng keeps the geometry (back-face test, spawn offset, side of an emitter sample, a diffuse sample below ng
 * ends the path), and a dielectric event about ns that disagrees with ng about crossing the surface is redone about ng.  With
 * obj_nrm == NULL or no flagged object this launches matpbr_path_render_objects' kernel and gives its bits.  Invalid arguments,
 * besides matpbr_path_render_objects': a flagged object with obj_nrm == NULL, an object range that starts below n_scene_tri. */
int matpbr_path_render_objects_normals(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                       float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                       int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream,
                                       const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri);

/* The shading normal of a smooth object on the CPU, with the routines the kernel runs (the barycentrics of the winning triangle
 * and the interpolation with its first two fallbacks): per lane the triangle record tri[N,3,3] = (v0, e1, e2), the corner normals
 * nrm[N,3,3] and the ray o[N,3], d[N,3] -> u[N], v[N], ns[N,3].  The face normal is normalize(e1 x e2), formed here with a plain
 * division (the kernel's uses the device's reciprocal square root). */
int matpbr_path_object_normal_host(const float* tri, const float* nrm, const float* o, const float* d, long N, float* u, float* v, float* ns);

/* matpbr_path_object_sample_host at vertices with a face normal ng[N,3] and a shading normal ns[N,3] (unit length, as
 * matpbr_path_object_normal_host returns it), with the routine the kernel runs at a smooth object: the third fallback (ns = ng where
 * the two disagree about wo's side), the sample about ns, the dielectric's redo about ng where the event disagrees with the geometry,
 * weight 0 for a diffuse sample below ng or a diffuse vertex seen from behind ng.  Same outputs, same flags. */
int matpbr_path_object_sample_shading_host(const MatpbrPathObject* object, const float* ng, const float* ns, const float* wo, const float* u,
                                           long N, float* wi, float* weight, float* pdf, int32_t* flags);

/* matpbr_path_render_objects_normals where an object may be of kind MATPBR_PATH_BSDF_PBR (with or without
 * MATPBR_PATH_OBJECT_SMOOTH).  pbr[n_objects] (HOST memory, copied before the call returns): record k is object k's material and is
 * read only where object k is of kind 3.  A vertex on such an object is the depth mesh's vertex of matpbr_path_render_normals on the
 * record's constants: one-sided about the outward face normal ng, no texel read, ns = ng or, where smooth, the interpolated normal
 * with its three fallbacks; the emitter sample needs ng . wl > 0 and takes f and its pdf from the BSDF about ns; the BSDF sample is
 * MatDiffBSDF's about ns (lobe by dim 6 > 0.5, weight f / (pdf + 1e-6) where pdf > 1e-6), not a delta event, a sample with
 * ng . wi <= 0 ends the path, and the next ray starts on ng's side.  This is level 3 of the table in DESIGN.md section 1.4, "The
 * object entries": with no object of kind 3 it launches matpbr_path_render_objects_normals' kernel and gives its bits (pbr may be NULL
 * then).  Invalid arguments, besides that entry point's: an object of kind 3 with pbr == NULL or with a record outside the ranges
 * above. */
int matpbr_path_render_objects_pbr(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                   float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                   int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream,
                                   const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                   const MatpbrPathObjectPbr* pbr);

/* The table lookup of matpbr_path_render_objects_pbr on the CPU, with the routine the kernel runs: triangle ids[N] -> kind[N] (0: the
 * id lies in no range; the smooth flag is kept), a[N,3], r[N], m[N] (the record of an object of kind 3; 0 for every other id).  The
 * table and the records are checked as the render checks them (pbr may be NULL when no object is of kind 3). */
int matpbr_path_object_lookup_host(const MatpbrPathObject* objects, int n_objects, const MatpbrPathObjectPbr* pbr, const int32_t* ids, long N,
                                   int32_t* kind, float* a, float* r, float* m);

/* ---- Emissive inserted objects ("Emissive inserted objects") -------------------------------------------------
 * The emitters of a scene are the envmap, where it has tables (row_cdf[He] > 0), then the objects of kind MATPBR_PATH_BSDF_AREA in
 * table order, each as one emitter; n_e is their count.  The header below travels to the kernel by value; the lights' triangle
 * records and cumulative areas are buffers. */
typedef struct MatpbrPathLights {
    int32_t n_lights;                         /* the objects of kind 4 */
    int32_t object[MATPBR_PATH_MAX_OBJECTS];  /* light l is objects[object[l]]: ascending */
    int32_t first[MATPBR_PATH_MAX_OBJECTS];   /* its records: [first[l], first[l] + n_tri[l]) of light_tris / light_cdf; first[0] = 0, contiguous */
    int32_t n_tri[MATPBR_PATH_MAX_OBJECTS];
    float area[MATPBR_PATH_MAX_OBJECTS];      /* its area: summed in fp64, > 0 */
} MatpbrPathLights;

/* The light tables of a merged mesh (host; vert / tri / objects as matpbr_path_bvh_build_objects and the renders take them): the
 * header, *n_light_tri = the records every light's triangles need, and, where light_tris != NULL, light_tris[n_light_tri, 3, 4]
 * (fp32: (v0, 0) (e1, 0) (e2, 0) of each light triangle in input order, rounded as the BVH rounds them) and light_cdf[n_light_tri]
 * (per light: the cumulative area / the light's area, built in fp64, stored fp32, upper bounds, the last exactly 1).  `capacity`:
 * the records both buffers hold (MATPBR_PATH_ERR_CAPACITY when too few).  With light_tris == NULL only the header and the count are
 * written: call once for the sizes, once more for the tables.  Invalid arguments: a bad table (a negative or non-finite radiance,
 * kind 4 with the smooth flag, ...), a light's range outside the mesh, a light of total area 0.  A table without lights gives
 * n_lights = 0 and *n_light_tri = 0. */
int matpbr_path_light_tables(const double* vert, long n_vert, const int32_t* tri, long n_tri, const MatpbrPathObject* objects, int n_objects,
                             const MatpbrPathObjectPbr* pbr, MatpbrPathLights* lights, float* light_tris, float* light_cdf, long capacity,
                             long* n_light_tri);

/* matpbr_path_render_objects_pbr where an object may be of kind MATPBR_PATH_BSDF_AREA, forward only.  `lights` (HOST, copied before
 * the call returns), light_tris and light_cdf (DEVICE, 16-byte aligned, as matpbr_path_light_tables made them).  At every non-delta
 * vertex ONE emitter is sampled (dims 2-5): idx = min(int(u2 n_e), n_e - 1), u2' = u2 n_e - idx (kept below 1); the envmap by
 * (u2', u3, u4, u5) with pdf_e / n_e; light l by the first triangle whose cumulative area exceeds u2', the point
 * y = v0 + (1 - s) e1 + s u4 e2 with s = sqrt(1 - u3), wl = normalize(y - po), dist = |y - po|, pdf = dist^2 / (A cos_l n_e); it needs
 * cos_l = n_l . (-wl) > 0, ng . wl > 0, dist > 0; the shadow ray is any-hit up to dist (1 - 1e-3); the sample adds
 * thr f p mis(pdf, pdf_b) / pdf.  A traced ray that lands on a light's front (ng . wo > 0) adds thr p w, w = 1 at depth 0 or after a
 * delta vertex, else mis(prev_pdf, t^2 / (A (ng . wo) n_e)), BEFORE the max_depth test, and ends; on its back it ends with nothing
 * added.  An escaped ray's weight takes env_pdf / n_e.  This is level 4 of the table in DESIGN.md section 1.4, "The object entries":
 * without an object of kind 4 it launches matpbr_path_render_objects_pbr's kernel and gives its bits (the three light arguments may
 * be NULL then).  Invalid arguments, besides that entry point's: a negative or
 * non-finite radiance, kind 4 with the smooth flag, null tables with a kind-4 object, a header that is not the table's (the lights
 * are the kind-4 objects in order, records contiguous from 0, n_tri the object's), an area that is not finite and > 0. */
int matpbr_path_render_objects_lights(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                      float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                      int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream,
                                      const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                      const MatpbrPathObjectPbr* pbr, const MatpbrPathLights* lights, const void* light_tris,
                                      const float* light_cdf);

/* The emitter sample of matpbr_path_render_objects_lights on the CPU, with the routines the kernel runs (every pointer HOST;
 * n_light_tri: the records the two buffers hold, checked against the header).  have_env: whether the envmap is emitter 0.  From
 * po[N,3] with u[N,4] = dims 2-5 -> emitter[N] (the index among the n_e emitters), u_re[N] = u2', and for a light: record[N] (the
 * triangle's index in light_tris; -1 for the envmap), y[N,3], wl[N,3], dist[N], pdf[N] (0 where cos_l <= 0 or dist = 0; the test
 * against the vertex's normal is the caller's).  For the envmap y, wl, dist, pdf are 0 (matpbr_path_env_sample_host samples it). */
int matpbr_path_light_sample_host(const MatpbrPathLights* lights, const void* light_tris, const float* light_cdf, long n_light_tri, int have_env,
                                  const float* po, const float* u, long N, int32_t* emitter, float* u_re, int32_t* record, float* y, float* wl,
                                  float* dist, float* pdf);

/* The hit side's pdf on the CPU, with the routine the kernel runs: a ray o[N,3], d[N,3] (unit length) that lands on record[N] of
 * light[N] -> t[N] (Moller-Trumbore's t on the record's plane, the traversal's operations) and pdf[N] = t^2 / (A (n_l . -d) n_e), 0
 * where t <= 0 or the ray meets the back. */
int matpbr_path_light_pdf_host(const MatpbrPathLights* lights, const void* light_tris, long n_light_tri, int have_env, const int32_t* light,
                               const int32_t* record, const float* o, const float* d, long N, float* t, float* pdf);

/* ---- Rough dielectric objects ("Rough dielectric objects") ------------------------------------------------------
 * matpbr_path_render_objects_lights where an object may be of kind MATPBR_PATH_BSDF_ROUGH_DIELECTRIC, forward only.  At a vertex on
 * such an object n is the outward normal the BSDF shades with (the face normal ng, or, where smooth, the interpolated one after its
 * three fallbacks), N = sign(n . wo) n, eta_it = int_ior / ext_ior entering and its inverse leaving.  The half vector h comes from
 * the visible normals of wo (dims 7, 8); dim 6 <= F(wo . h) reflects about h, else refracts about h with the radiance factor
 * eta_ti^2; the weight is G1(wi) (x eta_ti^2), the pdf the solid-angle density, and the vertex is never delta.  A direction w with
 * (ng . w)(n . w) <= 0 carries nothing.  The vertex shades from both sides (no back-face exit); its emitter sample (chosen as
 * matpbr_path_render_objects_lights chooses, sampled from the point spawn_eps off the face on ng's side) is taken on either side of
 * the face, its shadow ray starting spawn_eps off the face on the sample's side.  With a kind-5 object the table may hold no light:
 * the three light arguments may be NULL then, and the envmap, where it has tables, is the only emitter.  This is level 5 of the table
 * in DESIGN.md section 1.4, "The object entries": without a kind-5 object it launches matpbr_path_render_objects_lights' kernel and
 * gives its bits.  Invalid arguments, besides that entry point's: the bounds of kind 5 above. */
int matpbr_path_render_objects_rough(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                     float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                     int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream,
                                     const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                     const MatpbrPathObjectPbr* pbr, const MatpbrPathLights* lights, const void* light_tris,
                                     const float* light_cdf);

/* The BSDF sampler of a kind-5 object on the CPU, with the routine the kernel runs: face normals ng[N,3], shading normals ns[N,3]
 * (unit length; ns = ng on a flat object), wo[N,3], u[N,3] = dims 6, 7, 8 -> wi[N,3], weight[N,3] (0 = the path ends), pdf[N] (solid
 * angle), flags[N] (bit 1: transmitted; bit 0, delta, is never set). */
int matpbr_path_rough_sample_host(const MatpbrPathObject* object, const float* ng, const float* ns, const float* wo, const float* u, long N,
                                  float* wi, float* weight, float* pdf, int32_t* flags);

/* The BSDF evaluation of a kind-5 object on the CPU, with the routine the kernel runs at an emitter sample: directions wl[N,3] ->
 * f[N,3] (with its cosine, the radiance factor included) and pdf[N], the density matpbr_path_rough_sample_host gives wl. */
int matpbr_path_rough_eval_host(const MatpbrPathObject* object, const float* ng, const float* ns, const float* wo, const float* wl, long N,
                                float* f, float* pdf);

/* ---- Vertex-coloured inserted objects ("Vertex-coloured inserted objects") --------------------------------------
 * matpbr_path_render_objects_rough where an object of kind 2 or 3 may carry MATPBR_PATH_OBJECT_COLORED (with or without
 * MATPBR_PATH_OBJECT_SMOOTH), forward only.  obj_col (DEVICE, fp32, [n_tri - n_scene_tri, 3, 3]): one linear RGB triple per corner of
 * every inserted triangle, in input order, indexed by id - n_scene_tri (obj_nrm's layout), finite and in [0, 1] (the caller's
 * responsibility: the library cannot check a device buffer); the triangles of objects without the flag are never read.  At a hit on a
 * flagged object u, v are Moller-Trumbore's (the ones the smooth normal uses), c = clamp(c0 + u (c1 - c0) + v (c2 - c0), 0, 1) per
 * channel, and the vertex shades with reflectance p * c (kind 2) or albedo a * c (kind 3; roughness and metallic stay the record's).
 * Neither sampler depends on the colour: the object walks the paths of its uncoloured twin.  This is level 6 of the table in DESIGN.md
 * section 1.4, "The object entries": without a flagged object it launches matpbr_path_render_objects_rough's kernel choice and gives
 * its bits (obj_col may be NULL then).  Invalid arguments, besides that entry point's: a flagged object with obj_col == NULL, the flag
 * on kind 1, 4 or 5. */
int matpbr_path_render_objects_colors(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                      float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                      int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream,
                                      const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                      const MatpbrPathObjectPbr* pbr, const MatpbrPathLights* lights, const void* light_tris,
                                      const float* light_cdf, const float* obj_col);

/* The colour of a flagged object at a hit on the CPU, with the routines the kernel runs (the barycentrics of the winning triangle and
 * the interpolation): per lane the triangle record tri[N,3,3] = (v0, e1, e2), the corner colours col[N,3,3] and the ray o[N,3], d[N,3]
 * -> u[N], v[N], c[N,3].  Three equal corners give exactly their colour; every c lies in [0, 1]. */
int matpbr_path_object_color_host(const float* tri, const float* col, const float* o, const float* d, long N, float* u, float* v, float* c);

/* The colour guide of the denoiser: one ray per pixel through its centre, matpbr_path_features' ray and traversal.  out[H,W,3] (DEVICE)
 * = the interpolated colour c where the first hit lies on a flagged object, (1, 1, 1) everywhere else (no hit included).  objects
 * (HOST, copied before the call returns; any kind the render entries take), n_scene_tri and obj_col (DEVICE; nullable without a
 * flagged object) as matpbr_path_render_objects_colors takes them.  The barycentrics are formed without contraction, so that the CPU
 * twin gives the same bits. */
int matpbr_path_feature_colors(const void* nodes, const void* tris, int H, int W, float fov_x_deg, const MatpbrPathObject* objects, int n_objects,
                               long n_scene_tri, const float* obj_col, float* out, void* stream);
/* matpbr_path_feature_colors on the CPU with the routine the kernel runs (every pointer HOST). */
int matpbr_path_feature_colors_host(const void* nodes, const void* tris, int H, int W, float fov_x_deg, const MatpbrPathObject* objects,
                                    int n_objects, long n_scene_tri, const float* obj_col, float* out);

/* ---- Textured inserted objects ("Textured inserted objects") ----------------------------------------------------
 * matpbr_path_render_objects_colors where an object of kind 2 or 3 may carry MATPBR_PATH_OBJECT_TEXTURED (with or without the smooth
 * and the colour flag), forward only.  obj_uv (DEVICE, fp32, [n_tri - n_scene_tri, 3, 2]): the texture coordinate (s, t) of every corner
 * of every inserted triangle, in obj_nrm's layout (finite: the caller's responsibility); the triangles of objects without the flag are
 * never read.  texels (DEVICE, 16-byte aligned, n_texels float4 = linear r, g, b, 0 in [0, 1]): all images one after another.  tex (HOST,
 * one record per object, copied before the call returns).  At a hit on a flagged object (s, t) = st0 + u (st1 - st0) + v (st2 - st0)
 * with the smooth normal's u, v; an image is read with bilinear filtering and repeat wrapping, t = 0 its bottom row, texel centres at
 * half-integers; a coordinate that is not finite reads (0, 0, 0).  The vertex shades with reflectance p * c_vertex * c_base (kind 2) or
 * albedo a * c_vertex * c_base, roughness clamp(r * orm.g, 0.07, 1) and metallic clamp(m * orm.b, 0, 1) (kind 3); a factor the object
 * does not carry is 1.  This is level 7 of the table in DESIGN.md section 1.4, "The object entries": without a flagged object it
 * launches matpbr_path_render_objects_colors' kernel choice and gives its bits (obj_uv, tex, texels may be NULL and n_texels 0 then).
 * Invalid arguments, besides that entry point's: a flagged object with obj_uv, tex or texels NULL or texels misaligned, a record that
 * is not valid (MatpbrPathObjectTex), the flag on kind 1, 4 or 5. */
int matpbr_path_render_objects_textures(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                        float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                        int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream,
                                        const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                        const MatpbrPathObjectPbr* pbr, const MatpbrPathLights* lights, const void* light_tris,
                                        const float* light_cdf, const float* obj_col, const float* obj_uv, const MatpbrPathObjectTex* tex,
                                        const void* texels, long n_texels);

/* The texture lookups of a flagged object at a hit on the CPU, with the routines the kernel runs: per lane the triangle record
 * tri[N,3,3] = (v0, e1, e2), the corner coordinates uv[N,3,2] and the ray o[N,3], d[N,3]; one record `tex` (checked as a kind-3
 * object's) over the HOST buffer texels[n_texels] -> u[N], v[N], st[N,2], base[N,3], orm[N,3].  An image the record does not have gives
 * (1, 1, 1).  Four equal texels give exactly their value; every value lies in [0, 1]. */
int matpbr_path_object_texture_host(const float* tri, const float* uv, const float* o, const float* d, long N, const MatpbrPathObjectTex* tex,
                                    const void* texels, long n_texels, float* u, float* v, float* st, float* base, float* orm);

/* The tint guide of the denoiser: matpbr_path_feature_colors' ray, traversal and uncontracted barycentrics.  out[H,W,3] (DEVICE) =
 * c_vertex * c_base where the first hit lies on a coloured or textured object (a factor the object does not carry is 1), (1, 1, 1)
 * everywhere else.  obj_col, obj_uv, tex, texels, n_texels as matpbr_path_render_objects_textures takes them (the buffers DEVICE, tex
 * HOST; nullable where no object needs them).  The CPU twin gives the same bits. */
int matpbr_path_feature_tints(const void* nodes, const void* tris, int H, int W, float fov_x_deg, const MatpbrPathObject* objects, int n_objects,
                              long n_scene_tri, const float* obj_col, const float* obj_uv, const MatpbrPathObjectTex* tex, const void* texels,
                              long n_texels, float* out, void* stream);
/* matpbr_path_feature_tints on the CPU with the routine the kernel runs (every pointer HOST). */
int matpbr_path_feature_tints_host(const void* nodes, const void* tris, int H, int W, float fov_x_deg, const MatpbrPathObject* objects,
                                   int n_objects, long n_scene_tri, const float* obj_col, const float* obj_uv, const MatpbrPathObjectTex* tex,
                                   const void* texels, long n_texels, float* out);

/* The differential render ("Differential render"; Debevec 1998), forward only: what the inserted objects add to
 * and take from a photograph of the scene.  Arguments: matpbr_path_render_objects_textures' without `out`, the table checked as that
 * entry point checks it (level 7), then three sums and a count (DEVICE).  Per pixel and sample s of spp, with that render's random
 * numbers: c_s = 1 where the camera ray's closest hit is an inserted triangle (id >= n_scene_tri), else 0; L_with,s is the sample's
 * radiance as matpbr_path_render_objects_textures computes it; L_without,s is the same sample walked again from the camera ray with
 * every triangle of id >= n_scene_tri skipped by every traversal and the envmap as the only emitter.  The second walk runs only for a
 * sample with c_s = 0 that is touched: the table holds an object of kind 4, or a closest-hit or a shadow traversal of the first walk
 * returned an inserted triangle.  Outputs, each a mean over spp: fg[H,W,3] = c_s L_with,s; delta[H,W,3] = L_with,s - L_without,s over
 * the samples walked twice (an untouched sample adds nothing: delta is exactly 0 where none was); alpha[H,W] = c_s.  rewalked[H,W]
 * (nullable) has the number of second walks ADDED to it, as `rays` has the rays of both walks.  Every split into launches gives the
 * same bits.  Invalid arguments, besides that entry point's: n_objects == 0, fg, delta or alpha NULL. */
int matpbr_path_render_objects_diff(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                    float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                    int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, uint32_t* rays, void* stream,
                                    const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                    const MatpbrPathObjectPbr* pbr, const MatpbrPathLights* lights, const void* light_tris,
                                    const float* light_cdf, const float* obj_col, const float* obj_uv, const MatpbrPathObjectTex* tex,
                                    const void* texels, long n_texels, float* fg, float* delta, float* alpha, uint32_t* rewalked);

/* The differential render composited into the photograph: out[H,W,3] = max(0, (fg_sum + delta_sum) scale + (1 - alpha_sum scale) photo)
 * per channel, where the sums are matpbr_path_render_objects_diff's outputs added over some frames and scale = 1 / (their number).
 * Every product and sum is rounded on its own: where fg, delta and alpha are 0 the photograph comes through bit for bit (a photo >= 0),
 * and the CPU twin gives the same bits.  DEVICE pointers.  Invalid: a NULL pointer, H or W <= 0, scale not finite or <= 0. */
int matpbr_path_composite(const float* fg_sum, const float* delta_sum, const float* alpha_sum, const float* photo, int H, int W, float scale,
                          float* out, void* stream);
/* matpbr_path_composite on the CPU with the routine the kernel runs (every pointer HOST). */
int matpbr_path_composite_host(const float* fg_sum, const float* delta_sum, const float* alpha_sum, const float* photo, int H, int W, float scale,
                               float* out);

/* matpbr_path_trace_host over the triangles of id < n_scene_tri alone (the differential render's second walk): a triangle of a larger
 * id is skipped before its test.  any == 0: closest hit; any == 1: the shadow rays' traversal, which returns the first triangle it
 * finds (t_hit is then that triangle's distance, not the closest).  With n_scene_tri >= the mesh's triangle count and any == 0 it is
 * matpbr_path_trace_host, bit for bit.  Invalid, besides that entry point's: n_scene_tri < 0, any outside {0, 1}. */
int matpbr_path_trace_scene_host(const void* nodes, const void* tris, const float* o, const float* d, long N, float tmin, float tmax,
                                 float* t_hit, int32_t* tri_hit, long n_scene_tri, int any);

/* The differential render with the photograph seen through inserted glass ("Seen through glass"), forward only.
 * Arguments: matpbr_path_render_objects_diff's, then photo[H,W,3] (DEVICE; finite and >= 0 is the caller's contract) and
 * through[H,W,3] (DEVICE).  A sample is see-through where c_s = 1, every vertex so far was a dielectric one (kind 1, flat or smooth)
 * and the ray traced at depth k >= 1 lands on the front of a triangle of id < n_scene_tri at the point p.  It adds
 * thr_k photo[texel(p)] to `through` (thr_k: the chain's throughput; texel: the one the depth mesh's vertex reads its maps at), before
 * the max_depth test.  Where k + 1 < max_depth and the table holds an object of kind 4 or a traversal of the first walk after the
 * landing trace returned an inserted triangle, the sample is walked again from the camera ray, the same chain, with every triangle of
 * id >= n_scene_tri skipped from depth k on and the envmap as the only emitter, and fg takes L_with,s - L_tail,s; otherwise the two
 * tails are the same arithmetic and fg takes nothing, with no subtraction: such a sample is exactly thr_k photo.  A chain that ends on a miss, on another kind of object, on a light, on the sheet's back or inside the
 * glass at max_depth is not see-through, and every such sample keeps matpbr_path_render_objects_diff's rule.  through is a mean over
 * spp as fg is; delta and alpha are matpbr_path_render_objects_diff's bits; rewalked counts both kinds of second walk.  The picture
 * is matpbr_path_composite with fg + through in fg's place.  Every split into launches gives the same bits.  Invalid arguments,
 * besides that entry point's: photo or through NULL. */
int matpbr_path_render_objects_through(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                       float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                       int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, uint32_t* rays, void* stream,
                                       const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                       const MatpbrPathObjectPbr* pbr, const MatpbrPathLights* lights, const void* light_tris,
                                       const float* light_cdf, const float* obj_col, const float* obj_uv, const MatpbrPathObjectTex* tex,
                                       const void* texels, long n_texels, float* fg, float* delta, float* alpha, uint32_t* rewalked,
                                       const float* photo, float* through);
/* The differential render that also keeps the radiance without the objects ("Ratio shadow transfer"), forward
 * only.  Arguments: matpbr_path_render_objects_through's, then base[H,W,3] (DEVICE).  photo and through are both NULL or both
 * non-NULL: NULL means matpbr_path_render_objects_diff's rule for every sample, non-NULL matpbr_path_render_objects_through's.
 * base = (1 - c_s) L_without,s, a mean over spp as the other sums are: a sample with c_s = 0 adds its second walk's radiance where it
 * was walked twice, else its first walk's, which met no inserted triangle and so is the same arithmetic as a walk without them (no
 * second walk runs for it); a sample with c_s = 1 adds nothing.  base >= 0, and exactly 0 where alpha = 1.  fg, delta, alpha,
 * through and rewalked are the bits of the entry whose rule holds, and base + delta = the mean of (1 - c_s) L_with,s up to rounding.
 * The picture is matpbr_path_composite_ratio.  Every split into launches gives the same bits.  Invalid arguments, besides those
 * entry points': base NULL, exactly one of photo and through NULL. */
int matpbr_path_render_objects_ratio(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                     float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                     int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, uint32_t* rays, void* stream,
                                     const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                     const MatpbrPathObjectPbr* pbr, const MatpbrPathLights* lights, const void* light_tris,
                                     const float* light_cdf, const float* obj_col, const float* obj_uv, const MatpbrPathObjectTex* tex,
                                     const void* texels, long n_texels, float* fg, float* delta, float* alpha, uint32_t* rewalked,
                                     const float* photo, float* through, float* base);
/* The differential render composited into the photograph with its shadows transferred as a ratio ("Ratio
 * shadow transfer"): the sums are matpbr_path_render_objects_ratio's outputs added over some frames, scale = 1 / (their number),
 * K = 1 - alpha_sum scale.  Per channel, where delta_sum < 0 and base_sum > 0 (the objects darken it): B = base_sum scale,
 * D = delta_sum scale, g = max(0, B + D) / B in [0, 1], out = max(0, fg_sum scale + (K photo) g): the photograph is dimmed by the
 * share of light the model loses, so the model's albedo cancels and the photograph's texture stays.  Elsewhere (the objects brighten
 * the channel or leave it) out is matpbr_path_composite's, bit for bit: added light stays additive, its ratio having no bound where
 * base is dark.  Every operation is rounded on its own and the division is the correctly rounded one: the CPU twin gives the same
 * bits, and where fg, delta and alpha are 0 the photograph comes through bit for bit.  DEVICE pointers.  Invalid: a NULL pointer, H
 * or W <= 0, scale not finite or <= 0. */
int matpbr_path_composite_ratio(const float* fg_sum, const float* delta_sum, const float* base_sum, const float* alpha_sum, const float* photo, int H,
                                int W, float scale, float* out, void* stream);
/* matpbr_path_composite_ratio on the CPU with the routine the kernel runs (every pointer HOST). */
int matpbr_path_composite_ratio_host(const float* fg_sum, const float* delta_sum, const float* base_sum, const float* alpha_sum, const float* photo,
                                     int H, int W, float scale, float* out);
/* The camera chain of matpbr_path_render_objects_through on the CPU (every pointer HOST), from the routines the kernel runs: the
 * traversal of matpbr_path_trace_host, the dielectric samplers, the spawn offset and the texel lookup.  Lane l is sample sample[l] of
 * pixel pixel[l] (a flat index into [H,W]) under seed seed[l].  objects, obj_nrm (nullable where no object is smooth) and n_scene_tri
 * as the render takes them; the table may hold every kind and flag, and the chain reads the kind, the smooth flag and a dielectric's p.
 * depth[l] = the landing depth k, -1 where the sample is not see-through; texel[l] = the flat texel the landing point projects to;
 * thr[l,3] = thr_k; o[l,3], d[l,3] = the ray traced at depth k (-1 and zeros where depth is -1).  Invalid: a NULL pointer other than
 * obj_nrm, N < 0, H or W <= 0, a bad fov, max_depth outside 1..16, n_objects == 0, a bad table, a pixel outside the image, a
 * negative sample. */
int matpbr_path_through_chain_host(const void* nodes, const void* tris, int H, int W, float fov_x_deg, int max_depth,
                                   const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                   const int32_t* pixel, const uint32_t* seed, const int32_t* sample, long N, int32_t* depth, int32_t* texel,
                                   float* thr, float* o, float* d);

/* matpbr_path_render with the depth mesh shading as TransBSDF (myutils/mi_plugin.py:1477-1771), forward only.  mask[H,W] (uint8,
 * DEVICE, non-zero = edited) and bg[H,W,3] (fp32, DEVICE, the photograph seen through the glass) are read by the enqueued work;
 * `edit` is HOST memory, copied before the call returns.  Where the texel a vertex reads is masked, the BSDF is the glass of
 * DESIGN.md section 1.4 over bg at the refracted texel; elsewhere it is matpbr_path_render's value, and at every vertex the pdf
 * clamps VoH at 1e-4 and the sample weight is f / (pdf + 1e-4).  Invalid arguments: ior <= 0, spec_trans outside [0, 1], a negative
 * or non-finite refract_distance, a null mask or bg.  There is no variant with inserted objects. */
int matpbr_path_render_trans(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                             float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                             int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream,
                             const uint8_t* mask, const float* bg, const MatpbrPathTransEdit* edit);

/* matpbr_path_render with a shading-normal map ("Shading normals").  nrm[H,W,3] (fp32, DEVICE, unit length,
 * used as given) is read at the texel a vertex reads its material from and takes the place of MatDiffBSDF's `normal`: every cosine
 * of the BSDF, both samplers' frames, the pdf.  The face normal keeps the back-face test and the spawn offset, and a direction on
 * its far side carries nothing: an emitter sample there traces no shadow ray, a BSDF sample there ends the path.  With nrm == NULL
 * this is matpbr_path_render, bit for bit, and launches its kernel.  There is no variant with inserted objects or with the
 * transparency edit. */
int matpbr_path_render_normals(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                               float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                               int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream,
                               const float* nrm);

/* d (g . f) / d n of the BSDF value f (RGB, with its cosine) at N lanes on the CPU: n[N,3], wo[N,3], wi[N,3], a[N,3], r[N], m[N],
 * upstream g[N,3] -> d_n[N,3] = gl wi + gv wo + gh h, h = normalize(wi + wo), each cosine's gradient passed where the raw cosine is
 * positive, with respect to the three components of n as free variables.  The gates and the composition are the routine the
 * backward kernel runs; gl, gv, gh restate the device's cosine gradients with plain divisions. */
int matpbr_path_eval_normal_grad_host(const float* n, const float* wo, const float* wi, const float* a, const float* r, const float* m,
                                      const float* g, long N, float* d_n);

/* The masked branch of the edited BSDF on the CPU, with the routine the kernel runs: per lane the face normal n[N,3], wo[N,3] towards
 * the viewer, wi[N,3] towards the light (either side of the surface), the texel's a[N,3] r[N] m[N] and bg[N,3] at the refracted
 * texel -> f[N,3] (with its cosine) and pdf[N]. */
int matpbr_path_trans_eval_host(const MatpbrPathTransEdit* edit, const float* n, const float* wo, const float* wi, const float* a,
                                const float* r, const float* m, const float* bg, long N, float* f, float* pdf);

/* The edit's texel lookups on the CPU, with the routine the kernel runs: hit points p[N,3], face normals n[N,3], wo[N,3] in an
 * H x W image -> texel[N] (the point's own, row * W + col) and texel_refracted[N] (where bg is read). */
int matpbr_path_trans_lookup_host(const MatpbrPathTransEdit* edit, const float* p, const float* n, const float* wo, long N, int H, int W,
                                  float fov_x_deg, int32_t* texel, int32_t* texel_refracted);

/* Workspace of matpbr_path_render_bwd for an H x W image and an He x We envmap, in bytes (0 for a non-positive size). */
size_t matpbr_path_render_bwd_workspace_bytes(int H, int W, int He, int We);

/* The backward pass of matpbr_path_render with the same arguments (`spp`, `max_depth`, `seed`, `spp_per_launch` mean the same):
 * the exact derivative of the fixed-seed estimator with the sampling detached: directions, pdfs, MIS
 * weights, lobe choices and the envmap tables are constants; the gradient flows through the BSDF value at every vertex, to the
 * texel the vertex reads its material from, and through the envmap texels.  d_out[H,W,3] = d loss / d out.  The gradients are
 * ADDED to d_a[H,W,3], d_r[H,W,1], d_m[H,W,1], d_env[He,We,3] (device pointers); a null one is not computed and its buffer is not
 * touched.  Sums are 64-bit fixed point: the result is bit-identical from run to run and for every `spp_per_launch`.  d_env needs
 * He * We <= MATPBR_PATH_BWD_MAX_ENV_TEXELS.  `workspace`: device memory of matpbr_path_render_bwd_workspace_bytes(H, W, He, We)
 * bytes, 8-byte aligned, used by the enqueued work until it has run.  `rays` (nullable, [H,W]): the rays both replays of each
 * pixel traced are ADDED to it.  d_out must be finite. */
int matpbr_path_render_bwd(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W, float fov_x_deg,
                           const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He, int We, int spp,
                           int max_depth, uint32_t seed, int spp_per_launch, const float* d_out, float* d_a, float* d_r, float* d_m,
                           float* d_env, void* workspace, size_t workspace_bytes, uint32_t* rays, void* stream);

/* Workspace of matpbr_path_render_bwd_normals with a normal map: three more accumulators per pixel. */
size_t matpbr_path_render_bwd_normals_workspace_bytes(int H, int W, int He, int We);

/* The backward pass of matpbr_path_render_normals: matpbr_path_render_bwd's arguments, the map nrm[H,W,3] (DEVICE) and d_n[H,W,3]
 * (DEVICE, nullable: not computed, not touched), to which d loss / d nrm is ADDED.  The sampling stays detached; at every vertex
 * both BSDF values (the emitter term's and the sample factor's) send gl wi + gv wo + gh h to the texel the vertex reads, with
 * the upstreams of matpbr_path_render_bwd and the gates of matpbr_path_eval_normal_grad_host.  The gradient is with respect to the
 * three components as free variables: normalising is the caller's.  Same fixed-point sums, same bit-identity.  `workspace` holds
 * matpbr_path_render_bwd_normals_workspace_bytes(H, W, He, We) bytes.  With nrm == NULL, d_n must be NULL, the workspace of
 * matpbr_path_render_bwd suffices, and this is matpbr_path_render_bwd, bit for bit. */
int matpbr_path_render_bwd_normals(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                   float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                   int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, const float* d_out, float* d_a, float* d_r,
                                   float* d_m, float* d_env, void* workspace, size_t workspace_bytes, uint32_t* rays, void* stream,
                                   const float* nrm, float* d_n);

/* ---- Denoiser ("Denoiser"): first-hit features and a variance-guided edge-avoiding a-trous filter ----------
 * Forward only, deterministic (no atomics), opt-in.  All images fp32, contiguous, HWC.
 *   A, B [H,W,3]   two renders of the same scene with independent seeds and the same sample count, finite
 *   geom [H,W,8]   two float4 per pixel, (px, py, pz, rho) and (nx, ny, nz, id), of the camera ray through the pixel centre: p the
 *                  first hit, rho = |p| 2 tan(fov_x / 2) / W the pixel's footprint there, n the unit normal matpbr_path_render* shades
 *                  that camera vertex with, id (a float) -1 = no hit (p = n = 0, rho = 0), 0 = the depth mesh, 1 + k = object k
 *   alb [H,W,3]    the albedo guide (the caller composes it)
 *   cv [H,W,4]     (colour, variance of the colour's luminance): what the levels pass on
 * prepare: c0 = (A + B) / 2; v0 = the 3 x 3 binomial average [1 2 1] x [1 2 1] of (lum(A) - lum(B))^2 / 4 over the taps inside the image
 * with the pixel's id, normalised by the weights used; lum = 0.2126 R + 0.7152 G + 0.0722 B.
 * level l: stride s = 2^l, taps q = p + s (i, j), i, j in -2..2, those outside the image skipped, h = (1/16, 1/4, 3/8, 1/4, 1/16); the
 * centre weighs 9/64, every other tap w = h_i h_j [id_q == id_p] w_n w_x w_a w_c,
 *   w_n = max(0, n_p . n_q)^sigma_n                                                        (1 where id_p == -1)
 *   w_x = exp(-|n_p . (x_q - x_p)| / (sigma_x rho_p s sqrt(i^2 + j^2) + 1e-30))             (1 where id_p == -1)
 *   w_a = exp(-|alb_p - alb_q|^2 / sigma_a^2)
 *   w_c = exp(-|lum(c_p) - lum(c_q)| / (sigma_c sqrt(max(v_p, 0)) + 1e-3 lum(c_p) + 1e-30))
 * and c' = sum w c_q / sum w, v' = sum w^2 v_q / (sum w)^2.  The output is the colour after `levels` levels. */
typedef struct MatpbrPathDenoise {
    int32_t levels;                              /* 1..8 (5) */
    float sigma_n, sigma_x, sigma_a, sigma_c;    /* finite and > 0 (32, 1, 0.1, 4) */
} MatpbrPathDenoise;

/* geom of an H x W camera (matpbr_path_render's) over a BVH: one lane per pixel traces one closest-hit ray through the pixel centre.
 * objects[n_objects] (HOST, copied before the call returns), obj_nrm (DEVICE, nullable unless an object is smooth) and n_scene_tri as
 * matpbr_path_render_objects_normals takes them (an object may also be of kind MATPBR_PATH_BSDF_PBR or MATPBR_PATH_BSDF_AREA: the
 * features need its kind and its smooth flag only, and take no records or light tables; a light has id 1 + k and its face normal); with n_objects == 0 they may be null / 0.  nrm_map (DEVICE, nullable): the
 * shading-normal map of matpbr_path_render_normals, read at the texel the hit point projects to.  geom: DEVICE, 16-byte aligned. */
int matpbr_path_features(const void* nodes, const void* tris, int H, int W, float fov_x_deg, const MatpbrPathObject* objects, int n_objects,
                         const float* obj_nrm, long n_scene_tri, const float* nrm_map, float* geom, void* stream);
/* matpbr_path_features on the CPU with the routine the kernel runs (every pointer HOST). */
int matpbr_path_features_host(const void* nodes, const void* tris, int H, int W, float fov_x_deg, const MatpbrPathObject* objects, int n_objects,
                              const float* obj_nrm, long n_scene_tri, const float* nrm_map, float* geom);

/* The steps on their own (DEVICE pointers, 16-byte aligned cv and geom; `prm` HOST, copied before the call returns).  `level` in
 * 0..7; cv_out must not be cv_in.  Invalid argument: a null pointer, `levels` outside 1..8, a sigma that is not finite and > 0. */
int matpbr_path_denoise_prepare(const float* A, const float* B, const float* geom, int H, int W, float* cv0, void* stream);
int matpbr_path_denoise_level(const float* cv_in, const float* geom, const float* alb, int H, int W, const MatpbrPathDenoise* prm, int level,
                              float* cv_out, void* stream);
/* The same steps on the CPU with the per-pixel routines the kernels run (every pointer HOST). */
int matpbr_path_denoise_prepare_host(const float* A, const float* B, const float* geom, int H, int W, float* cv0);
int matpbr_path_denoise_level_host(const float* cv_in, const float* geom, const float* alb, int H, int W, const MatpbrPathDenoise* prm, int level,
                                   float* cv_out);

/* Workspace of matpbr_path_denoise: two [H,W,4] buffers, in bytes (0 for a non-positive size). */
size_t matpbr_path_denoise_workspace_bytes(int H, int W);
/* The chain: prepare, then `levels` levels ping-ponging in `workspace` (DEVICE, 16-byte aligned, used by the enqueued work until it has
 * run); the last level writes its colour to out[H,W,3].  Equal to the separate calls bit for bit. */
int matpbr_path_denoise(const float* A, const float* B, const float* geom, const float* alb, int H, int W, const MatpbrPathDenoise* prm, float* out,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- Denoiser for the differential render: the a-trous filter over matpbr_path_render_objects_diff's outputs ----
 * Forward only, deterministic (no atomics), opt-in; added at version 3.  fgA, deltaA [H,W,3], alphaA [H,W] and the same for B: two sums
 * of that entry point's outputs over the same number of frames, with independent seeds and equal spp; scale = 1 / (frames summed per
 * half), finite and > 0; geom, alb and prm as matpbr_path_denoise takes them.
 * A pixel's own layer is the object layer where id >= 1, else the scene layer.  abar = (0.5 (alphaA + alphaB)) scale; the own layer's
 * coverage k is abar (object) or max(0, 1 - abar) (scene), its signal X is fg (object) or delta (scene); the other layer's signal and
 * alpha are never filtered.
 * prepare: g = scale / k; c0 = (0.5 (X_A + X_B)) g; v0 = the 3 x 3 binomial average of ((lum(X_A) - lum(X_B))^2 / 4) g_q^2 over the taps
 * inside the image with the pixel's id and k_q > 0, normalised by the weights used; where k = 0, (c0, v0) = 0 and no quotient is
 * formed.  cov[H,W] = k.
 * level l: matpbr_path_denoise_level's with every tap weight, the centre's 9/64 included, multiplied by k_q, and
 *   w_c = exp(-|lum(c_p) - lum(c_q)| / (sigma_c sqrt(max(v_p, 0)) + 1e-3 |lum(c_p)| + 1e-30));
 * a pixel with k = 0 gives (0, 0, 0, 0).
 * finish: own = k c_L; fg' = own on object pixels, else (0.5 (fgA + fgB)) scale; delta' = own on scene pixels, else
 * (0.5 (deltaA + deltaB)) scale; alpha' = abar.  The picture is matpbr_path_composite(fg', delta', alpha', photo, 1).
 * Where deltaA and deltaB are exactly 0 within Chebyshev distance 2 (2^levels - 1) + 1 of a scene pixel, delta' there is +0.
 * DEVICE pointers, cv and geom 16-byte aligned; `prm` HOST.  Invalid argument: a null pointer, H or W <= 0, a bad prm, a level outside
 * 0..7, a scale that is not finite and > 0, cv_out == cv_in. */
int matpbr_path_denoise_diff_prepare(const float* fgA, const float* deltaA, const float* alphaA, const float* fgB, const float* deltaB,
                                     const float* alphaB, const float* geom, int H, int W, float scale, float* cv0, float* cov, void* stream);
int matpbr_path_denoise_diff_level(const float* cv_in, const float* cov, const float* geom, const float* alb, int H, int W,
                                   const MatpbrPathDenoise* prm, int level, float* cv_out, void* stream);
int matpbr_path_denoise_diff_finish(const float* cv, const float* cov, const float* fgA, const float* deltaA, const float* alphaA, const float* fgB,
                                    const float* deltaB, const float* alphaB, const float* geom, int H, int W, float scale, float* fg, float* delta,
                                    float* alpha, void* stream);
/* The same steps on the CPU with the per-pixel routines the kernels run (every pointer HOST). */
int matpbr_path_denoise_diff_prepare_host(const float* fgA, const float* deltaA, const float* alphaA, const float* fgB, const float* deltaB,
                                          const float* alphaB, const float* geom, int H, int W, float scale, float* cv0, float* cov);
int matpbr_path_denoise_diff_level_host(const float* cv_in, const float* cov, const float* geom, const float* alb, int H, int W,
                                        const MatpbrPathDenoise* prm, int level, float* cv_out);
int matpbr_path_denoise_diff_finish_host(const float* cv, const float* cov, const float* fgA, const float* deltaA, const float* alphaA,
                                         const float* fgB, const float* deltaB, const float* alphaB, const float* geom, int H, int W, float scale,
                                         float* fg, float* delta, float* alpha);

/* Workspace of matpbr_path_denoise_diff: two [H,W,4] buffers and cov[H,W], in bytes (0 for a non-positive size). */
size_t matpbr_path_denoise_diff_workspace_bytes(int H, int W);
/* The chain: prepare, `levels` levels ping-ponging in `workspace` (16-byte aligned, used by the enqueued work until it has run), finish
 * -> fg[H,W,3], delta[H,W,3], alpha[H,W].  Equal to the separate calls bit for bit.  The _host twin takes HOST pointers throughout. */
int matpbr_path_denoise_diff(const float* fgA, const float* deltaA, const float* alphaA, const float* fgB, const float* deltaB, const float* alphaB,
                             const float* geom, const float* alb, int H, int W, float scale, const MatpbrPathDenoise* prm, float* fg, float* delta,
                             float* alpha, void* workspace, size_t workspace_bytes, void* stream);
int matpbr_path_denoise_diff_host(const float* fgA, const float* deltaA, const float* alphaA, const float* fgB, const float* deltaB,
                                  const float* alphaB, const float* geom, const float* alb, int H, int W, float scale, const MatpbrPathDenoise* prm,
                                  float* fg, float* delta, float* alpha, void* workspace, size_t workspace_bytes);

/* ---- Moving inserted objects ("Moving inserted objects"): a grafted BVH whose object side is moved and refitted
 * on the device from a rest pose; added at version 3.  The render, feature, denoise and composite entry points take the moved buffers as
 * they take any: the node, triangle, corner-normal and light-record layouts are the ones above. */

/* The pose of one object, a similarity p' = R (s (p - c)) + c + t: R row-major, rows orthonormal to 1e-5 with det > 0 (no mirror: it would
 * flip the winding), s > 0, everything finite.  Exactly (R = 1, s = 1, t = 0) leaves the object at rest: its records are copied.  Corner
 * normals turn by R alone and are not renormalised, which the 1e-5 covers: |R n| stays within 2e-5 of 1 and every reader of the corner
 * normals normalises after interpolating. */
typedef struct MatpbrPathXform {
    float R[9];
    float s;
    float t[3];
    float c[3];
} MatpbrPathXform;

/* matpbr_path_bvh_build_objects with the two sides kept apart.  Node 0 is the graft root: slot 0 the depth mesh's subtree (triangles
 * [0, n_scene_tri), at least one, which name vertices below n_scene_vert alone: the depth mesh's own, referenced or not), slot 1 the inserted triangles' ([n_scene_tri, n_tri), at least one); a side of 4 triangles or fewer is the slot's
 * leaf.  The nodes follow as [scene nodes][object nodes] from *first_object_node on, a child always behind its parent; `tris` is [scene
 * triangles in their leaf order][object triangles in theirs], ids the merged mesh's.  Each side is built by matpbr_path_bvh_build's
 * builder capped one level lower, so *depth <= MATPBR_PATH_MAX_BVH_DEPTH; the scene side's topology and boxes are those of
 * matpbr_path_bvh_build over the scene alone, renumbered (where that build stays above level 40).  rest_tris[n_tri - n_scene_tri]: the
 * object triangles' records, the rest pose every move starts from.  node_level[max_nodes]: the level of each object node (the object
 * subtree's root is 1), *object_depth the deepest slot level of that side.  *pad = 1e-6 S, S the largest coordinate magnitude of the mesh
 * and `reach` (>= 0: the largest any later pose will have).  The object side's boxes are matpbr_path_objects_move's refit of the rest
 * pose: a move by the identity reproduces this build byte for byte.  max_nodes >= 1 + max(1, n_scene_tri) + max(1, n_tri - n_scene_tri).
 * Host only. */
int matpbr_path_bvh_build_grafted(const double* vert, long n_vert, long n_scene_vert, const int32_t* tri, long n_tri, long n_scene_tri, double reach,
                                  void* nodes, long max_nodes, void* tris, void* rest_tris, int32_t* node_level, long* n_nodes, int* depth, long* n_leaves,
                                  long* first_object_node, int* object_depth, float* pad);

/* 0 when matpbr_path_objects_move would take every one of xform[n_objects] (HOST), else MATPBR_PATH_ERR_INVALID_ARG. */
int matpbr_path_xform_check_host(const MatpbrPathXform* xform, int n_objects);

/* Moves the objects of a grafted BVH to the poses xform[n_objects] (HOST, copied before return; object k's is xform[k]) and refits the
 * object nodes, always from the rest pose.  Triangle k of the object side: tris[n_scene_tri + k] = (v0', id) (e1', 0) (e2', 0) of
 * rest_tris[k], v0' = p'(v0), e' = R (s e), evaluated in fp64 and rounded once; a smooth object's corner normals obj_nrm = R rest_nrm (both
 * [n_object_tri,3,3], input order; NULL when no object is smooth); the light records light_tris = the same transform of rest_light_tris
 * (both [n_light_tri,3] float4, `lights` the header they came with, HOST; NULL and 0 without lights), bit-equal to the moved triangles of
 * the same ids.  Refit: a leaf slot's box is the min / max over its triangles of v0', fl(v0' + e1'), fl(v0' + e2') in fp32 widened by pad,
 * an inner slot's the union of its child's two boxes, bottom-up by node_level[n_object_nodes] (DEVICE) from object_depth, slot 1 of node
 * 0 last.  The scene's nodes and triangles are not written.  The caller keeps every pose within the reach pad was built for and scales
 * lights->area by s^2.  DEVICE pointers, nodes / tris / rest_tris / the light records 16-byte aligned; two launches on `stream`.  Invalid
 * argument: a null or misaligned pointer, a range outside the object triangles or overlapping another, a bad xform, a smooth object
 * without both normal buffers, a header that does not match the table.  The _host twin takes HOST pointers and gives the same bytes. */
int matpbr_path_objects_move(void* nodes, void* tris, const void* rest_tris, long n_scene_tri, long n_object_tri, long first_object_node,
                             long n_object_nodes, const int32_t* node_level, int object_depth, const MatpbrPathObject* objects, int n_objects,
                             const MatpbrPathXform* xform, float pad, const float* rest_nrm, float* obj_nrm, const void* rest_light_tris,
                             void* light_tris, long n_light_tri, const MatpbrPathLights* lights, void* stream);
int matpbr_path_objects_move_host(void* nodes, void* tris, const void* rest_tris, long n_scene_tri, long n_object_tri, long first_object_node,
                                  long n_object_nodes, const int32_t* node_level, int object_depth, const MatpbrPathObject* objects, int n_objects,
                                  const MatpbrPathXform* xform, float pad, const float* rest_nrm, float* obj_nrm, const void* rest_light_tris,
                                  void* light_tris, long n_light_tri, const MatpbrPathLights* lights);

/* ---- Media inside glass ("Media inside glass"): a homogeneous absorbing and scattering medium behind the
 * interface of an object of kind 1 or 5 whose kind carries MATPBR_PATH_OBJECT_MEDIUM; forward only; added at version 3.
 * The path carries one integer med, an object index or -1 (-1 at the camera).  After the BSDF sample at a vertex on a flagged object k,
 * med = k where ng . wi < 0 (ng the outward face normal: the ray leaves into the object), else -1; a vertex on anything else leaves med
 * as it is; a traversal that skips the inserted triangles reads med as -1; a ray that escapes with med >= 0 (an open mesh) takes the
 * envmap unattenuated.  A segment with med >= 0 whose trace hit at t: where sigma_s > 0, s = -logf(1 - u9) / sigma_s (u9: dim 9 of the
 * depth; dims 9-11 are the medium's) and, where s < t, the depth is a medium vertex at o + s d: thr[c] *= expf(-sigma_a[c] s), the
 * max_depth test as at a surface, no emitter sample, the new direction from Henyey-Greenstein about d by dims 10, 11 with weight 1
 * (|g| < 1e-3: cos = 1 - 2 u, else cos = (1 + g^2 - ((1 - g^2) / (1 - g + 2 g u))^2) / (2 g); phi = 2 pi u; the diffuse sampler's frame),
 * no spawn offset, med unchanged, and whatever the ray meets next takes MIS weight 1.  Otherwise thr[c] *= expf(-sigma_a[c] t) and the
 * surface vertex runs as without a medium. */

/* matpbr_path_render_objects_textures where an object of kind 1 or 5 may carry MATPBR_PATH_OBJECT_MEDIUM (with or without the smooth
 * flag).  media (HOST, one record per object, copied before the call returns).  This is level 8 of the table in DESIGN.md section 1.4,
 * "The object entries": without a flagged object it launches matpbr_path_render_objects_textures' kernel choice and gives its bits
 * (media may be NULL then), and so it does where no flagged object's record has a coefficient above 0 (such a medium multiplies by
 * exactly 1: the table is walked without the flag).  Invalid arguments, besides that entry point's: the flag on kind 2, 3 or 4, a flagged object with media ==
 * NULL or with a record that is not valid (MatpbrPathObjectMedium). */
int matpbr_path_render_objects_media(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                     float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                     int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, float* out, uint32_t* rays, void* stream,
                                     const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                     const MatpbrPathObjectPbr* pbr, const MatpbrPathLights* lights, const void* light_tris,
                                     const float* light_cdf, const float* obj_col, const float* obj_uv, const MatpbrPathObjectTex* tex,
                                     const void* texels, long n_texels, const MatpbrPathObjectMedium* media);

/* The differential family with media: matpbr_path_render_objects_ratio's arguments, then media as above.  photo and through are both
 * NULL or both non-NULL, and base may be NULL as well: the four shapes are matpbr_path_render_objects_diff (neither), _through (photo),
 * _ratio without and with photo (base).  Without a flagged object, or where no flagged object's record has a coefficient above 0, it
 * launches the existing kernel of the same shape and gives its bits.  With one: trip 0's records (c_s, touched, the chain, the landing) are taken after the scatter decision and only where the
 * segment reached its hit; a medium vertex ends the see-through chain; the segment's attenuation is in thr_k before thr_k photo[texel]
 * is added to `through`; a segment that reaches a triangle of id < n_scene_tri with med >= 0 (a mesh that pokes through the scene)
 * touches the sample.  A pixel that no sample touches keeps the photograph's bits.  Invalid arguments, besides
 * matpbr_path_render_objects_ratio's (base aside) and matpbr_path_render_objects_media's: exactly one of photo and through NULL. */
int matpbr_path_render_objects_diff_media(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                          float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                          int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, uint32_t* rays, void* stream,
                                          const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                          const MatpbrPathObjectPbr* pbr, const MatpbrPathLights* lights, const void* light_tris,
                                          const float* light_cdf, const float* obj_col, const float* obj_uv, const MatpbrPathObjectTex* tex,
                                          const void* texels, long n_texels, float* fg, float* delta, float* alpha, uint32_t* rewalked,
                                          const float* photo, float* through, float* base, const MatpbrPathObjectMedium* media);

/* ---- Reflected in inserted objects ("Reflected in inserted objects"): the see-through rule along chains that
 * pass objects whose kind carries MATPBR_PATH_OBJECT_PHOTO; forward only; added at version 3. */

/* matpbr_path_render_objects_diff_media with photo and through required (base and media nullable with that entry's meaning), where an
 * object of kind 2, 3 or 5 may carry MATPBR_PATH_OBJECT_PHOTO.  Level 9 of the table in DESIGN.md section 1.4, "The object entries":
 * without a flagged object it launches the existing kernel of the same shape and gives its bits.  With one, the walk is that
 * entry's but for the chain: a vertex keeps the chain alive where its object is of kind 1 or carries the flag (a medium vertex still
 * ends it).  A flagged vertex is not delta: its emitter sample, with shadow ray and MIS weight, is taken as ever and stays in the
 * sample's radiance, and so do the envmap a chain ray escapes to and the light it meets; a flagged vertex whose path ends (a one-sided
 * back hit, a kind-3 sample below the face, a throughput of zero) does not land.  The landing is unchanged: depth k >= 1, the front of
 * a triangle of id < n_scene_tri, thr_k photo[texel(p)] added to `through` before the max_depth test, thr_k now with the flagged
 * vertices' weights f cos / pdf and no MIS weight (the depth mesh is no emitter).  With L_chain,s the radiance gathered at depths below
 * k, a see-through sample adds fg_s = L_chain,s + (L_tailwith,s - L_tail,s): the bracket only where the touch rule asks for the second
 * walk, else L_chain,s exactly.  The second walk replays the chain with the same dims 6, 7, 8 over every triangle and takes no emitter
 * sample (and traces no shadow ray) at depths below k; from k on it is matpbr_path_render_objects_through's.  The photograph gives the
 * radiance p sends to the camera and is used for whatever direction the chain arrives from: the diffuse assumption of "Seen through
 * glass".  delta, alpha and base are the unflagged table's bits; rewalked counts both kinds of second walk.  Every split into launches
 * gives the same bits.  Invalid arguments, besides that entry point's: photo or through NULL, the flag on kind 1 or 4. */
int matpbr_path_render_objects_reflect(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                       float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                       int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, uint32_t* rays, void* stream,
                                       const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                       const MatpbrPathObjectPbr* pbr, const MatpbrPathLights* lights, const void* light_tris,
                                       const float* light_cdf, const float* obj_col, const float* obj_uv, const MatpbrPathObjectTex* tex,
                                       const void* texels, long n_texels, float* fg, float* delta, float* alpha, uint32_t* rewalked,
                                       const float* photo, float* through, float* base, const MatpbrPathObjectMedium* media);

/* The camera chain of matpbr_path_render_objects_reflect on the CPU (every pointer HOST): matpbr_path_through_chain_host's arguments
 * with pbr (one record per object, nullable where no flagged object is of kind 3) after n_scene_tri, and its outputs.  One body serves
 * both: on a table without the flag the two give the same bits.  A flagged vertex runs the samplers the kernel runs (the diffuse and
 * the rough dielectric one, about the interpolated normal where the object is smooth); at kind 3 the depth mesh's sampler is restated
 * with plain divisions and square roots, the device's being hardware instructions, so thr agrees with the kernel's to rounding, not to
 * the bit.  A flagged object may not carry the colour or the texture flag here, and no object a medium.  Invalid: that entry's, a
 * flagged object of kind 1 or 4, a flagged coloured or textured object, a flagged object of kind 3 with pbr NULL or a bad record. */
int matpbr_path_reflect_chain_host(const void* nodes, const void* tris, int H, int W, float fov_x_deg, int max_depth,
                                   const MatpbrPathObject* objects, int n_objects, const float* obj_nrm, long n_scene_tri,
                                   const MatpbrPathObjectPbr* pbr, const int32_t* pixel, const uint32_t* seed, const int32_t* sample, long N,
                                   int32_t* depth, int32_t* texel, float* thr, float* o, float* d);

/* ---- Material edits in the photograph ("Material edits in the photograph"): the differential render of edited
 * maps; no inserted objects, the envmap the only emitter; forward only; added at version 3. */

/* matpbr_path_render's arguments up to spp_per_launch (a, r, m: the fitted maps), rays and stream as there, then the edited maps
 * a_e[H,W,3], r_e[H,W], m_e[H,W], mask[H,W] (uint8, non-zero = edited), nrm[H,W,3] (nullable: the shading-normal map of
 * matpbr_path_render_normals, which is not edited), and the outputs delta[H,W,3], base[H,W,3], rewalked[H,W] (nullable, added to).
 * Every pointer DEVICE.  Sample s of a pixel is walked as matpbr_path_render (matpbr_path_render_normals) walks it, but a vertex
 * whose texel is masked reads its material from the edited maps; the first such read marks the sample touched.  A touched sample
 * is walked again from the camera ray on, with the same random numbers, on the fitted maps alone.  delta = the mean over spp of
 * (first walk - second walk) of the touched samples; base = the mean over spp of the radiance on the fitted maps of every sample,
 * the second walk's or the only one's (no subtraction is performed for an untouched sample); rewalked counts the second walks.
 * Where rewalked is 0, delta has all-zero bits.  base + delta is the edited scene's radiance.  The first walk samples by the edited
 * maps, so the two walks may part at the first masked vertex.  The pictures are matpbr_path_composite (fg and alpha zero) and
 * matpbr_path_composite_ratio.  Every split into launches gives the same bits.  Invalid arguments, besides matpbr_path_render's:
 * a NULL edited map, mask, delta or base. */
int matpbr_path_render_edit_diff(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                                 float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                                 int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, uint32_t* rays, void* stream,
                                 const float* a_e, const float* r_e, const float* m_e, const uint8_t* mask, const float* nrm, float* delta,
                                 float* base, uint32_t* rewalked);

/* ---- Relighting in the photograph ("Relighting in the photograph"): one walk under two environments and the
 * quotient composite; no inserted objects, the envmaps the only emitters; forward only; added at version 3. */

/* matpbr_path_render's arguments up to spp_per_launch (env and its tables: environment A, the fitted light), rays and stream as
 * there, then environment B, the new light, with its own size and its own tables of matpbr_path_env_tables: env_b[He_b,We_b,3],
 * row_cdf_b[He_b+1], col_cdf_b[He_b,We_b+1], env_pdf_b[He_b,We_b]; nrm[H,W,3] (nullable: the shading-normal map of
 * matpbr_path_render_normals); and the outputs base[H,W,3], relit[H,W,3].  Every pointer DEVICE.  Sample s of a pixel is walked
 * once, as matpbr_path_render (matpbr_path_render_normals) walks it: no decision of that walk reads the envmap.  At every vertex the
 * emitter sample is taken once per environment that has tables (row_cdf[He] > 0), from the same dims 2-5, each with its own shadow
 * ray and MIS weight; at an escape each environment is read at its own texel with its own MIS weight.  base = the mean over spp of
 * the radiance under A, relit = under B: each is what matpbr_path_render gives with that environment, up to the rounding of its
 * sums.  The instructions that read an environment are the same for A and B, so where B is A (the same values, the pointers may
 * differ) relit has base's bits.  rays counts the closest-hit rays once and each environment's shadow rays.  Every split into
 * launches gives the same bits.  Invalid arguments, besides matpbr_path_render's: a NULL env_b, row_cdf_b, col_cdf_b, env_pdf_b,
 * base or relit, He_b or We_b <= 0. */
int matpbr_path_render_relight(const void* nodes, const void* tris, const float* a, const float* r, const float* m, int H, int W,
                               float fov_x_deg, const float* env, const float* row_cdf, const float* col_cdf, const float* env_pdf, int He,
                               int We, int spp, int max_depth, uint32_t seed, int spp_per_launch, uint32_t* rays, void* stream,
                               const float* env_b, const float* row_cdf_b, const float* col_cdf_b, const float* env_pdf_b, int He_b, int We_b,
                               const float* nrm, float* base, float* relit);
/* The quotient image: the sums are matpbr_path_render_relight's outputs added over some frames, scale = 1 / (their number).  Per
 * channel B0 = base_sum scale, B1 = relit_sum scale, g = (B1 + floor) / (B0 + floor), out = max(0, photo g): the photograph times
 * the model's radiance under the new light over that under the fitted one, in which the model's albedo cancels to first order.
 * floor > 0 bounds the quotient where the model is dark: g <= (B1 + floor) / floor.  Every operation is rounded on its own and the
 * division is the correctly rounded one: the CPU twin gives the same bits, and where relit_sum has base_sum's bits g is exactly 1 and
 * the photograph (>= 0) comes through bit for bit.  DEVICE pointers.  Invalid: a NULL pointer, H or W <= 0, scale or floor not
 * finite or <= 0. */
int matpbr_path_composite_relight(const float* base_sum, const float* relit_sum, const float* photo, int H, int W, float scale, float floor,
                                  float* out, void* stream);
/* matpbr_path_composite_relight on the CPU with the routine the kernel runs (every pointer HOST). */
int matpbr_path_composite_relight_host(const float* base_sum, const float* relit_sum, const float* photo, int H, int W, float scale, float floor,
                                       float* out);

/* One segment inside a medium on the CPU, with the routine the kernel runs: the record `medium` (checked), per lane the traced
 * distance t[N] and u9[N] -> scattered[N] (1: the segment ends at a medium vertex), dist[N] (s there, else t), weight[N,3] =
 * expf(-sigma_a dist).  u9 is read only where sigma_s > 0. */
int matpbr_path_medium_segment_host(const MatpbrPathObjectMedium* medium, const float* t, const float* u9, long N, int32_t* scattered,
                                    float* dist, float* weight);

/* The phase sampler on the CPU, with the routine the kernel runs: g (|g| <= 0.99), propagation directions d[N,3] (unit length),
 * u[N,2] = dims 10, 11 -> wi[N,3]. */
int matpbr_path_phase_sample_host(float g, const float* d, const float* u, long N, float* wi);

#ifdef __cplusplus
}
#endif

#endif /* MATPBR_PATH_H */
