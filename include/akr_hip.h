/*
 * akr_hip.h — C-ABI drop-in boundary of the MI355X (gfx950) ray-scene intersection and
 * unidirectional path-tracing backend for AkariRender.
 *
 * Plain pointers and sizes only; no C++ or torch types cross this boundary.  Every export
 * returns an int status (0 = ok) and never throws or aborts across the ABI; the message of the
 * last failure on a context is available from akr_hip_last_error().  The C++ host adapter
 * (akarirender-1_amd/csrc/akari_hip.hpp) turns a non-zero status into std::runtime_error, the
 * reference's AKR_ASSERT_THROW convention (src/akari/common/panic.h:52-57).
 *
 * What each entry point replaces in the reference (paths relative to the reference root):
 *
 *  akr_hip_upload_mesh       MeshInstance<C> views built by AkariMesh::compile
 *                            (src/akari/core/nodes/mesh.cpp:47-61; layout kernel/instance.h:30-35)
 *  akr_hip_upload_textures   ConstantTexture / ImageTexture  (src/akari/kernel/texture.h:30-66)
 *  akr_hip_upload_materials  Material<C> closed Variant     (src/akari/kernel/material.h:205-298)
 *  akr_hip_upload_lights     AreaLight list + Distribution1D built in SceneNode::compile
 *                            (src/akari/core/nodes/scene.cpp:51-92; common/distribution.h:46-102)
 *  akr_hip_build_accel       BVHAccelerator<C>::build / Scene<C>::commit
 *                            (src/akari/kernel/bvh-accelerator.h:673-678; kernel/scene.cpp:64-81)
 *  akr_hip_trace (any_hit=0) BVHAccelerator<C>::intersect  (bvh-accelerator.h:679-681, 488-518)
 *  akr_hip_trace (any_hit=1) BVHAccelerator<C>::occlude    (bvh-accelerator.h:682, 519-547)
 *  akr_hip_set_camera        PerspectiveCameraNode::compile + PerspectiveCamera::preprocess
 *                            (src/akari/core/nodes/camera.cpp:26-52; kernel/camera.h:45-59)
 *  akr_hip_render            gpu::PathTracer<C>::render / cpu::PathTracer<C>::render
 *                            (kernel/integrators/gpu/cuda/integrator.cpp:137-424,
 *                             kernel/integrators/cpu/integrator.cpp:89-142), called from
 *                             SceneNode::render (src/akari/core/nodes/scene.cpp:137-150)
 *  akr_hip_kernel_stats      print_kernel_stats (src/akari/kernel/cuda/launch.cpp:92-118)
 *
 * Semantics are those of the reference CPU path (no radiance clamp unless ray_clamp > 0,
 * max_depth from the parameters, NEE only, LCG sampler seeded x + y*W per pixel).
 *
 * Threading and ordering: a context is bound to one device.  Its traces and renders share the
 * context's work counters, traversal overflow stacks and queues, so every trace / render call on a
 * context is ordered after the previous one on the device (an event the next call's stream waits
 * on), whatever streams the caller passes; calls from several host threads on one context must
 * still be serialised by the caller.  Different contexts are independent.
 */
#ifndef AKR_HIP_H
#define AKR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: akr_trace_counts gained deep_rays[3]; akr_pixel_probe / akr_hip_pixel_probe added
 * 3: akr_trace_counts gained leaf_tests[3]
 *    (still 3 with the render session, adaptive sampling, feature and filter calls below: they only
 *    add exports and change no struct layout) */
#define AKR_HIP_API_VERSION 3

typedef struct akr_hip_ctx akr_hip_ctx;

/* Ray<C> (common/math.h:183-199): origin, tmin, direction, tmax.  32 bytes. */
typedef struct akr_ray {
    float o[3];
    float tmin;
    float d[3];
    float tmax;
} akr_ray;

/* Intersection<C> (kernel/scene.h:40-49).  Miss: t = +inf, geom_id = prim_id = -1. 32 bytes. */
typedef struct akr_hit {
    float t;
    float u, v;        /* barycentrics (b1, b2) of the Moller-Trumbore test, instance.h:57-68 */
    int32_t geom_id;   /* index of the mesh in upload order */
    int32_t prim_id;   /* triangle index inside that mesh */
    int32_t _pad[3];
} akr_hit;

enum { AKR_TEX_CONSTANT = 0, AKR_TEX_IMAGE = 1 };
typedef struct akr_texture {
    int32_t type;      /* AKR_TEX_CONSTANT: value[] used; AKR_TEX_IMAGE: image index */
    float value[3];
    int32_t image;
    int32_t _pad[3];
} akr_texture;

/* Mirror and Glass are perfectly specular: a scene that holds one renders in the
 * wavefront form.  A light triangle must still be Emissive. */
enum { AKR_MAT_DIFFUSE = 0, AKR_MAT_GLOSSY = 1, AKR_MAT_EMISSIVE = 2, AKR_MAT_MIX = 3, AKR_MAT_MIRROR = 4,
       AKR_MAT_GLASS = 5 };
typedef struct akr_material {
    int32_t type;
    int32_t color;      /* texture index: Diffuse/Glossy/Emissive colour, Mirror reflectance, Glass tint */
    int32_t roughness;  /* texture index: Glossy roughness (x channel, squared -> alpha); Glass reuses it for
                           the index of refraction (x channel of a constant texture, finite, in [1, 8]) */
    int32_t fraction;   /* texture index: Mix fraction (x channel) */
    int32_t first;      /* material index: Mix material_A */
    int32_t second;     /* material index: Mix material_B */
    int32_t double_sided; /* Emissive */
    int32_t _pad;
} akr_material;

/* One emissive triangle (AreaLight, kernel/light.h:47-71). */
typedef struct akr_area_light {
    int32_t geom_id;
    int32_t prim_id;
} akr_area_light;

/* PerspectiveCameraNode fields (core/nodes/camera.cpp:26-52). */
typedef struct akr_camera {
    float position[3];
    float rotation_deg[3];
    double fov_deg;
    int32_t resolution[2];
    int32_t _pad[2];
} akr_camera;

/* Path node fields (core/nodes/integrator.cpp:50-84).  ray_clamp <= 0 disables the clamp
 * (reference CPU semantics); > 0 clamps each sample to [0, ray_clamp] (GPU semantics).
 * flags: AKR_PT_EXACT_CULL = traverse with the reference's intersectAABB bit for bit (it keeps
 * boxes that lie behind the ray origin); default is the standard slab test, same hits. */
#define AKR_PT_EXACT_CULL 1
typedef struct akr_pt_params {
    int32_t spp;
    int32_t max_depth;
    float ray_clamp;
    int32_t flags;
} akr_pt_params;

/* Ambient-occlusion integrator parameters (cpu::AmbientOcclusion, kernel/integrators/cpu/
 * integrator.h:35-45; AOIntegratorNode defaults spp 16, occlude +inf, core/nodes/integrator.cpp:26-49). */
typedef struct akr_ao_params {
    int32_t spp;
    float occlude;  /* a closest hit of the AO ray with t < occlude occludes it */
    int32_t flags;  /* AKR_PT_EXACT_CULL */
    int32_t _pad;
} akr_ao_params;

/* Pixel rectangle [x0, x1) x [y0, y1). */
typedef struct akr_rect {
    int32_t x0, y0, x1, y1;
} akr_rect;

typedef struct akr_build_params {
    int32_t max_leaf_size;  /* <= 8 */
    int32_t n_bins;         /* SAH bins per axis (reference: 32, bvh-accelerator.h:104) */
    float traversal_cost;   /* SAH cost of a traversal step (default 1) */
    float intersect_cost;   /* SAH cost of a triangle test (default 4: measured best for the wide
                             * traversal, where a leaf visit also pays its exact-box test) */
    int32_t n_threads;      /* 0 = hardware concurrency */
    int32_t builder;        /* AKR_BUILDER_SAH (host binned SAH, default), _LBVH (GPU) or _SBVH (host) */
    float spatial_budget;   /* SBVH: extra references allowed, as a fraction of the triangles
                             * (0 = default 0.5) */
    int32_t wide_collapse;  /* the traversal's 4-wide view: AKR_COLLAPSE_SAH (0,
                             * default) or AKR_COLLAPSE_BALANCED */
} akr_build_params;
#define AKR_COLLAPSE_SAH 0       /* treelets of up to 3 BVH2 nodes chosen for the fewest expected visits */
#define AKR_COLLAPSE_BALANCED 1  /* a wide node folds in only its own internal children */
#define AKR_BUILDER_SAH 0
#define AKR_BUILDER_LBVH 1  /* GPU Morton/Karras build: much faster, lower tree quality */
#define AKR_BUILDER_SBVH 2  /* host SBVH: the reference's spatial splits (bvh-accelerator.h:125-475) */

typedef struct akr_accel_info {
    uint64_t n_nodes;       /* 64-byte BVH2 nodes, node 0 is the virtual root */
    uint64_t n_tris;        /* 48-byte leaf-ordered triangle records */
    int32_t max_depth;
    int32_t max_leaf;
    double build_ms;
    double sah_cost;
} akr_accel_info;

typedef struct akr_kernel_stat {
    char name[48];
    uint64_t launches;
    double total_ms;
    double min_ms;
    double max_ms;
} akr_kernel_stat;

/* Traversal counters (filled when option "count_tests" is 1). */
typedef struct akr_trace_counts {
    uint64_t rays;
    uint64_t box_tests;
    uint64_t tri_tests;
    uint64_t closest_rays;
    uint64_t shadow_rays;
    uint64_t per_mode[3][3]; /* [closest, any-hit, shadow] x [rays, box_tests, tri_tests] */
    /* SIMD lane slots per mode: [traversal-loop lane-iterations (64 per wave-iteration), of which
     * lanes holding a ray, triangle-loop lane-iterations, node visits]; visits / slots[0] and
     * tri_tests / slots[2] are lane utilisations. */
    uint64_t lane_slots[3][4];
    /* rays per mode whose traversal stack grew past the LDS-resident entries into the global
     * overflow area (the deep-stack path, kernels.hip stack_pop / wide_order_push) */
    uint64_t deep_rays[3];
    /* leaf records fetched per mode (each an exact leaf-box test; with the node visits, the
     * dependent fetch rounds of a traversal) */
    uint64_t leaf_tests[3];
} akr_trace_counts;

/* Test-only per-pixel fingerprint of the last render's sample loop (option "pixel_probe" = 1),
 * one record per film slot in packed tile order (as akr_hip_render_device): the LCG state after the
 * pixel's last sample (its draw count encodes every path length, kernel/sampler.h:54-67), and the
 * closest-hit and shadow traces of all its samples (pathtracer.h:69-91, 133-164).  The seed is
 * recorded by every render form; the ray counts by the wavefront form and by the counting build of
 * the persistent kernels (option "count_tests"), flagged in `flags`. */
#define AKR_PROBE_SEED 1u
#define AKR_PROBE_RAYS 2u
typedef struct akr_pixel_probe {
    uint32_t seed;
    uint32_t closest_rays;   /* camera + extension rays traced (none at depth == max_depth) */
    uint32_t shadow_rays;    /* NEE shadow rays traced */
    uint32_t flags;          /* AKR_PROBE_SEED | AKR_PROBE_RAYS: which fields were recorded */
} akr_pixel_probe;

int akr_hip_api_version(void);
int akr_hip_device_count(int *n);

int akr_hip_create(int device, akr_hip_ctx **out);
int akr_hip_destroy(akr_hip_ctx *ctx);
const char *akr_hip_last_error(const akr_hip_ctx *ctx);
/* Options: "stats" (per-kernel HIP-event timing: 0 off, 1 every kernel, 2 trace_closest only), "count_tests" (traversal counters),
 * "count_lines" (with count_tests: k_path marks the 128-B lines it reads, see akr_hip_path_profile),
 * "exact_cull", "wide", "lean", "shadow_grid_pct", "rays_per_lane" (tuning / A-B).
 * Render forms and their tuning (all give the same bits): "path" (0 wavefront,
 * 1 persistent kernel, 2 auto), "path_auto_pixels", "path_auto_complex";
 * the persistent form: "path_spec" (k_path_spec: 1 always, 0 never, 2 auto), "path_defer" (k_path_defer:
 * 1 forced, 0 k_path forced, 2 auto), the auto rule's "path_tail_ppl10" and "path_tail_steps" and its
 * overrides "path_spec_pixels", "path_defer_pixels", "path_defer_min_tris"; k_path_spec's "path_spec_depth",
 * "path_spec_fetch", "path_spec_fetch_pixels";
 * "path_tab", "path_mix", "path_min_wait", "path_grid_pct", "path_prio";
 * k_path's pop site: "path_pop_rounds" (1..255) and "path_pop_keep" (1..64): pop rounds run while at least
 * path_pop_keep lanes are unserved, at most path_pop_rounds per iteration (255 / 1: until the slowest lane);
 * the cost order: "path_order", "path_order_min_spp", "path_order_share_pixels", "path_order_share_min_spp",
 * "path_order_shift", "path_order_pair", "path_order_classes", "path_order_cap", "path_order_sub",
 * "path_order_pilot_spp", "wave_order" (the wavefront's camera rays in cost order).
 * "verify" (default 1): in-band film check after every render.  Test only: "pixel_probe" (record
 * akr_pixel_probe per slot), "fault_test" (raise the hang guard's fault word once), "ray_steps",
 * "serial_shadow", "any_far_first". */
int akr_hip_set_option(akr_hip_ctx *ctx, const char *key, int64_t value);
/* One more key is a session switch rather than a knob of the render: "film_variance" (0 or 1, default 0; read when a
 * session starts) makes the session track the variance of every slot's mean from its passes, see
 * akr_hip_render_variance below.
 * And another: "mis" (0 or 1, default 0; read when a session starts, a continue keeps the session's value; any
 * other value is refused) makes direct lighting the power-heuristic combination of the next-event sample and the
 * BSDF sample the extension ray already is.  No draw and no ray is added: every slot's sampler
 * state and ray counts are those of a render without it.  The render takes the wavefront form whatever "path"
 * says, and akr_hip_render_form reports it.  The AO integrator ignores it.
 * And a choice of form: "env_path" (0 or 1, default 0; read at every render and continue, like "path"; any other
 * value is refused).  An environment light keeps the wavefront form unless it is 1; with it on, "path" decides as
 * it does without an environment, and where it takes a persistent kernel, k_path's environment build renders the
 * scene ("path_defer" and "path_spec" are not consulted unless "env_forms" is 1, below).  The
 * result is the wavefront's bit for bit; akr_hip_render_form reports k_path.  "mis", exact_cull, "wide" 0 and a view
 * outside the lean test's bounds keep the wavefront as before.  Without an environment it changes nothing.
 * And which persistent forms it may take: "env_forms" (0 or 1, default 0; read at every render and continue; any
 * other value is refused).  It acts only when an environment is set and "env_path" is 1: the render form rule then
 * decides exactly as it does without an environment ("path_defer", "path_spec", the cache and tail rules, the gated
 * launch of two candidates, subset lists), and k_path, k_path_defer and k_path_spec each have an environment build
 * that carries the choice out.  The result is the same bit for bit; akr_hip_render_form reports
 * the form that ran and akr_hip_render_shading its shading build.  With it 0, or "env_path" 0, or no environment,
 * every launch is the one it was. */

int akr_hip_upload_mesh(akr_hip_ctx *ctx, const float *vertices, uint64_t n_vertices,
                        const int32_t *indices, const float *normals, const float *texcoords,
                        const int32_t *material_indices, uint64_t n_triangles,
                        const int32_t *material_slots, int32_t n_slots, int32_t *geom_id);
/* akr_hip_upload_mesh appends: geom_id counts the meshes the context holds.  This forgets them all (and the
 * acceleration structure built over them), so that the context can take another scene's meshes from
 * geom_id 0; textures, materials, lights, environment and camera stay as they were uploaded. */
int akr_hip_clear_meshes(akr_hip_ctx *ctx);
int akr_hip_upload_images(akr_hip_ctx *ctx, const float *rgba, const int32_t *widths,
                          const int32_t *heights, int32_t n_images);
int akr_hip_upload_textures(akr_hip_ctx *ctx, const akr_texture *textures, int32_t n);
int akr_hip_upload_materials(akr_hip_ctx *ctx, const akr_material *materials, int32_t n);
int akr_hip_upload_lights(akr_hip_ctx *ctx, const akr_area_light *lights, int32_t n,
                          const float *power);

/* Environment light: an N x N octahedral map of the sphere over the square
 * [-1, 1]^2, RGB f32, row-major, nearest-texel lookup, importance-sampled in direct lighting and seen by
 * camera rays that leave the scene.  rgb: resolution * resolution * 3 floats, finite and >= 0, not black
 * everywhere; null removes the environment.  scale multiplies every texel; world_to_env is the row-major
 * 3x3 R of d_env = R d_world; select_prob, inside (0, 1), is the share of the direct-lighting draws the
 * environment takes in a scene that also has area lights.  The distribution's tables are built on the host
 * here.  Ends the render session, as every upload does.  A context with an environment renders in the
 * wavefront form whatever option "path" says (akr_hip_render_form reports it). */
typedef struct akr_environment {
    int32_t resolution;
    int32_t _pad;
    float scale[3];
    float select_prob;
    float world_to_env[9];
} akr_environment;
int akr_hip_upload_environment(akr_hip_ctx *ctx, const akr_environment *env, const float *rgb);
/* What the map does, through the device functions the shading calls; host buffers, synchronous.
 * sample: u[2n] in [0, 1]^2 -> world directions dir[3n], the sampled texels with the scale applied rgb[3n]
 * and the solid-angle pdfs pdf[n].  eval: world directions dir[3n] -> the texel each one looks up and the
 * pdf with which sampling draws it. */
int akr_hip_environment_sample(akr_hip_ctx *ctx, const float *u, uint64_t n, float *dir, float *rgb, float *pdf);
int akr_hip_environment_eval(akr_hip_ctx *ctx, const float *dir, uint64_t n, float *rgb, float *pdf);

int akr_hip_build_accel(akr_hip_ctx *ctx, const akr_build_params *params);
/* Adopt a BVH2 built elsewhere (the arrays akr_hip_accel_export writes: akr_bvh_node[n_nodes],
 * akr_bvh_tri[n_tris]) for the uploaded meshes, instead of building one: the same wide view and
 * device copy follow.  The tree is validated first (akr_bvh_validate); results are those of the
 * context that built it, bit for bit.  Lets the ranks of a node build the scene's BVH once. */
int akr_hip_import_accel(akr_hip_ctx *ctx, const void *nodes, uint64_t n_nodes, const void *tris,
                         uint64_t n_tris, int32_t n_threads);
int akr_hip_accel_info(akr_hip_ctx *ctx, akr_accel_info *info);
int akr_hip_accel_export(akr_hip_ctx *ctx, void *nodes, uint64_t node_bytes, void *tris,
                         uint64_t tri_bytes);
int akr_hip_set_camera(akr_hip_ctx *ctx, const akr_camera *camera);
/* The thin lens of the reference's kernel camera (kernel/camera.h:43-44, 75-80): lens_radius and
 * focal_distance, which its camera node never sets.  Both must be finite and >= 0; any other value fails,
 * names the value and leaves the context as it was.  (0, 0) is the pinhole and the state of a new context.
 * The lens is active when both are > 0 (camera.h:75): a camera ray then leaves the point
 * concentric_disk(u1) * lens_radius of the lens towards the point where the pinhole ray meets the plane
 * z = -focal_distance of camera space.  u1 is the draw every sample already makes ahead of the film draw,
 * so no sampler state changes.  With an active lens akr_hip_render runs the wavefront form whatever the
 * options "path", "env_path", "env_forms" and "path_auto_complex" say (akr_hip_render_form reports it), and
 * akr_hip_render_ao and the feature pass use the same rays; the cost-order pilot keeps pinhole rays.
 * akr_hip_set_lens ends the render session, as akr_hip_set_camera does; akr_hip_set_camera leaves the lens
 * alone.  akr_camera and AKR_HIP_API_VERSION are unchanged. */
int akr_hip_set_lens(akr_hip_ctx *ctx, float lens_radius, float focal_distance);
/* Reads the lens back (any pointer may be null); *active is 1 under the reference's condition above. */
int akr_hip_lens(akr_hip_ctx *ctx, float *lens_radius, float *focal_distance, int32_t *active);

/* Batched trace, host buffers in and out, synchronous. */
int akr_hip_trace(akr_hip_ctx *ctx, const akr_ray *rays, uint64_t n, akr_hit *hits, int any_hit);
/* Batched trace on device buffers (akr_ray[n] -> akr_hit[n]) on `stream` (hipStream_t, may be 0). */
int akr_hip_trace_device(akr_hip_ctx *ctx, const void *d_rays, uint64_t n, void *d_hits,
                         int any_hit, void *stream);

/* Render the pixels of `tiles` (clipped to the camera resolution) and ACCUMULATE into host
 * full-frame buffers radiance[W*H*3] (sum of L) and weight[W*H] (sample count), the reference
 * Film's Pixel{radiance, weight} (core/film.h:31-35).  Synchronous. */
int akr_hip_render(akr_hip_ctx *ctx, const akr_pt_params *params, const akr_rect *tiles,
                   int32_t n_tiles, float *radiance, float *weight);
/* cpu::AmbientOcclusion::render (kernel/integrators/cpu/integrator.cpp:40-87) — replaces
 * AOIntegrator::render (core/nodes/integrator.cpp:33-38) for the pixels of `tiles`: per sample,
 * L = 1 if the camera ray hits and the cosine-sampled ray about the geometric normal from the hit
 * point has no closest hit with t < occlude, else 0; accumulated like akr_hip_render.  Reuses the
 * path tracer's raygen / closest-hit trace; with occlude = +inf the AO ray is an occlusion query
 * (shadow-mode trace), otherwise a closest-hit trace whose t is compared.  Synchronous. */
int akr_hip_render_ao(akr_hip_ctx *ctx, const akr_ao_params *params, const akr_rect *tiles,
                      int32_t n_tiles, float *radiance, float *weight);
/* Multi-GPU render from one host process (SURVEY.md §8b akr_hip_render_node): tile j goes to
 * ctxs[j % n_ctx] (one context per device, each holding the same scene and camera), the contexts
 * render concurrently on one host thread each, and their films are gathered on ctxs[0]'s device
 * (device-to-device / xGMI peer copies) and merged there into the frame in context order, which is
 * added to the host buffers — the same pixels as akr_hip_render on one context, bit for bit.
 * (Multi-process runs over RCCL use akr_hip_render_device + akari_amd/dist.py instead.)
 * On failure the message is on ctxs[0]. */
int akr_hip_render_node(akr_hip_ctx *const *ctxs, int32_t n_ctx, const akr_pt_params *params,
                        const akr_rect *tiles, int32_t n_tiles, float *radiance, float *weight);
/* Same, but writes (overwrites) device buffers in packed tile order: pixel k of the tile list
 * (tiles in order, row-major inside a tile) -> radiance[3k..3k+2], weight[k].  Returns the
 * pixel count in *n_pixels.  The work is enqueued on `stream`; with option "verify" on (the
 * default) the call then WAITS on the host for the render and its in-band check (every slot holds
 * spp samples, and no persistent wave stopped on its hang guard) before it returns, so the check
 * can fail this call.  With "verify" 0 the call returns once the work is enqueued (fully
 * asynchronous); a hang-guard fault is then reported by the context's next render or
 * akr_hip_synchronize. */
int akr_hip_render_device(akr_hip_ctx *ctx, const akr_pt_params *params, const akr_rect *tiles,
                          int32_t n_tiles, float *d_radiance, float *d_weight, void *stream,
                          uint64_t *n_pixels);

/* ---- Render sessions: continue a finished path render.
 *
 * A context remembers its last path render as a session: the tile list and its packed film slots,
 * max_depth, ray_clamp, flags, the camera resolution, and per slot the samples done, the film sums
 * and the LCG sampler state after the last sample.  A continue renders `spp` more samples per slot
 * from exactly there, so a render of a spp continued by b spp equals one render of a + b spp bit for
 * bit, in radiance, weight and sampler state, whichever form ran each segment.
 *
 *  - akr_hip_render and akr_hip_render_device start a new session (replacing any earlier one), and so
 *    does akr_hip_render_state_import.  A continue extends the session.
 *  - akr_hip_upload_mesh / _images / _textures / _materials / _lights, akr_hip_clear_meshes, akr_hip_build_accel,
 *    akr_hip_import_accel, akr_hip_set_camera, akr_hip_render_ao, and akr_hip_render_node on a member
 *    context end it.  A continue without a session returns a non-zero status whose message begins
 *    "no render session to continue"; the context stays usable.  A continue that fails while
 *    rendering ends the session (its film may be partly extended).
 *  - akr_hip_trace, akr_hip_trace_device and the query calls keep it.
 *  - akr_hip_render_features, akr_hip_render_features_device, akr_hip_denoise and akr_hip_denoise_device keep
 *    it: they touch neither the film, the sampler states, the per-slot counts nor the session record.
 *    So do akr_hip_render_variance, akr_hip_render_variance_device, akr_hip_denoise_guided and its device form.
 *  - With option "film_variance" set when the session starts, the session also tracks the variance of every
 *    slot's mean from its passes: a fresh render starts the tracker from nothing, an import takes the imported
 *    film as one batch, every continue adds a batch, and whatever ends the session ends the tracker (the rules
 *    are with akr_hip_render_variance below).  The film, the sampler states and the probe do not depend on it.
 *  - akr_hip_set_option between segments is allowed, and may switch the render form, the cost order
 *    and exact_cull: all give the same bits.
 *  - spp = 0 renders nothing and returns the totals.  A total above 2^24 samples per slot is refused
 *    (the weight is an f32 count); the session stays.
 *  - The film checks (option "verify") compare every slot's weight with the session's total.
 *  - With option "pixel_probe" the probe of a continue holds each slot's sampler state after the
 *    total, and the ray counts of that segment alone. */
typedef struct akr_render_state_info {
    uint64_t n_pixels;            /* film slots, packed tile order */
    int32_t spp_done, max_depth;
    float ray_clamp;
    int32_t flags;
    int32_t width, height, n_tiles, _pad;  /* n_tiles: the clipped, non-empty tiles */
} akr_render_state_info;

/* spp more samples per slot of the context's session.  Host form: ADDS the session's totals to
 * full-frame buffers exactly as akr_hip_render of spp_done + spp samples would have (pass zeroed
 * buffers to get the film).  Synchronous. */
int akr_hip_render_continue(akr_hip_ctx *ctx, int32_t spp, float *radiance, float *weight);
/* Device form: overwrites packed buffers with the session's totals like akr_hip_render_device, with
 * the same "verify" behaviour. */
int akr_hip_render_continue_device(akr_hip_ctx *ctx, int32_t spp, float *d_radiance, float *d_weight,
                                   void *stream, uint64_t *n_pixels);
int akr_hip_render_state_info(akr_hip_ctx *ctx, akr_render_state_info *info);
/* The session's state to host memory, n = its n_pixels: sampler[n] (LCG state after each slot's
 * last sample; x + y * width where no sample was drawn), film[n][4] (sum r, g, b, weight). */
int akr_hip_render_state_export(akr_hip_ctx *ctx, uint32_t *sampler, float *film, uint64_t n);
/* Establish a session as if params->spp samples had just been rendered over `tiles` (the context
 * holds the scene, tree and camera): n must equal the clipped tile list's pixel count and every
 * film[k][3] must equal params->spp, else the call is refused and changes nothing.  Seeds
 * x + y * width, a zero film and spp 0, continued, reproduce a fresh render. */
int akr_hip_render_state_import(akr_hip_ctx *ctx, const akr_pt_params *params, const akr_rect *tiles,
                                int32_t n_tiles, const uint32_t *sampler, const float *film, uint64_t n);

/* ---- Sessions whose slots hold different sample counts, and adaptive sampling.
 *
 * A masked continue renders `spp` more samples for the slots whose byte in mask[n] (packed tile
 * order, n = the session's n_pixels) is non-zero and nothing for the others.  A slot's samples are one
 * LCG chain, so a slot that has received c samples equals the c-spp render at that pixel bit for bit,
 * whatever its neighbours received.  The mask is compacted on the device into the ascending list of
 * active slots, and the pass is the usual launch over that shorter list, unranked (the cost order of
 * §3.10 is not computed for a subset; all orders give the same bits).  The auto form rule sees the
 * number of active slots as its pixel count.
 *
 *  - n != n_pixels is refused and the session stays.  No session: "no render session to continue".
 *  - An all-zero mask, or spp = 0, renders nothing and returns the totals.
 *  - The 2^24 cap applies to the largest resulting count; a refused call changes nothing.
 *  - A later akr_hip_render_continue adds spp to every slot, from each slot's own count.
 *  - akr_render_state_info.spp_done reports the largest count, akr_hip_render_state_spp_range both ends.
 *  - akr_hip_render_state_export is unchanged: its film weights are the counts.  akr_hip_render_state_import
 *    refuses such a film (its weights differ from spp): a non-uniform session cannot be checkpointed.
 *  - Option "verify" compares every slot's weight with that slot's expected count.
 *  - Option "pixel_probe": each slot's sampler state after its own total (for slots the mask leaves out,
 *    the state they already had), and the ray counts of that pass alone. */
int akr_hip_render_continue_masked(akr_hip_ctx *ctx, int32_t spp, const uint8_t *mask, uint64_t n,
                                   float *radiance, float *weight);
int akr_hip_render_continue_masked_device(akr_hip_ctx *ctx, int32_t spp, const uint8_t *d_mask, uint64_t n,
                                          float *d_radiance, float *d_weight, void *stream,
                                          uint64_t *n_pixels);
/* The smallest and the largest sample count of the session's slots (equal for a uniform session). */
int akr_hip_render_state_spp_range(akr_hip_ctx *ctx, int32_t *spp_min, int32_t *spp_max);

/* Adaptive render: sample until the film has converged, strip by strip.  A strip is 64 consecutive
 * slots in packed tile order (the last may be short).  Every slot gets min_spp samples; then passes
 * run over the strips still active (pass_spp more samples each, or with pass_spp 0 as many as the
 * strip holds, doubling its count), clipped so that no count passes the cap params->spp.  After each
 * pass the convergence test compares the film I with the snapshot P taken before that pass; per slot,
 * with counts c1 > c0 > 0, in f32, left to right, unfused, correctly rounded / and sqrt:
 *     m1 = I / c1, m0 = P / c0 (per channel)
 *     d = |m1r - m0r| + |m1g - m0g| + |m1b - m0b|,  s = m1r + m1g + m1b,  e = s > 0 ? d / sqrt(s) : 0
 * The strip error E is the sum of its slots' e as a fixed binary tree (adjacent pairs, six levels;
 * absent slots of a short strip count 0) divided by the strip's slot count.  A strip stops when
 * E <= threshold (a NaN keeps sampling) and never restarts; a strip that goes on takes the film as its
 * new snapshot.  The loop ends when no strip is active or the active strips hold the cap.  All active
 * strips hold the same count at every moment.  params->spp <= min_spp is a plain render of params->spp
 * with no test.  The film does not depend on the render form, the cost order or exact_cull.  The
 * session stays and can be continued, masked or uniformly.  The host reads four bytes per pass (the
 * number of active slots); the film stays on the device between passes. */
typedef struct akr_adaptive_params {
    int32_t min_spp;    /* every slot gets these before the first test, >= 1 */
    int32_t pass_spp;   /* samples per later pass; 0: each pass doubles the active slots' count */
    float threshold;    /* >= 0, not NaN */
    int32_t _pad;
} akr_adaptive_params;
typedef struct akr_adaptive_info {
    int32_t passes;           /* the min_spp pass and every later pass */
    int32_t spp_min, spp_max, _pad;
    uint64_t samples;         /* sum of all slots' counts */
    uint64_t strips, strips_at_cap;   /* strips still above the threshold when they reached params->spp */
} akr_adaptive_info;
/* Host form: ADDS the film to full-frame buffers like akr_hip_render.  `info` may be null. */
int akr_hip_render_adaptive(akr_hip_ctx *ctx, const akr_pt_params *params, const akr_adaptive_params *ap,
                            const akr_rect *tiles, int32_t n_tiles, float *radiance, float *weight,
                            akr_adaptive_info *info);
/* Device form: overwrites packed buffers like akr_hip_render_device.  The passes are enqueued on
 * `stream`, and the call waits on the host for each pass's active count. */
int akr_hip_render_adaptive_device(akr_hip_ctx *ctx, const akr_pt_params *params, const akr_adaptive_params *ap,
                                   const akr_rect *tiles, int32_t n_tiles, float *d_radiance, float *d_weight,
                                   void *stream, uint64_t *n_pixels, akr_adaptive_info *info);
/* The same render one pass at a time, for callers that want the film between passes (previews, a time
 * budget).  akr_hip_adaptive_begin renders min_spp for every slot (starting the session) and takes the
 * snapshot; each akr_hip_adaptive_step runs one pass over the active strips and its test.  *more is 1
 * while a pass remains.  begin followed by steps until *more is 0 is akr_hip_render_adaptive, bit for
 * bit and in `info`; stopping earlier leaves the film and session of the passes done.  Between steps
 * akr_hip_render_continue with spp 0 returns the film so far; a continue that draws samples ends the
 * adaptive run (a later step is refused) but keeps the session. */
int akr_hip_adaptive_begin(akr_hip_ctx *ctx, const akr_pt_params *params, const akr_adaptive_params *ap,
                           const akr_rect *tiles, int32_t n_tiles, akr_adaptive_info *info, int32_t *more);
int akr_hip_adaptive_step(akr_hip_ctx *ctx, akr_adaptive_info *info, int32_t *more);
/* The last convergence test's values of the session's adaptive render, n_strips = ceil(n_pixels / 64):
 * each strip's error E and whether it is still active.  A strip that stopped earlier keeps the error
 * it stopped with.  Fails when the session ran no test. */
int akr_hip_adaptive_error(akr_hip_ctx *ctx, float *strip_error, uint8_t *strip_active, uint64_t n_strips);

/* ---- Feature buffers and the edge-avoiding a-trous filter of the film.
 *
 * Feature pass.  Every film slot of the tile list (clipped, packed tile order, exactly as in
 * akr_hip_render_device) gets `spp` camera rays from the slot's own LCG chain seeded x + y * width.  A ray takes
 * four draws (the camera ray's) and nothing else advances the chain: sample k uses draws 4k..4k+3.  Sample 0 is
 * therefore the beauty render's first camera ray; LATER SAMPLES ARE NOT the render's later camera rays, because
 * the render's chain also holds the draws of each path.  Each ray is traced closest-hit with the context's
 * ordinary trace.  A hit adds to the slot's record of 12 floats
 *     (ar, ag, ab, hits,  nx, ny, nz, t,  px, py, pz, 0)
 * 1 to hits, the hit distance to t, the point p = lerp3(v0, v1, v2, u, v), the geometric normal
 * normalize(cross(v1 - v0, v2 - v0)) negated when its dot with the ray direction is > 0 (turned towards the
 * viewer: windings are arbitrary), and the albedo: the colour (at the interpolated texcoord) of the material
 * the path tracer would shade, found by walking Mix as Material::select_material does with the next draw of a
 * COPY of the chain after the camera ray as the selector (so the mean over samples is the blend).  Diffuse,
 * Glossy and Emissive give their colour (Emissive whichever way it faces, so that the filter's albedo stop keeps
 * a lamp from bleeding into a coplanar ceiling); a null material is a hit with albedo 0.  A miss adds nothing.
 * All f32, sums in sample order.  spp >= 1; flags: AKR_PT_EXACT_CULL or 0.
 * The pass keeps the render session (it has its own accumulators and chain states). */
typedef struct akr_feature_params {
    int32_t spp;
    int32_t flags;
} akr_feature_params;
/* Host form: ADDS the records into a full-frame features[W*H*12], as akr_hip_render adds its film.  Synchronous. */
int akr_hip_render_features(akr_hip_ctx *ctx, const akr_feature_params *params, const akr_rect *tiles,
                            int32_t n_tiles, float *features);
/* Device form: overwrites a packed d_features[n*12] (slot order) on `stream`; returns n in *n_pixels. */
int akr_hip_render_features_device(akr_hip_ctx *ctx, const akr_feature_params *params, const akr_rect *tiles,
                                   int32_t n_tiles, float *d_features, void *stream, uint64_t *n_pixels);

/* Filter.  Inputs, frame ordered: radiance[W*H*3] and weight[W*H] (the film as akr_hip_render returns it: weight 0
 * outside the tiles, differing weights in an adaptive film) and features[W*H*12] (sums, as above).  Output
 * out_rgb[W*H*3]: the filtered MEAN colour.  Needs no scene; keeps the session.  Refused with a message: a null
 * pointer, W * H == 0, parameters out of range.
 *
 * Definition (only + - * /, sqrt, fabs, comparisons and rmax / dot / sub / length of akr_math.h; f32, unfused,
 * left to right).  Per pixel p:
 *     valid = weight > 0;  c = valid ? radiance / weight : 0
 *     h = hits;  a, n, t, x = h > 0 ? the record's sums / h : 0;  l = length(n);  nh = l > 0 ? n / l : 0
 *     per channel m = (demodulate && a.ch > 1e-3f) ? a.ch : 1;  I0 = c / m
 * Iteration i = 0 .. iterations - 1: step s = 1 << i, sc = sigma_color * (1.0f / (1 << i)),
 * hk = {1/16, 1/4, 3/8, 1/4, 1/16}; num = den = 0; for j = 0..4 (outer), k = 0..4 (inner) the tap is
 * q = (x + (k - 2) s, y + (j - 2) s).  A tap is SKIPPED (a select, not a multiply by 0) when q is outside the
 * frame, q is invalid (its weight is not > 0), or any channel of I_q is not finite.  Tap weight
 *     w = ((hk[j] * hk[k]) * g) * wc
 * with g = wc = 1 at the centre tap, and elsewhere
 *     g  = wn * wz * wa when both p and q have hits, 1 when neither has, 0 otherwise
 *     wn = rmax(dot(nh_p, nh_q), 0), squared normal_squarings times
 *     wz = rmax(1 - fabsf(dot(nh_p, sub(x_q, x_p))) / (sigma_depth * t_p), 0)
 *     wa = rmax(1 - (|da.r| + |da.g| + |da.b|) / sigma_albedo, 0),  da = a_q - a_p
 *     wc = sigma_color > 0 ? 1 / (1 + dot(d, d) / (sc * sc)) : 1,  d = I_q - I_p
 * An accepted tap does num += w * I_q per channel and den += w.  The iteration's result: 0 for an invalid p,
 * I_p unchanged when it is not finite, else den > 0 ? num / den : I_p.
 * Output: out = I_last * m; invalid pixels give 0. */
#define AKR_DENOISE_NO_DEMODULATE 1  /* m = 1: films that are not albedo times lighting (ambient occlusion) */
typedef struct akr_denoise_params {
    int32_t iterations;        /* 1..8 */
    int32_t normal_squarings;  /* 0..8 */
    float sigma_depth;         /* > 0 */
    float sigma_albedo;        /* > 0 */
    float sigma_color;         /* <= 0 disables the colour stop */
    int32_t flags;             /* AKR_DENOISE_NO_DEMODULATE or 0 */
    int32_t _pad[2];
} akr_denoise_params;
/* Host form: host pointers.  Synchronous. */
int akr_hip_denoise(akr_hip_ctx *ctx, const akr_denoise_params *params, int32_t width, int32_t height,
                    const float *radiance, const float *weight, const float *features, float *out_rgb);
/* Device form: device pointers; the work is enqueued on `stream`. */
int akr_hip_denoise_device(akr_hip_ctx *ctx, const akr_denoise_params *params, int32_t width, int32_t height,
                           const float *d_radiance, const float *d_weight, const float *d_features,
                           float *d_out_rgb, void *stream);

/* ---- Film variance from the session's passes, and the variance-guided filter.
 *
 * Tracker.  Option "film_variance" (0 / 1, default 0) is read when a session starts.  With it on, the session
 * carries per slot a snapshot P of the film at the slot's last update and (M2r, M2g, M2b, K), K the number of
 * batches as an f32 count.  After every call that draws samples (the fresh render, akr_hip_render_continue,
 * akr_hip_render_continue_masked, every pass of akr_hip_render_adaptive, akr_hip_adaptive_begin / _step, and the
 * device forms of these) each slot is updated from the film F = (R, G, B, W); f32, unfused, left to right,
 * correctly rounded /:
 *     n = F.w - P.w;  if !(n > 0) the slot stays as it is
 *     if P.w > 0:  per channel  d = (F.ch - P.ch) / n - P.ch / P.w
 *                               M2.ch = M2.ch + (d * d) * ((P.w * n) / F.w)
 *     K = K + 1;  P = F
 * (West's weighted incremental update on the batch means: a slot's first batch leaves M2 at 0 and K at 1, and
 * M2 / (K - 1) estimates the per-sample variance without bias whatever the batch sizes.)  A call that draws no
 * sample updates nothing; with the option off nothing is allocated or launched.
 *  - A fresh render starts from P = 0, M2 = 0, K = 0.
 *  - akr_hip_render_state_import sets P to the imported film and K to 1 where the weight is positive: a
 *    checkpoint is ONE batch, whatever passes rendered it (a checkpoint holds no variance).
 *  - The tracker has its own snapshot; it does not use the adaptive render's.
 *  - akr_hip_render_features, akr_hip_denoise, akr_hip_denoise_guided, traces and queries keep the tracker;
 *    whatever ends the session ends it.
 *  - Masked and adaptive sessions need nothing special: a slot's weight is its count, and a slot a pass leaves
 *    out sees n = 0.
 * Export: per slot (vr, vg, vb, K); for K >= 2  v.ch = (M2.ch / (K - 1)) / F.w, the variance of the slot's MEAN
 * colour, else 0.  The host form ADDS the records into a full-frame variance[W*H*4], as akr_hip_render adds its
 * film (pass a zeroed buffer; K adds up where tiles overlap).  The device form overwrites a packed
 * d_variance[n*4] (slot order) on `stream` and returns n in *n_pixels.  Both keep the session.  Both are refused
 * with a message that says why when the context has no session ("no render session ...") or the session was
 * started without "film_variance" ("film variance: the session was started without option film_variance"). */
int akr_hip_render_variance(akr_hip_ctx *ctx, float *variance);
int akr_hip_render_variance_device(akr_hip_ctx *ctx, float *d_variance, void *stream, uint64_t *n_pixels);

/* Guided filter: akr_hip_denoise with one more frame-ordered input variance[W*H*4] (as above: the variance of the
 * mean colour and K) and sigma_variance (> 0 and finite).  akr_hip_denoise and its struct are unchanged.
 *
 * Definition: that of akr_hip_denoise with these additions (f32, unfused, left to right, the same operations).
 * Per pixel p, with valid and the demodulation divisor m of akr_hip_denoise:
 *     hv = valid && K >= 2 && vr, vg, vb finite;  V0.ch = hv ? v.ch / (m.ch * m.ch) : 0
 * hv never changes.  Each iteration, before the taps, for a pixel with hv:
 *     G = the 3x3 mean of the current V at stride 1: gk = {1/4, 1/2, 1/4}, gn = gd = 0; for j = 0..2 (outer),
 *     k = 0..2 (inner) the tap q = (x + k - 1, y + j - 1) is SKIPPED when it is outside the frame or has no hv
 *     (an invalid pixel has none), else gn.ch += (gk[j] * gk[k]) * V_q.ch, gd += gk[j] * gk[k];
 *     G = gd > 0 ? gn / gd : V_p
 * Colour stop of a non-centre tap when p has hv (whatever sigma_color is):
 *     e.ch = (d.ch * d.ch) / (G.ch + 1e-8f),  r = ((e.r + e.g) + e.b) / ((3.0f * sigma_variance) * sigma_variance)
 *     wc = 1 / (1 + r)
 * The stride does not tighten it: the propagated variance shrinks by itself.  A pixel without hv keeps the wc of
 * akr_hip_denoise, sigma_color included.
 * Propagation: every accepted tap also does vnum.ch += (w * w) * V_q.ch, with V_q = 0 when q has no hv.  The
 * iteration's V: V_p unchanged for an invalid or non-finite p, else den > 0 ? vnum / (den * den) : V_p.
 * Unchanged: the skip rules for out-of-frame, invalid and non-finite taps, the result rules for invalid and
 * non-finite pixels, g, the stencil and the remodulation.  So with no hv pixel anywhere the output equals
 * akr_hip_denoise's bit for bit. */
typedef struct akr_denoise_guided_params {
    akr_denoise_params base;
    float sigma_variance;      /* > 0 and finite; 2 is the library's default */
    int32_t _pad[3];
} akr_denoise_guided_params;
int akr_hip_denoise_guided(akr_hip_ctx *ctx, const akr_denoise_guided_params *params, int32_t width, int32_t height,
                           const float *radiance, const float *weight, const float *features, const float *variance,
                           float *out_rgb);
int akr_hip_denoise_guided_device(akr_hip_ctx *ctx, const akr_denoise_guided_params *params, int32_t width,
                                  int32_t height, const float *d_radiance, const float *d_weight,
                                  const float *d_features, const float *d_variance, float *d_out_rgb, void *stream);

/* Host-only BVH build (no device needed): the same builder akr_hip_build_accel runs, for tools
 * and CPU-side checks.  Arrays are owned by the handle; free with akr_bvh_host_free. */
typedef struct akr_bvh_host akr_bvh_host;
int akr_bvh_host_build(const float *vertices, uint64_t n_vertices, const int32_t *indices,
                       uint64_t n_triangles, const akr_build_params *params, akr_bvh_host **out,
                       akr_accel_info *info);
const void *akr_bvh_host_nodes(const akr_bvh_host *h);
const void *akr_bvh_host_tris(const akr_bvh_host *h);
void akr_bvh_host_free(akr_bvh_host *h);
/* The 4-wide quantized view the traversal kernels walk (akr_bvh4_node / akr_bvh_leaf), built from
 * the handle's BVH2 on first call; pointers stay valid until akr_bvh_host_free. */
int akr_bvh_host_wide(akr_bvh_host *h, uint64_t *n_nodes, uint64_t *n_leaves, uint32_t *root_ref);
/* Host check of a BVH2 before it is adopted (no device): a tree from the virtual root, references and
 * leaf ranges in range, triangle ids < n_scene_tris, depth <= AKR_BVH_MAX_DEPTH.  0 = valid. */
int akr_bvh_validate(const void *nodes, uint64_t n_nodes, const void *tris, uint64_t n_tris,
                     uint64_t n_scene_tris, int32_t *max_depth);
const void *akr_bvh_host_wide_nodes(const akr_bvh_host *h);
const void *akr_bvh_host_wide_leaves(const akr_bvh_host *h);

int akr_hip_kernel_stats(akr_hip_ctx *ctx, akr_kernel_stat *out, int32_t max_n, int32_t *n);
int akr_hip_trace_counts(akr_hip_ctx *ctx, akr_trace_counts *out);

/* Diagnostic (option count_tests): phase profile of the persistent path kernel's last counted
 * launches, summed over waves, wall-clock ticks at 100 MHz: out[0..10] = waves, outer iterations,
 * processing phases, traversal-loop iterations, ticks processing / traversing / in leaves / in
 * total, the longest wave's ticks, lanes processed, ticks of processing spent on finished rays'
 * results (shading), k_path_spec's speculative samples started / dropped, and the time split of the
 * traversal and leaf phases: ticks issuing their loads, waiting for them, working after them, then
 * k_path's processing split: the park, the sample end with splat / pixel fetch / camera ray, and the
 * unpark with the new rays' start, and the shading's wait for the hit's record (out[19..22]),
 * then the leaf phases entered with a leaf held and the lanes holding one, summed (out[23..24]), then
 * the distinct 128-B lines of the wide nodes, the leaf blob and the shading records that the last
 * k_path render with "count_lines" read (out[25..27]), then k_path's pop site and push (out[28..34]):
 * iterations in which a lane popped, the pop rounds the wave ran in them, the rounds and the pops summed
 * over lanes, iterations with a push, those in which some lane had fewer than four free LDS stack rows,
 * and of these the ones whose entries all fitted in LDS ("bounded pop").
 * Not part of the reference interface. */
int akr_hip_path_profile(akr_hip_ctx *ctx, uint64_t *out, int32_t n);
int akr_hip_reset_stats(akr_hip_ctx *ctx);
/* The last akr_hip_render's lanes per pixel (always 1) and sample passes launched (diagnostic). */
int akr_hip_render_info(akr_hip_ctx *ctx, int32_t *lanes, int32_t *passes);
/* Which form ran the last path render (all give the same bits): the wavefront
 * kernels (north_star's layout: raygen -> closest -> shade -> shadow -> splat launches), the
 * persistent path kernel, its deferred-NEE form or its speculative-sample
 * form; *ordered = 1 when
 * the persistent kernel fetched pixels in pilot-cost order.  AKR_FORM_NONE: nothing rendered. */
#define AKR_FORM_NONE (-1)
#define AKR_FORM_WAVEFRONT 0
#define AKR_FORM_PATH 2
#define AKR_FORM_PATH_DEFER 3
#define AKR_FORM_PATH_SPEC 4
int akr_hip_render_form(akr_hip_ctx *ctx, int32_t *form, int32_t *ordered);
/* Which shading build the last path render ran (both give the same bits).  A persistent
 * form's product build runs the simple one when the committed material and light tables hold constant
 * Diffuse / Emissive only; its counting build, a persistent form on any other scene and the wavefront
 * kernels run the general one.  AKR_SHADING_NONE: nothing rendered. */
#define AKR_SHADING_NONE (-1)
#define AKR_SHADING_GENERAL 0
#define AKR_SHADING_SIMPLE 1
int akr_hip_render_shading(akr_hip_ctx *ctx, int32_t *shading);
/* The inputs of the last persistent render's form choice: its pixels per resident
 * lane x 1000, and the cost-ordering pilot's camera rays and their summed traversal steps; -1 when the
 * choice did not read the pilot (a forced form, no cost order, or a render too large for a tail form). */
int akr_hip_render_form_inputs(akr_hip_ctx *ctx, int64_t *pixels_per_lane_x1000, int64_t *pilot_rays,
                               int64_t *pilot_steps);
int akr_hip_synchronize(akr_hip_ctx *ctx);
/* Copies the first n records of the last render's pixel probe (see akr_pixel_probe); fails when
 * the last render ran without option "pixel_probe" or has fewer slots. */
int akr_hip_pixel_probe(akr_hip_ctx *ctx, akr_pixel_probe *out, uint64_t n);
/* Diagnostic: with option "ray_steps" set, each standalone trace (akr_hip_trace /
 * akr_hip_trace_device) runs the counting kernel and records, per ray, the traversal-loop
 * iterations it was active for plus its triangle tests (0xFFFFFFFF: traced by the exact BVH2
 * fallback); this copies the first n of the last trace to host memory. */
int akr_hip_ray_steps(akr_hip_ctx *ctx, uint32_t *out, uint64_t n);

#ifdef __cplusplus
}
#endif
#endif /* AKR_HIP_H */
