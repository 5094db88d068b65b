// kernels.h — host-side launchers of the gfx950 kernels (kernels.hip).
#pragma once
#include "akr_device.h"
#include "path_build.h"

namespace akr {

// TRACE_PILOT: closest-hit traversal that records only each ray's step count (a.ray_steps, capped at
// a.step_cap) for the cost-ordered fetch's pilot: no hits, no counters
enum : int { TRACE_CLOSEST = 0, TRACE_ANY = 1, TRACE_SHADOW = 2, TRACE_PILOT = 3 };

// tight = standard slab test (default); !tight = the reference's intersectAABB, bit for bit
void launch_trace(int mode, bool count, bool tight, bool wide, const TraceArgs &a, uint32_t grid, hipStream_t st);
int trace_blocks_per_cu(int mode);
void launch_raygen(const RaygenArgs &a, hipStream_t st);
// the wavefront shade kernel of a build (path_build.h): k_shade[_env][_spec][_mis].  env, m and d are read only
// where the build has them: an environment light, multiple importance sampling of lights
// (§3.18), a Mirror or a Glass in the scene (§3.19; under MIS the specular forms take m alone).  The film of the
// MIS and specular forms is splatted by launch_splat_mis over MisDev::E or SpecDev::E
void launch_shade(ShadeBuild b, const ShadeArgs &s, const EnvDev *env, const MisDev *m, const SpecDev *d, uint32_t max_items,
                  hipStream_t st);
void launch_splat(const SplatArgs &a, uint32_t max_items, hipStream_t st);
void launch_splat_mis(const SplatMisArgs &a, uint32_t max_items, hipStream_t st);
// the unit kernels of akr_hip_environment_sample (sample) / akr_hip_environment_eval
void launch_env_unit(bool sample, const EnvUnitArgs &a, hipStream_t st);
void launch_pick_form(const unsigned long long *sum, unsigned long long thresh, uint32_t *gate, hipStream_t st);
void launch_store_word(const uint32_t *src, uint32_t *dst, hipStream_t st);
void launch_ao_shade(const AoShadeArgs &a, uint32_t max_items, hipStream_t st);
void launch_ao_resolve(const AoResolveArgs &a, uint32_t max_items, hipStream_t st);
// persistent path kernel forms: the kernel of the build key (path_build.h; the
// table in DESIGN.md §0.5), with tab dropped when the tables do not fit LDS.  env is read by the key's
// environment builds only (options env_path and env_forms)
void launch_path(PathBuild b, const PathArgs &a, const AKR_GLOBAL EnvDev *env, uint32_t grid, hipStream_t st);
int path_blocks_per_cu(PathBuild b);  // of the key's product build (count = false)
bool path_tab_fits(int32_t n_mats, int32_t n_lights);
void launch_check_weights(const float4 *film, uint32_t n, float expect, uint32_t *bad, hipStream_t st);
void launch_merge_film(const float4 *film, const uint32_t *pixel, const uint32_t *order, uint32_t n, int32_t width,
                       float *rad, float *w, hipStream_t st);
void launch_unpack(const float4 *film, uint32_t n, float *rad, float *w, hipStream_t st);
void launch_expand_pixels(const uint4 *tiles, uint32_t n_tiles, uint32_t n, uint32_t *pixel, hipStream_t st);
void launch_probe_seed(const uint32_t *seed, uint32_t n, uint4 *probe, hipStream_t st);
void launch_probe_cost(const uint4 *probe, uint32_t n, uint32_t *cost, hipStream_t st);
// cost-ordered pixel fetch: pilot camera rays, sort keys, and the stable key sort (lbvh.hip, rocPRIM)
// 5-bit cost classes (31 = the costliest, with the rays the pilot does not trace): with the shard's 3 bits
// the key is one byte, so the radix sort is a single 8-bit pass (12-bit classes took 17 kernel launches,
// ~0.11 ms; the pilot's 64-step cap at the default shift 2 needs 17 classes)
constexpr uint32_t kOrderClassBits = 5, kOrderClassMask = (1u << kOrderClassBits) - 1u;
void launch_pilot_rays(const CameraDev &cam, const uint32_t *pixel, uint32_t n, uint32_t sub, float4 *rays,
                       hipStream_t st);
void launch_order_keys(const uint32_t *steps, uint32_t n, uint32_t shift, uint32_t cmax, uint32_t sub, uint32_t *key,
                       uint32_t *idx, hipStream_t st, unsigned long long *sum = nullptr);
size_t pixel_order_tmp_bytes(uint32_t n);
void sort_pixel_order(void *tmp, size_t tmp_bytes, const uint32_t *key_in, uint32_t *key_out, const uint32_t *idx_in,
                      uint32_t *idx_out, uint32_t n, hipStream_t st);

// adaptive sampling: mask -> ascending list of active slots (per-wave counts, their
// exclusive scan by rocPRIM in lbvh.hip, the scatter), per-slot expected counts, the convergence test
void launch_mask_count(const uint8_t *mask, uint32_t n, uint32_t *wcount, hipStream_t st);
size_t scan_tmp_bytes(uint32_t n);
void scan_exclusive_u32(void *tmp, size_t tmp_bytes, const uint32_t *in, uint32_t *out, uint32_t n, hipStream_t st);
void launch_mask_compact(const uint8_t *mask, uint32_t n, const uint32_t *woff, uint32_t *list, uint32_t *total,
                         hipStream_t st);
void launch_fill_u32(uint32_t *p, uint32_t n, uint32_t v, hipStream_t st);
void launch_count_add(uint32_t *count, const uint32_t *list, uint32_t n, uint32_t spp, hipStream_t st);
void launch_check_counts(const float4 *film, const uint32_t *count, uint32_t n, uint32_t *bad, hipStream_t st);
void launch_count_range(const uint32_t *count, const uint32_t *list, uint32_t n, uint32_t *out, hipStream_t st);
void launch_init_seed(const uint32_t *pixel, uint32_t n, int32_t width, uint32_t *seed, hipStream_t st);
void launch_probe_fill(const uint32_t *seed, uint32_t n, uint4 *probe, uint32_t flags, hipStream_t st);
void launch_adaptive_test(const float4 *film, float4 *prev, uint32_t n, float threshold, float *strip_err,
                          uint8_t *strip_active, uint8_t *mask, hipStream_t st);

// feature pass: sample k's camera ray of every slot from the slot's own chain
// (seed[i], or x + y * width when `first`), and the hit's albedo / normal / depth / position sums
void launch_feature_rays(const CameraDev &cam, const uint32_t *pixel, uint32_t n, uint32_t *seed, bool first,
                         float4 *rays, hipStream_t st);
void launch_feature_shade(const FeatureArgs &a, hipStream_t st);
// with an active thin lens: k_raygen's and k_feature_rays' lens forms
void launch_raygen_lens(const RaygenLensArgs &a, hipStream_t st);
void launch_feature_rays_lens(const CameraDev &cam, const LensDev &lens, const uint32_t *pixel, uint32_t n, uint32_t *seed,
                              bool first, float4 *rays, hipStream_t st);

// edge-avoiding a-trous filter of the film (denoise.hip): frame-ordered buffers of n = W * H
// pixels; guide = 3 float4 per pixel (unit normal | depth, position | 0, albedo | 0), I = (colour | state)
struct DenoiseArgs {
    const float4 *guide;
    const float4 *in;
    float4 *out;
    int32_t width, height, step, squarings;
    int32_t color_stop;                     // sigma_color > 0
    float sigma_depth, sigma_albedo, sc2;   // sc2: sc * sc of this iteration, sc = sigma_color * (1 / step)
};
void launch_denoise_prep(const float *radiance, const float *weight, const float *features, uint32_t n, bool demodulate,
                         float4 *guide, float4 *I, hipStream_t st);
void launch_denoise_atrous(const DenoiseArgs &a, hipStream_t st);
void launch_denoise_finish(const float4 *guide, const float4 *I, uint32_t n, bool demodulate, float *out_rgb,
                           hipStream_t st);

// the variance-guided filter: DenoiseArgs with a ping-pong pair of its own for the variance
// record V = (variance of the demodulated mean | hv as 1 or 0)
struct DenoiseGuidedArgs {
    DenoiseArgs d;
    const float4 *vin;
    float4 *vout;
    float sv3;  // (3 * sigma_variance) * sigma_variance
};
void launch_denoise_prep_variance(const float *variance, const float4 *guide, const float4 *I, uint32_t n, bool demodulate,
                                  float4 *V, hipStream_t st);
void launch_denoise_atrous_guided(const DenoiseGuidedArgs &a, hipStream_t st);
// the film variance tracker: P = each slot's film at its last update, M = (M2r, M2g, M2b, K)
void launch_variance_update(const float4 *film, uint32_t n, float4 *P, float4 *M, hipStream_t st);
void launch_variance_resolve(const float4 *film, const float4 *M, uint32_t n, float *out, hipStream_t st);

}  // namespace akr
