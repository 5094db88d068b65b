// akari_hip.hpp — C++17 host adapter over the C-ABI (include/akr_hip.h).
//
// Mirrors the reference's plug-in interface for the hot path so the MI355X backend drops in
// beside EmbreeAccelerator / BVHAccelerator and the CPU/GPU integrators:
//
//   akari::hip::HipAccelerator   ~ Accelerator concept: build(scene), intersect(ray, isct),
//                                  occlude(ray)   (kernel/bvh-accelerator.h:673-682,
//                                  kernel/embree.inl:37-45; dispatch kernel/scene.cpp:26-81)
//   akari::hip::HipPathTracer    ~ gpu::PathTracer / cpu::PathTracer with
//                                  render(scene, film)  (kernel/integrators/gpu/integrator.h:39-59,
//                                  core/nodes/integrator.cpp:50-84)
//   akari::hip::Film             ~ Film<C>: Pixel{radiance, weight} (core/film.h:31-113)
//
// Errors: a non-zero C-ABI status becomes std::runtime_error (the AKR_ASSERT_THROW convention,
// common/panic.h:52-57) carrying akr_hip_last_error().
#pragma once
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <cmath>
#include <algorithm>
#include <string>
#include <limits>
#include <utility>
#include <vector>

#include "../../include/akr_hip.h"

namespace akari::hip {

inline void check(akr_hip_ctx *ctx, int status, const char *what) {
    if (status != 0)
        throw std::runtime_error(std::string(what) + ": " + (ctx ? akr_hip_last_error(ctx) : "no context"));
}

// Flat mesh view, the MeshInstance<C> fields (kernel/instance.h:30-35).
struct MeshView {
    const float *vertices = nullptr;     // 3 * n_vertices
    uint64_t n_vertices = 0;
    const int32_t *indices = nullptr;    // 3 * n_triangles
    const float *normals = nullptr;      // 9 * n_triangles
    const float *texcoords = nullptr;    // 6 * n_triangles
    const int32_t *material_indices = nullptr;
    uint64_t n_triangles = 0;
    std::vector<int32_t> material_slots; // mesh-local material index -> scene material index
};

struct SceneDesc {
    std::vector<MeshView> meshes;
    std::vector<akr_texture> textures;
    std::vector<akr_material> materials;
    std::vector<akr_area_light> lights;
    std::vector<float> light_power;      // SceneNode::compile power weights (core/nodes/scene.cpp:72-87)
    akr_camera camera{};
};

// Mirror and Glass, which the reference lacks: the records SceneDesc::materials takes.
// `color` names a texture (reflectance / tint); a Glass's `ior` names a constant texture whose x is the index
// of refraction, carried in akr_material::roughness.
inline akr_material mirror_material(int32_t color) {
    akr_material m{AKR_MAT_MIRROR, color, -1, -1, -1, -1, 0};
    return m;
}
inline akr_material glass_material(int32_t color, int32_t ior) {
    akr_material m{AKR_MAT_GLASS, color, ior, -1, -1, -1, 0};
    return m;
}

class HipAccelerator {
  public:
    explicit HipAccelerator(int device = 0) {
        int st = akr_hip_create(device, &ctx_);
        if (st != 0) throw std::runtime_error("akr_hip_create failed (no HIP device " + std::to_string(device) + ")");
    }
    ~HipAccelerator() { akr_hip_destroy(ctx_); }
    HipAccelerator(const HipAccelerator &) = delete;
    HipAccelerator &operator=(const HipAccelerator &) = delete;

    // BVHAccelerator::build(Scene<C>&): uploads the flat scene and builds the BVH on the host.
    void build(const SceneDesc &s, const akr_build_params *params = nullptr) {
        check(ctx_, akr_hip_upload_textures(ctx_, s.textures.data(), (int32_t)s.textures.size()), "upload_textures");
        check(ctx_, akr_hip_upload_materials(ctx_, s.materials.data(), (int32_t)s.materials.size()), "upload_materials");
        for (const auto &m : s.meshes) {
            int32_t gid = -1;
            check(ctx_, akr_hip_upload_mesh(ctx_, m.vertices, m.n_vertices, m.indices, m.normals, m.texcoords,
                                            m.material_indices, m.n_triangles, m.material_slots.data(),
                                            (int32_t)m.material_slots.size(), &gid),
                  "upload_mesh");
        }
        check(ctx_, akr_hip_upload_lights(ctx_, s.lights.data(), (int32_t)s.lights.size(), s.light_power.data()),
              "upload_lights");
        check(ctx_, akr_hip_set_camera(ctx_, &s.camera), "set_camera");
        check(ctx_, akr_hip_build_accel(ctx_, params), "build_accel");
    }
    // Scene<C>::intersect(ray, isct) -> bool (kernel/scene.cpp:26-45), batched on the device.
    void intersect(const std::vector<akr_ray> &rays, std::vector<akr_hit> &hits) const {
        hits.resize(rays.size());
        check(ctx_, akr_hip_trace(ctx_, rays.data(), rays.size(), hits.data(), 0), "trace");
    }
    bool intersect(const akr_ray &ray, akr_hit *isct) const {
        check(ctx_, akr_hip_trace(ctx_, &ray, 1, isct, 0), "trace");
        return isct->geom_id != -1 && isct->prim_id != -1;   // Intersection::hit (scene.h:48)
    }
    // Scene<C>::occlude(ray) -> bool (kernel/scene.cpp:46-63)
    void occlude(const std::vector<akr_ray> &rays, std::vector<uint8_t> &occluded) const {
        std::vector<akr_hit> hits(rays.size());
        check(ctx_, akr_hip_trace(ctx_, rays.data(), rays.size(), hits.data(), 1), "trace(any)");
        occluded.resize(rays.size());
        for (size_t i = 0; i < rays.size(); i++) occluded[i] = hits[i].geom_id != -1;
    }
    bool occlude(const akr_ray &ray) const {
        akr_hit h;
        check(ctx_, akr_hip_trace(ctx_, &ray, 1, &h, 1), "trace(any)");
        return h.geom_id != -1;
    }
    akr_accel_info info() const {
        akr_accel_info i;
        check(ctx_, akr_hip_accel_info(ctx_, &i), "accel_info");
        return i;
    }
    akr_hip_ctx *handle() const { return ctx_; }

  private:
    akr_hip_ctx *ctx_ = nullptr;
};

// Film<C> (core/film.h:72-113): per-pixel sum of radiance and weight; value = radiance / weight.
struct Film {
    int width = 0, height = 0;
    std::vector<float> radiance, weight;
    Film(int w, int h) : width(w), height(h), radiance(3 * (size_t)w * h, 0.0f), weight((size_t)w * h, 0.0f) {}
    void pixel(int x, int y, float rgb[3]) const {
        size_t p = (size_t)x + (size_t)y * width;
        float w = weight[p];
        for (int c = 0; c < 3; c++) rgb[c] = w != 0 ? radiance[3 * p + c] / w : radiance[3 * p + c];
    }
    // Film::write_image (core/film.h:97-113) with GammaCorrection (common/color.h:58-61) and the
    // 8-bit quantisation of DefaultImageWriter (core/image.cpp:38-60): row-major RGB bytes.  pow
    // in f64 rounded to f32 (the correctly rounded powf); identical to akari_amd/film.py.
    std::vector<uint8_t> srgb8() const {
        std::vector<uint8_t> out(3 * (size_t)width * height);
        for (int y = 0; y < height; y++)
            for (int x = 0; x < width; x++) {
                float rgb[3];
                pixel(x, y, rgb);
                for (int c = 0; c < 3; c++) {
                    const float L = rgb[c];
                    const float p = (float)std::pow((double)L, (double)(1.0f / 2.4f));
                    float s = L < 0.0031308f ? L * 12.92f : 1.055f * p - 0.055f;
                    if (!(s >= 0.0f)) s = 0.0f;  // clamp to [0, 1] (NaN -> 0)
                    if (s > 1.0f) s = 1.0f;
                    const int q = (int)std::round((double)s * 255.5);
                    out[3 * ((size_t)x + (size_t)y * width) + c] = (uint8_t)std::min(255, std::max(0, q));
                }
            }
        return out;
    }
    // 8-bit RGB PNG with stored (uncompressed) deflate blocks: no codec dependency.
    bool write_png(const std::string &path) const {
        const std::vector<uint8_t> rgb = srgb8();
        std::vector<uint8_t> raw;
        raw.reserve((size_t)height * (1 + 3 * (size_t)width));
        for (int y = 0; y < height; y++) {
            raw.push_back(0);  // filter type 0
            raw.insert(raw.end(), rgb.begin() + 3 * (size_t)y * width, rgb.begin() + 3 * (size_t)(y + 1) * width);
        }
        std::vector<uint8_t> z = {0x78, 0x01};
        for (size_t pos = 0; pos < raw.size() || pos == 0;) {
            const size_t n = std::min<size_t>(65535, raw.size() - pos);
            const bool last = pos + n >= raw.size();
            z.push_back(last ? 1 : 0);
            z.push_back((uint8_t)(n & 0xFF));
            z.push_back((uint8_t)(n >> 8));
            z.push_back((uint8_t)(~n & 0xFF));
            z.push_back((uint8_t)((~n >> 8) & 0xFF));
            z.insert(z.end(), raw.begin() + pos, raw.begin() + pos + n);
            pos += n;
            if (last) break;
        }
        uint32_t a = 1, b = 0;  // Adler-32 of the raw stream
        for (uint8_t c : raw) {
            a = (a + c) % 65521;
            b = (b + a) % 65521;
        }
        for (int k = 3; k >= 0; k--) z.push_back((uint8_t)(((b << 16) | a) >> (8 * k)));
        FILE *f = std::fopen(path.c_str(), "wb");
        if (!f) return false;
        static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
        std::fwrite(sig, 1, 8, f);
        auto be32 = [](std::vector<uint8_t> &v, uint32_t x) {
            for (int k = 3; k >= 0; k--) v.push_back((uint8_t)(x >> (8 * k)));
        };
        auto chunk = [&](const char *tag, const std::vector<uint8_t> &data) {
            std::vector<uint8_t> c;
            be32(c, (uint32_t)data.size());
            c.insert(c.end(), tag, tag + 4);
            c.insert(c.end(), data.begin(), data.end());
            uint32_t crc = 0xFFFFFFFFu;  // CRC-32 over tag + data
            for (size_t i = 4; i < c.size(); i++) {
                crc ^= c[i];
                for (int k = 0; k < 8; k++) crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
            }
            be32(c, crc ^ 0xFFFFFFFFu);
            std::fwrite(c.data(), 1, c.size(), f);
        };
        std::vector<uint8_t> ihdr;
        be32(ihdr, (uint32_t)width);
        be32(ihdr, (uint32_t)height);
        ihdr.insert(ihdr.end(), {8, 2, 0, 0, 0});
        chunk("IHDR", ihdr);
        chunk("IDAT", z);
        chunk("IEND", {});
        std::fclose(f);
        return true;
    }
    // Portable float map (no image codec dependency); write_image's divide-by-weight applied.
    bool write_pfm(const std::string &path) const {
        FILE *f = std::fopen(path.c_str(), "wb");
        if (!f) return false;
        std::fprintf(f, "PF\n%d %d\n-1.0\n", width, height);
        for (int y = height - 1; y >= 0; y--)
            for (int x = 0; x < width; x++) {
                float rgb[3];
                pixel(x, y, rgb);
                std::fwrite(rgb, sizeof(float), 3, f);
            }
        std::fclose(f);
        return true;
    }
};

// gpu::PathTracer<C> (spp, max_depth, tile_size, ray_clamp, wavefront) — always wavefront here.
class HipPathTracer {
  public:
    int spp = 16, max_depth = 5, tile_size = 256;
    float ray_clamp = 0.0f;   // <= 0: reference CPU semantics (no clamp); > 0: GPU clamp
    HipPathTracer() = default;
    HipPathTracer(int spp_, int max_depth_, int tile_size_, float ray_clamp_)
        : spp(spp_), max_depth(max_depth_), tile_size(tile_size_), ray_clamp(ray_clamp_) {}

    // render(const Scene<C>&, Film<C>*): accumulates every tile of the film
    void render(const HipAccelerator &scene, Film &film) const {
        std::vector<akr_rect> tiles;
        for (int y = 0; y < film.height; y += tile_size)
            for (int x = 0; x < film.width; x += tile_size) tiles.push_back({x, y, x + tile_size, y + tile_size});
        akr_pt_params p{spp, max_depth, ray_clamp, 0};
        check(scene.handle(),
              akr_hip_render(scene.handle(), &p, tiles.data(), (int32_t)tiles.size(), film.radiance.data(),
                             film.weight.data()),
              "render");
    }

    // Environment light (include/akr_hip.h): an n x n octahedral map (rgb: 3 n n floats,
    // row-major), lit by importance-sampled direct lighting and seen by camera rays that leave the scene.
    // world_to_env: row-major 3x3 of d_env = R d_world, or null for the identity.  Renders of a scene with an
    // environment take the wavefront form.  Ends the render session, like every upload.
    static void set_environment(const HipAccelerator &scene, int n, const float *rgb, const float *world_to_env = nullptr,
                                float scale = 1.0f, float select_prob = 0.5f) {
        akr_environment e{};
        e.resolution = n;
        e.select_prob = select_prob;
        for (int c = 0; c < 3; c++) e.scale[c] = scale;
        for (int c = 0; c < 9; c++) e.world_to_env[c] = world_to_env ? world_to_env[c] : (c % 4 == 0 ? 1.0f : 0.0f);
        if (!rgb) throw std::runtime_error("set_environment: null map (clear_environment removes one)");
        check(scene.handle(), akr_hip_upload_environment(scene.handle(), &e, rgb), "upload_environment");
    }
    static void clear_environment(const HipAccelerator &scene) {
        check(scene.handle(), akr_hip_upload_environment(scene.handle(), nullptr, nullptr), "upload_environment");
    }

    // Thin lens (include/akr_hip.h): PerspectiveCamera's lens_radius and focal_distance
    // (kernel/camera.h:43-44, 75-80), both finite and >= 0; (0, 0) is the pinhole.  With both > 0 the renders take
    // the wavefront form.  Ends the render session; HipAccelerator::build (akr_hip_set_camera) leaves it alone.
    static void set_lens(const HipAccelerator &scene, float radius, float focal) {
        check(scene.handle(), akr_hip_set_lens(scene.handle(), radius, focal), "set_lens");
    }

    // Render sessions (include/akr_hip.h): the accelerator's context remembers its last render(), and
    // render_continue adds `more` samples per pixel from where it stopped; the film is cleared and then
    // holds the session's totals, bit for bit the film of one render() of all the samples.
    void render_continue(const HipAccelerator &scene, int more, Film &film) const {
        std::fill(film.radiance.begin(), film.radiance.end(), 0.0f);
        std::fill(film.weight.begin(), film.weight.end(), 0.0f);
        check(scene.handle(), akr_hip_render_continue(scene.handle(), more, film.radiance.data(), film.weight.data()),
              "render_continue");
    }
    // the totals into packed device buffers (radiance[3n], weight[n]) on `stream`; returns the slot count
    uint64_t render_continue_device(const HipAccelerator &scene, int more, float *d_radiance, float *d_weight,
                                    void *stream = nullptr) const {
        uint64_t n = 0;
        check(scene.handle(), akr_hip_render_continue_device(scene.handle(), more, d_radiance, d_weight, stream, &n),
              "render_continue_device");
        return n;
    }
    akr_render_state_info render_state_info(const HipAccelerator &scene) const {
        akr_render_state_info i;
        check(scene.handle(), akr_hip_render_state_info(scene.handle(), &i), "render_state_info");
        return i;
    }
    // the session's sampler states [n] and film sums [4n] (r, g, b, weight), packed tile order
    void render_state_export(const HipAccelerator &scene, std::vector<uint32_t> &sampler, std::vector<float> &sums) const {
        const uint64_t n = render_state_info(scene).n_pixels;
        sampler.resize(n);
        sums.resize(4 * n);
        check(scene.handle(), akr_hip_render_state_export(scene.handle(), sampler.data(), sums.data(), n),
              "render_state_export");
    }
    // a session as if spp_done samples of this tracer had been rendered over a width x height film
    void render_state_import(const HipAccelerator &scene, int width, int height, int spp_done,
                             const std::vector<uint32_t> &sampler, const std::vector<float> &sums) const {
        if (sums.size() != 4 * sampler.size()) throw std::runtime_error("render_state_import: four sums per sampler state");
        std::vector<akr_rect> tiles;
        for (int y = 0; y < height; y += tile_size)
            for (int x = 0; x < width; x += tile_size) tiles.push_back({x, y, x + tile_size, y + tile_size});
        akr_pt_params p{spp_done, max_depth, ray_clamp, 0};
        check(scene.handle(),
              akr_hip_render_state_import(scene.handle(), &p, tiles.data(), (int32_t)tiles.size(), sampler.data(),
                                          sums.data(), sampler.size()),
              "render_state_import");
    }

    // Adaptive sampling (include/akr_hip.h).  render_continue_masked: `more` samples for
    // the slots whose byte of `mask` (packed tile order, one per slot of the session) is non-zero; the
    // film is cleared and then holds the session's totals.
    void render_continue_masked(const HipAccelerator &scene, int more, const std::vector<uint8_t> &mask, Film &film) const {
        std::fill(film.radiance.begin(), film.radiance.end(), 0.0f);
        std::fill(film.weight.begin(), film.weight.end(), 0.0f);
        check(scene.handle(),
              akr_hip_render_continue_masked(scene.handle(), more, mask.data(), mask.size(), film.radiance.data(),
                                             film.weight.data()),
              "render_continue_masked");
    }
    // this tracer's spp is the cap: min_spp for every pixel, then passes over the 64-slot strips whose
    // error is above `threshold` (pass_spp 0: each pass doubles their count); accumulates into the film
    akr_adaptive_info render_adaptive(const HipAccelerator &scene, Film &film, float threshold, int min_spp = 16,
                                      int pass_spp = 0) const {
        std::vector<akr_rect> tiles;
        for (int y = 0; y < film.height; y += tile_size)
            for (int x = 0; x < film.width; x += tile_size) tiles.push_back({x, y, x + tile_size, y + tile_size});
        akr_pt_params p{spp, max_depth, ray_clamp, 0};
        akr_adaptive_params ap{min_spp, pass_spp, threshold, 0};
        akr_adaptive_info info;
        check(scene.handle(),
              akr_hip_render_adaptive(scene.handle(), &p, &ap, tiles.data(), (int32_t)tiles.size(), film.radiance.data(),
                                      film.weight.data(), &info),
              "render_adaptive");
        return info;
    }
    // the last convergence test: each strip's error and whether it is still active
    void adaptive_error(const HipAccelerator &scene, std::vector<float> &strip_error,
                        std::vector<uint8_t> &strip_active) const {
        const uint64_t n = (render_state_info(scene).n_pixels + 63) / 64;
        strip_error.resize(n);
        strip_active.resize(n);
        check(scene.handle(), akr_hip_adaptive_error(scene.handle(), strip_error.data(), strip_active.data(), n),
              "adaptive_error");
    }
    // the smallest and the largest sample count of the session's slots
    std::pair<int, int> render_state_spp_range(const HipAccelerator &scene) const {
        int32_t lo = 0, hi = 0;
        check(scene.handle(), akr_hip_render_state_spp_range(scene.handle(), &lo, &hi), "render_state_spp_range");
        return {lo, hi};
    }

    // Feature buffers and the a-trous filter of the film (include/akr_hip.h); both keep the
    // session.  render_features: `feature_spp` camera samples per pixel of the film's tiles; `features` is
    // cleared and then holds the 12 sums per pixel (albedo rgb, hits, normal xyz, t, position xyz, 0).
    void render_features(const HipAccelerator &scene, const Film &film, int feature_spp, std::vector<float> &features) const {
        std::vector<akr_rect> tiles;
        for (int y = 0; y < film.height; y += tile_size)
            for (int x = 0; x < film.width; x += tile_size) tiles.push_back({x, y, x + tile_size, y + tile_size});
        features.assign(12 * (size_t)film.width * film.height, 0.0f);
        akr_feature_params p{feature_spp, 0};
        check(scene.handle(), akr_hip_render_features(scene.handle(), &p, tiles.data(), (int32_t)tiles.size(), features.data()),
              "render_features");
    }
    // the film filtered with `p`, guided by `features`: the mean colour, 3 floats per pixel
    static akr_denoise_params denoise_defaults() { return akr_denoise_params{5, 5, 0.02f, 0.3f, 0.5f, 0, {0, 0}}; }
    void denoise(const HipAccelerator &scene, const Film &film, const std::vector<float> &features,
                 std::vector<float> &out_rgb, const akr_denoise_params &p = denoise_defaults()) const {
        if (features.size() != 12 * film.weight.size()) throw std::runtime_error("denoise: twelve feature sums per pixel");
        out_rgb.assign(film.radiance.size(), 0.0f);
        check(scene.handle(),
              akr_hip_denoise(scene.handle(), &p, film.width, film.height, film.radiance.data(), film.weight.data(),
                              features.data(), out_rgb.data()),
              "denoise");
    }

    // Film variance from the session's passes and the variance-guided filter (include/akr_hip.h, DESIGN.md
    // §3.16).  track_variance before the render that starts the session; render_variance: `variance` is
    // cleared and then holds (vr, vg, vb, K) per pixel, the variance of the mean colour and the batch count.
    void track_variance(const HipAccelerator &scene, bool on = true) const {
        check(scene.handle(), akr_hip_set_option(scene.handle(), "film_variance", on ? 1 : 0), "track_variance");
    }
    // Multiple importance sampling of lights (option "mis", include/akr_hip.h): before the
    // render that starts the session; a continue keeps the session's value.
    void set_mis(const HipAccelerator &scene, bool on = true) const {
        check(scene.handle(), akr_hip_set_option(scene.handle(), "mis", on ? 1 : 0), "set_mis");
    }
    // Under an environment light, let the persistent path kernel render where option "path" takes it (option
    // "env_path", include/akr_hip.h): read at every render and continue; the same bits.
    void set_env_path(const HipAccelerator &scene, bool on = true) const {
        check(scene.handle(), akr_hip_set_option(scene.handle(), "env_path", on ? 1 : 0), "set_env_path");
    }
    // ... and let the form rule choose among k_path, k_path_defer and k_path_spec as it does without an
    // environment (option "env_forms"): acts with set_env_path(true) only; the same bits.
    void set_env_forms(const HipAccelerator &scene, bool on = true) const {
        check(scene.handle(), akr_hip_set_option(scene.handle(), "env_forms", on ? 1 : 0), "set_env_forms");
    }
    void render_variance(const HipAccelerator &scene, const Film &film, std::vector<float> &variance) const {
        variance.assign(4 * (size_t)film.width * film.height, 0.0f);
        check(scene.handle(), akr_hip_render_variance(scene.handle(), variance.data()), "render_variance");
    }
    static akr_denoise_guided_params denoise_guided_defaults() {
        return akr_denoise_guided_params{denoise_defaults(), 2.0f, {0, 0, 0}};
    }
    void denoise_guided(const HipAccelerator &scene, const Film &film, const std::vector<float> &features,
                        const std::vector<float> &variance, std::vector<float> &out_rgb,
                        const akr_denoise_guided_params &p = denoise_guided_defaults()) const {
        if (features.size() != 12 * film.weight.size()) throw std::runtime_error("denoise: twelve feature sums per pixel");
        if (variance.size() != 4 * film.weight.size()) throw std::runtime_error("denoise: four variance floats per pixel");
        out_rgb.assign(film.radiance.size(), 0.0f);
        check(scene.handle(),
              akr_hip_denoise_guided(scene.handle(), &p, film.width, film.height, film.radiance.data(), film.weight.data(),
                                     features.data(), variance.data(), out_rgb.data()),
              "denoise_guided");
    }

    // Multi-GPU in one process (akr_hip_render_node): tile j on accelerators[j % n], one per device,
    // each built from the same scene; the merged film equals render() on one of them.
    void render_node(const std::vector<const HipAccelerator *> &accels, Film &film) const {
        if (accels.empty()) throw std::runtime_error("render_node: no accelerators");
        std::vector<akr_rect> tiles;
        for (int y = 0; y < film.height; y += tile_size)
            for (int x = 0; x < film.width; x += tile_size) tiles.push_back({x, y, x + tile_size, y + tile_size});
        std::vector<akr_hip_ctx *> h;
        for (auto *a : accels) h.push_back(a->handle());
        akr_pt_params p{spp, max_depth, ray_clamp, 0};
        check(h[0],
              akr_hip_render_node(h.data(), (int32_t)h.size(), &p, tiles.data(), (int32_t)tiles.size(),
                                  film.radiance.data(), film.weight.data()),
              "render_node");
    }
};

// cpu::AmbientOcclusion<C> (spp, occlude; kernel/integrators/cpu/integrator.h:35-45), rendered on
// the GPU through akr_hip_render_ao.
class HipAmbientOcclusion {
  public:
    int spp = 16, tile_size = 16;
    float occlude = std::numeric_limits<float>::infinity();
    HipAmbientOcclusion() = default;
    HipAmbientOcclusion(int spp_, float occlude_) : spp(spp_), occlude(occlude_) {}

    void render(const HipAccelerator &scene, Film &film) const {
        const int ts = std::max(16, tile_size);  // one call renders every tile: size is a batching knob
        std::vector<akr_rect> tiles;
        for (int y = 0; y < film.height; y += ts)
            for (int x = 0; x < film.width; x += ts) tiles.push_back({x, y, x + ts, y + ts});
        akr_ao_params p{spp, occlude, 0, 0};
        check(scene.handle(),
              akr_hip_render_ao(scene.handle(), &p, tiles.data(), (int32_t)tiles.size(), film.radiance.data(),
                                film.weight.data()),
              "render_ao");
    }
};

}  // namespace akari::hip
