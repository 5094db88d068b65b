// capi.hip — implementation of the C-ABI boundary declared in include/akr_hip.h.
//
// One context = one device + one stream.  Scene arrays are staged on the host, flattened across
// meshes (global triangle id = mesh base + prim id) and uploaded once; the BVH is built on the
// host (bvh_build.cpp) and uploaded.  akr_hip_render runs the wavefront pipeline
// raygen -> {closest-hit -> shade -> shadow}^depth -> splat once per sample pass, entirely on
// the stream (no host synchronisation inside a render; queue counts live in device memory).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "akr_device.h"
#include "bvh_build.h"
#include "kernels.h"
#include "options.h"
#include "leaf_layout.h"
#include "path_plan.h"
#include "session.h"
#include "shade_simple.h"
#include "tile_layout.h"

using namespace akr;

#define HIPCHK(x)                                                                                        \
    do {                                                                                                 \
        hipError_t e_ = (x);                                                                             \
        if (e_ != hipSuccess) throw std::runtime_error(std::string(#x) + " failed: " + hipGetErrorString(e_)); \
    } while (0)

namespace {

template <class T>
struct DBuf {
    T *p = nullptr;
    size_t n = 0;
    DBuf() = default;
    DBuf(const DBuf &) = delete;
    DBuf &operator=(const DBuf &) = delete;
    ~DBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    void reserve(size_t count) {
        if (count <= n && p) return;
        release();
        size_t c = std::max<size_t>(count, 1);
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&p), c * sizeof(T)));
        n = c;
    }
    void upload(const T *h, size_t count, hipStream_t st) {
        reserve(count);
        if (count) HIPCHK(hipMemcpyAsync(p, h, count * sizeof(T), hipMemcpyHostToDevice, st));
    }
};

struct Stat {
    uint64_t launches = 0;
    double total = 0, mn = 1e30, mx = 0;
};

// Camera (restated from core/nodes/camera.cpp:26-52 and kernel/camera.h:45-59)
struct M4 {
    float m[4][4];
};
M4 m_ident() {
    M4 r{};
    for (int i = 0; i < 4; i++) r.m[i][i] = 1.0f;
    return r;
}
M4 m_from(const float (&a)[16]) {
    M4 r;
    for (int i = 0; i < 16; i++) r.m[i / 4][i % 4] = a[i];
    return r;
}
M4 m_mul(const M4 &a, const M4 &b) {  // Matrix::operator*, math.h:93-101 (sequential dot)
    M4 r;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            float s = a.m[i][0] * b.m[0][j];
            s += a.m[i][1] * b.m[1][j];
            s += a.m[i][2] * b.m[2][j];
            s += a.m[i][3] * b.m[3][j];
            r.m[i][j] = s;
        }
    return r;
}
float hsinf(float x) { return (float)std::sin((double)x); }
float hcosf(float x) { return (float)std::cos((double)x); }
M4 m_scale(float x, float y, float z) { return m_from({x, 0, 0, 0, 0, y, 0, 0, 0, 0, z, 0, 0, 0, 0, 1}); }
M4 m_translate(float x, float y, float z) { return m_from({1, 0, 0, x, 0, 1, 0, y, 0, 0, 1, z, 0, 0, 0, 1}); }
M4 m_rx(float t) { float s = hsinf(t), c = hcosf(t); return m_from({1, 0, 0, 0, 0, c, -s, 0, 0, s, c, 0, 0, 0, 0, 1}); }
M4 m_ry(float t) { float s = hsinf(t), c = hcosf(t); return m_from({c, 0, s, 0, 0, 1, 0, 0, -s, 0, c, 0, 0, 0, 0, 1}); }
M4 m_rz(float t) { float s = hsinf(t), c = hcosf(t); return m_from({c, -s, 0, 0, s, c, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}); }

CameraDev make_camera(const akr_camera &c) {
    const float pi = 3.1415926535897932384f;
    if (c.resolution[0] <= 0 || c.resolution[1] <= 0 || c.resolution[0] > 65535 || c.resolution[1] > 65535)
        throw std::runtime_error("camera resolution must be in [1, 65535]");
    CameraDev cam;
    cam.width = c.resolution[0];
    cam.height = c.resolution[1];
    float rx = c.rotation_deg[0] * pi / 180.0f, ry = c.rotation_deg[1] * pi / 180.0f, rz = c.rotation_deg[2] * pi / 180.0f;
    M4 c2w = m_rz(rz);
    c2w = m_mul(m_rx(ry), c2w);
    c2w = m_mul(m_ry(rx), c2w);
    c2w = m_mul(m_translate(c.position[0], c.position[1], c.position[2]), c2w);
    float fov = (float)(c.fov_deg * (double)pi / 180.0);
    M4 m = m_ident();
    m = m_mul(m_scale(1.0f / cam.width, 1.0f / cam.height, 1), m);
    m = m_mul(m_scale(2, 2, 1), m);
    m = m_mul(m_translate(-1, -1, 0), m);
    m = m_mul(m_scale(1, -1, 1), m);
    float s = (float)std::atan((double)(fov / 2));  // atan, not tan (camera.h:51)
    if (cam.width > cam.height)
        m = m_mul(m_scale(s, s * float(cam.height) / cam.width, 1), m);
    else
        m = m_mul(m_scale(s * float(cam.width) / cam.height, s, 1), m);
    for (int i = 0; i < 16; i++) {
        cam.r2c[i] = m.m[i / 4][i % 4];
        cam.c2w[i] = c2w.m[i / 4][i % 4];
    }
    return cam;
}

// Mapped host words written by kernels (k_store_word) are set to this by the host before the
// store is issued.  The host never acts on a value it has not seen change from the sentinel, so a
// stale read (a store not yet visible when the event it waited on completed, or a value left by an
// earlier render) can only delay a decision, never make a wrong one.
constexpr uint32_t kMappedSentinel = 0xFFFFFFFFu;

// Waits (up to ~2 s) until a mapped word no longer holds the sentinel; returns the sentinel if it
// never changes.
uint32_t read_mapped(const volatile uint32_t *p) {
    const auto t0 = std::chrono::steady_clock::now();
    while (true) {
        const uint32_t v = *p;
        if (v != kMappedSentinel) return v;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) return kMappedSentinel;
        std::this_thread::yield();
    }
}

}  // namespace

struct akr_hip_ctx {
    int device = 0;
    int n_cu = 256;
    hipStream_t stream = nullptr;
    std::string err;
    Options opt;  // every knob akr_hip_set_option sets (options.h)
    // Every trace / render of a context is ordered after the previous one, whatever streams the
    // caller passes: they share the refill counters, the overflow stacks and the queues.
    hipEvent_t ev_done = nullptr;
    bool done_recorded = false;
    // the in-band film check (option "verify"): device counter + mapped host word
    DBuf<uint32_t> d_bad;
    uint32_t *h_check = nullptr, *d_check_host = nullptr;
    // Fault word (mapped, coherent host memory): a persistent kernel's hang guard sets it
    // (k_path_defer).  Checked after every render on the host, whatever "verify" says.
    uint32_t *h_fault = nullptr, *d_fault_host = nullptr;
    // Test-only per-slot fingerprint of the last render (option "pixel_probe", akr_pixel_probe)
    DBuf<uint4> d_probe;
    uint64_t probe_n = 0;
    bool probe_ok = false;

    // host staging (flattened over meshes)
    std::vector<float> verts;
    std::vector<int32_t> idx;
    std::vector<float> normals, texcoords;
    std::vector<int32_t> matid;
    std::vector<uint32_t> mesh_base{0};
    std::vector<akr_texture> texs;
    std::vector<akr_material> mats;
    std::vector<float> images;
    std::vector<int64_t> img_off;
    std::vector<int32_t> img_w, img_h;
    std::vector<akr_area_light> lights;
    std::vector<float> power;
    bool scene_dirty = true;
    bool accel_built = false;
    akr_accel_info info{};
    BvhOutput bvh;
    Bvh4Output bvh4;

    // device scene
    DBuf<akr_bvh_node> d_nodes;
    DBuf<akr_bvh4_node> d_wnodes;
    DBuf<float4> d_wleaves;          // leaf blob (see TraceArgs::wide_leaves)
    uint32_t wide_root_dev = AKR_CHILD_EMPTY;
    bool leaf_one_kernel = false;  // k_path's one-triangle leaf phase pays on this tree (leaf_layout.h leaf_one_pays)
    uint64_t bvh_dev_bytes = 0;       // the uploaded wide nodes + leaf blob
    DBuf<float4> d_tris;
    DBuf<ShadeTri> d_shade_tri;
    DBuf<float> d_tc, d_images, d_cdf, d_func;
    DBuf<MatDev> d_mats;
    DBuf<TexDev> d_texs;
    DBuf<LightDev> d_lights;
    DBuf<uint32_t> d_mesh_base;
    float func_int = 0;
    int32_t n_lights = 0;
    int32_t n_mats = 0;
    bool has_image_tex = false;
    bool simple_shading = true;  // every material Diffuse / Emissive with constant textures
    // the committed tables allow the persistent kernels' simple shading build (shade_simple.h); set by every
    // commit_scene(), so it follows the scene a render sees.  simple_shading above chooses the form, this
    // the build: an image texture no material uses keeps the wavefront form but not the general build
    bool shade_simple = false;
    int32_t last_shading = AKR_SHADING_NONE;  // akr_hip_render_shading

    CameraDev cam{};
    bool cam_set = false;
    // The thin lens, akr_hip_set_lens: (0, 0) is the pinhole.  Where it is active the camera
    // rays of the wavefront render, the AO render and the feature pass come from the lens kernels, and render()
    // takes the wavefront form; the context's lens decides at every call, continues included.
    LensDev lens{0.0f, 0.0f};
    bool lens_active() const { return lens.radius > 0 && lens.focal > 0; }  // camera.h:75
    void raygen_launch(const RaygenArgs &rg, hipStream_t st) {
        if (lens_active()) launch_raygen_lens(RaygenLensArgs{rg, lens}, st);
        else launch_raygen(rg, st);
    }

    // Environment light: the map and the tables of its distribution, built by
    // akr_hip_upload_environment; env.n == 0: none.  A scene with one renders in the wavefront form.
    EnvDev env{};
    DBuf<float4> d_env_map;
    DBuf<float> d_env_tab;  // marginal CDF, marginal pdf, conditional CDFs, conditional pdfs
    // `env` itself on the device, for k_path's environment build, which reads it behind one pointer (option
    // env_path); copied by the first such render after an upload, so nothing is allocated or
    // copied while the option is off
    DBuf<EnvDev> d_env_rec;
    bool env_rec_stale = true;
    const AKR_GLOBAL EnvDev *env_rec(hipStream_t st) {
        if (env_rec_stale) {
            d_env_rec.upload(&env, 1, st);
            env_rec_stale = false;
        }
        return (const AKR_GLOBAL EnvDev *)d_env_rec.p;
    }
    bool env_on() const { return env.n > 0; }
    const EnvDev &require_env() const {
        if (!env_on()) throw std::runtime_error("no environment light (akr_hip_upload_environment)");
        return env;
    }

    // path / queue buffers
    size_t cap = 0;
    // The last render's tiles and slot count (tile_layout.h).  The pixel list is expanded from them on the
    // device (k_expand_pixels); the host copy h_pixel is built only for the host-side merges that need it
    // (host_pixels()).
    TileLayout lay;
    DBuf<uint4> d_tiles;
    static_assert(sizeof(TileRec) == sizeof(uint4) && alignof(TileRec) == alignof(uint4) && offsetof(TileRec, x0) == offsetof(uint4, x) &&
                      offsetof(TileRec, y0) == offsetof(uint4, y) && offsetof(TileRec, width) == offsetof(uint4, z) &&
                      offsetof(TileRec, first) == offsetof(uint4, w),
                  "k_expand_pixels reads a TileRec as a uint4");
    // `l`'s tiles into `d` and every slot's pixel into `pixel`, on `st`
    static void expand_layout(const TileLayout &l, DBuf<uint4> &d, uint32_t *pixel, hipStream_t st) {
        d.upload(reinterpret_cast<const uint4 *>(l.tiles.data()), l.tiles.size(), st);
        launch_expand_pixels(d.p, (uint32_t)l.tiles.size(), (uint32_t)l.n, pixel, st);
    }
    // The session (session.h): the last path render, which akr_hip_render_continue extends.
    // Its slots are lay / d_pixel, its sampler states d_seed and its sums d_film.  Every render starts by
    // dropping it (setup_pixels); so do scene, tree and camera changes.
    Session session;
    void drop_session() { session.valid = false; }
    const Session &require_session() const { return akr::require_session(session); }
    // Adaptive sampling: the active-slot list of a subset pass and its compaction
    // scratch, the per-slot expected counts of a non-uniform session, and the convergence test's
    // snapshot, slot mask and per-strip results
    DBuf<uint32_t> d_count, d_active, d_wcount, d_woff, d_nactive, d_crange;
    DBuf<uint8_t> d_mask, d_scan_tmp, d_strip_active;
    DBuf<float> d_strip_err;
    DBuf<float4> d_prev;
    // Film variance tracker, for sessions started with option "film_variance": each slot's
    // film at its last update and (M2r, M2g, M2b, K), sized with the session; var_track is the option as the
    // session's first call read it.  d_var_out stages an export.
    DBuf<float4> d_var_prev, d_var_m2;
    DBuf<float> d_var_out;
    bool var_track = false;
    // A session starts: the tracker's state is zeroed (nothing is allocated or enqueued with the option off)
    void variance_begin(uint64_t N, hipStream_t st) {
        var_track = opt.film_variance;
        if (!var_track || N == 0) return;
        d_var_prev.reserve(N);
        d_var_m2.reserve(N);
        HIPCHK(hipMemsetAsync(d_var_prev.p, 0, N * sizeof(float4), st));
        HIPCHK(hipMemsetAsync(d_var_m2.p, 0, N * sizeof(float4), st));
    }
    // After the last kernel that writes d_film has been joined into `st`: one batch for every slot whose
    // weight grew
    void variance_update(uint64_t N, hipStream_t st) {
        if (!var_track || N == 0) return;
        if (d_var_prev.n < N || d_var_m2.n < N) throw std::runtime_error("film variance: the tracker's buffers changed");
        timed("variance_update", st, [&] { launch_variance_update(d_film.p, (uint32_t)N, d_var_prev.p, d_var_m2.p, st); });
        HIPCHK(hipGetLastError());
    }
    // (vr, vg, vb, K) of every slot into `out` (device, packed) on `st`; returns the slots
    uint64_t require_variance() const {
        const uint64_t N = require_session().n;
        if (!var_track)
            throw std::runtime_error("film variance: the session was started without option film_variance "
                                     "(set it to 1 before the render or import that starts the session)");
        return N;
    }
    uint64_t variance_resolve(float *out, hipStream_t st) {
        const uint64_t N = require_variance();
        serialize(st);
        if (N == 0) return 0;
        if (d_var_prev.n < N || d_var_m2.n < N) throw std::runtime_error("film variance: the tracker's buffers changed");
        timed("variance_resolve", st, [&] { launch_variance_resolve(d_film.p, d_var_m2.p, (uint32_t)N, out, st); });
        HIPCHK(hipGetLastError());
        return N;
    }
    // Multiple importance sampling of lights, for sessions started with option "mis": the
    // carried records (ping-ponged with the state queues), the terminal accumulator of each pass parity and
    // the per-triangle selection pdf.  mis_on is the option as the session's first call read it.  They are
    // sized for the session's slots, apart from ensure_capacity's set: growing them moves nothing else.
    DBuf<float4> d_carry[2], d_E[2];
    DBuf<float> d_tri_sel;
    std::vector<float> tri_sel;  // commit_scene: per global triangle id (the sum, if the list names it twice)
    bool tri_sel_dirty = true;
    bool mis_on = false;
    void mis_begin(uint64_t N, hipStream_t st) {
        mis_on = opt.mis;
        if (!mis_on || N == 0) return;
        for (int k = 0; k < 2; k++) {
            d_carry[k].reserve(N);
            d_E[k].reserve(N);
        }
        if (tri_sel_dirty) {
            d_tri_sel.upload(tri_sel.data(), tri_sel.size(), st);
            HIPCHK(hipStreamSynchronize(st));
            tri_sel_dirty = false;
        }
    }
    // Mirror and Glass, for renders of a scene that holds one: the via_delta flag
    // queues (ping-ponged with the state queues; the MIS builds keep the bit in d_carry instead) and d_E above.
    // spec_on is commit_scene()'s has_specular as the render call read it: the scene decides, not the session,
    // so render() asks at every call, and a continue of a session whose buffers stand reserves nothing.
    DBuf<uint32_t> d_spec_flag[2];
    bool has_specular = false;
    bool spec_on = false;
    void spec_begin(uint64_t N) {
        spec_on = has_specular;
        if (!spec_on || N == 0) return;
        for (int k = 0; k < 2; k++) {
            d_E[k].reserve(N);
            if (!mis_on) d_spec_flag[k].reserve(N);
        }
    }
    std::vector<uint32_t> h_pixel;
    bool h_pixel_ok = false;
    DBuf<uint32_t> d_pixel, d_seed, d_slot0, d_slot1, d_counts;
    DBuf<float4> d_ray0, d_ray1, d_state0, d_state1, d_hit, d_film;
    DBuf<float4> d_L[2];  // per-sample radiance, alternating by sample pass (passes overlap)
    DBuf<float4> d_sray[2], d_scolor[2];  // shadow queues, alternating by bounce
    DBuf<uint32_t> d_ao_slot[2];          // AO queues traced closest-hit (finite occlude): slots
    int last_passes = 0;
    int32_t last_form = AKR_FORM_NONE, last_ordered = 0;  // akr_hip_render_form
    // Shadow traces run on a second stream, so the shadow trace of bounce b overlaps the closest-hit
    // trace of bounce b+1 (independent work): each persistent launch's tail is filled by the other.
    // Both internal: `main` (high priority) runs raygen / closest-hit / shade, `side` (low priority)
    // runs shadow traces and splat, so the last shadow trace and splat of sample pass s overlap
    // raygen and the first closest-hit trace of pass s + 1.
    hipStream_t main_st = nullptr, side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_join_main = nullptr, ev_shade[2] = {nullptr, nullptr},
               ev_shadow[2] = {nullptr, nullptr}, ev_splat[2] = {nullptr, nullptr};
    DBuf<uint2> d_ovf, d_ovf_side;  // traversal stack overflow: main-stream and side-stream traces
    DBuf<uint32_t> d_work;  // dynamic-fetch counters of a standalone trace launch (kTraceWords)
    uint32_t ovf_threads = 0;
    uint32_t trace_grid[3] = {0, 0, 0};
    // resident workgroups of the persistent path kernels' product builds, by build_index (path_build.h): a
    // counting launch runs on its product build's grid.  ensure_trace_grid() fills every build without an
    // environment; an environment build (options env_path, env_forms) is queried when it first renders, and is
    // never above the grid the overflow stacks are sized for
    uint32_t path_grid[kPathBuilds] = {};
    uint32_t grid_of(PathBuild b) {
        b.count = false;
        uint32_t &g = path_grid[build_index(b)];
        if (!g) g = std::min<uint32_t>((uint32_t)(n_cu * path_blocks_per_cu(b)), ovf_threads / kTraceBlock);
        return g;
    }
    // the render form rule is plan_path() in path_plan.h; its knobs are in `opt`
    // the last render's form inputs (akr_hip_render_form_inputs): pixels per lane x 1000, the pilot's
    // rays and their summed steps
    int64_t last_ppl1000 = 0, last_pilot_rays = -1, last_pilot_steps = -1;
    DBuf<unsigned long long> d_steps_sum;   // the pilot's summed steps
    DBuf<uint32_t> d_gate;                  // k_pick_form's choice between the two launched forms
    // the last render launched two gated forms (gate_forms[gate]) / read the pilot's step sum on the
    // device: resolved on the host by resolve_form() when the form or its inputs are queried
    bool form_pending = false, pilot_sum_pending = false;
    int32_t gate_forms[2] = {AKR_FORM_NONE, AKR_FORM_NONE};
    DBuf<uint4> d_pprobe;  // the path pilot's per-slot probe
    DBuf<uint32_t> d_okey[2], d_oidx[2], d_owork;
    DBuf<uint8_t> d_otmp;
    DBuf<TraceCounters> d_ocnt;
    bool order_warm = false;
    DBuf<float4> d_contrib;   // k_path_defer: per-lane NEE contributions awaiting their shadow result
    DBuf<float4> d_trace_rays;
    DBuf<akr_hit> d_trace_hits;
    // akr_hip_render_node on the lead context: the frame and the staging of other contexts' films
    DBuf<float> d_frame;
    std::vector<std::unique_ptr<DBuf<float4>>> g_film;     // [k]: context k's packed film (staging)
    std::vector<std::unique_ptr<DBuf<uint32_t>>> g_pix;    // [k]: its pixel list
    DBuf<uint32_t> d_gorder;                               // merge orders of overlapping tiles
    hipEvent_t ev_gather = nullptr;  // this context's push to the lead device is done

    // instrumentation (its options: options.h)
    int wide_collapse = AKR_COLLAPSE_SAH;  // akr_build_params::wide_collapse of the last build
    DBuf<uint32_t> d_steps;
    uint64_t n_steps = 0;
    DBuf<TraceCounters> d_counters;
    DBuf<PathProfile> d_pprof;  // k_path counting build: per-wave phase profile
    // option count_lines: the bitmap of 128-B lines a render read, and the bit ranges of its three
    // regions (wide nodes, leaf blob, shading records)
    DBuf<uint32_t> d_lines;
    uint32_t lines_span[4] = {0, 0, 0, 0};
    std::vector<hipEvent_t> pool;
    struct Pending {
        const char *name;
        hipEvent_t a, b;
    };
    std::vector<Pending> pending;
    std::map<std::string, Stat> stat;

    ~akr_hip_ctx() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (auto &p : pending) {
            (void)hipEventDestroy(p.a);
            (void)hipEventDestroy(p.b);
        }
        for (auto e : pool) (void)hipEventDestroy(e);
        if (side) (void)hipStreamSynchronize(side);
        if (main_st) (void)hipStreamSynchronize(main_st);
        for (hipEvent_t e : {ev_fork, ev_join, ev_join_main, ev_shade[0], ev_shade[1], ev_shadow[0], ev_shadow[1], ev_splat[0], ev_splat[1]})
            if (e) (void)hipEventDestroy(e);
        if (h_check) (void)hipHostFree(h_check);
        if (h_fault) (void)hipHostFree(h_fault);
        if (ev_done) (void)hipEventDestroy(ev_done);
        if (ev_gather) (void)hipEventDestroy(ev_gather);
        if (main_st) (void)hipStreamDestroy(main_st);
        if (side) (void)hipStreamDestroy(side);
        if (stream) (void)hipStreamDestroy(stream);
    }

    hipEvent_t event() {
        if (!pool.empty()) {
            hipEvent_t e = pool.back();
            pool.pop_back();
            return e;
        }
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        return e;
    }

    template <class F>
    void timed(const char *name, hipStream_t st, F &&launch) {
        if (!opt.stats_on() || (opt.stats_closest_only() && std::strcmp(name, "trace_closest") != 0 && std::strcmp(name, "path") != 0)) {
            launch();
            return;
        }
        hipEvent_t a = event(), b = event();
        HIPCHK(hipEventRecord(a, st));
        launch();
        HIPCHK(hipEventRecord(b, st));
        pending.push_back({name, a, b});
        if (pending.size() > 4096) flush_stats();
    }

    void flush_stats() {
        for (auto &p : pending) {
            HIPCHK(hipEventSynchronize(p.b));
            float ms = 0;
            HIPCHK(hipEventElapsedTime(&ms, p.a, p.b));
            Stat &s = stat[p.name];
            s.launches++;
            s.total += ms;
            s.mn = std::min(s.mn, (double)ms);
            s.mx = std::max(s.mx, (double)ms);
            pool.push_back(p.a);
            pool.push_back(p.b);
        }
        pending.clear();
    }

    SceneDev scene_dev() const {
        SceneDev s{};
        s.tri = (decltype(s.tri))d_shade_tri.p;  // device code sees them as global pointers
        s.texcoords = (decltype(s.texcoords))d_tc.p;
        s.has_image_tex = has_image_tex ? 1 : 0;
        s.mats = (decltype(s.mats))d_mats.p;
        s.texs = (decltype(s.texs))d_texs.p;
        s.images = (decltype(s.images))d_images.p;
        s.lights = (decltype(s.lights))d_lights.p;
        s.light_cdf = (decltype(s.light_cdf))d_cdf.p;
        s.n_lights = n_lights;
        s.n_mats = n_mats;
        return s;
    }

    uint64_t n_tris() const { return matid.size(); }

    void commit_scene() {
        if (!scene_dirty) return;
        const uint64_t nt = n_tris();
        // validate references
        for (uint64_t g = 0; g < nt; g++)
            if (matid[g] >= (int32_t)mats.size()) throw std::runtime_error("material index out of range");
        for (size_t m = 0; m < mats.size(); m++) {
            const akr_material &x = mats[m];
            auto tex_ok = [&](int32_t t) { return t >= 0 && t < (int32_t)texs.size(); };
            auto mat_ok = [&](int32_t t) { return t >= 0 && t < (int32_t)mats.size(); };
            bool ok = true;
            if (x.type == AKR_MAT_DIFFUSE || x.type == AKR_MAT_EMISSIVE) ok = tex_ok(x.color);
            else if (x.type == AKR_MAT_GLOSSY) ok = tex_ok(x.color) && tex_ok(x.roughness);
            else if (x.type == AKR_MAT_MIX) ok = tex_ok(x.fraction) && mat_ok(x.first) && mat_ok(x.second);
            else if (x.type == AKR_MAT_MIRROR) ok = tex_ok(x.color);
            else if (x.type == AKR_MAT_GLASS) ok = tex_ok(x.color) && tex_ok(x.roughness);
            else ok = false;
            if (!ok) throw std::runtime_error("material " + std::to_string(m) + " has an invalid type or reference");
            if (x.type == AKR_MAT_GLASS) {  // the index of refraction: `roughness` reused
                const akr_texture &t = texs[x.roughness];
                if (t.type != AKR_TEX_CONSTANT)
                    throw std::runtime_error("material " + std::to_string(m) +
                                             ": a Glass's index of refraction must be a constant texture, not an image");
                const float ior = t.value[0];
                if (!std::isfinite(ior) || ior < 1.0f || ior > 8.0f)
                    throw std::runtime_error("material " + std::to_string(m) +
                                             ": a Glass's index of refraction must be finite and lie in [1, 8]");
            }
        }
        has_specular = false;
        for (auto &m : mats) has_specular = has_specular || m.type == AKR_MAT_MIRROR || m.type == AKR_MAT_GLASS;
        // shading the persistent path kernels run well inline: constant Diffuse / Emissive only
        simple_shading = true;
        for (auto &m : mats) simple_shading = simple_shading && (m.type == AKR_MAT_DIFFUSE || m.type == AKR_MAT_EMISSIVE);
        has_image_tex = false;
        for (auto &t : texs) {
            if (t.type == AKR_TEX_IMAGE && (t.image < 0 || t.image >= (int32_t)img_w.size()))
                throw std::runtime_error("image texture references a missing image");
            has_image_tex = has_image_tex || t.type == AKR_TEX_IMAGE;
        }
        simple_shading = simple_shading && !has_image_tex;
        // one 80-byte shading record per triangle: corners, per-face-vertex normals, material
        std::vector<ShadeTri> st(nt);
        for (uint64_t g = 0; g < nt; g++) {
            const float *v0 = &verts[3 * (size_t)idx[3 * g + 0]];
            const float *v1 = &verts[3 * (size_t)idx[3 * g + 1]];
            const float *v2 = &verts[3 * (size_t)idx[3 * g + 2]];
            const float *nn = &normals[9 * g];
            float mbits;
            std::memcpy(&mbits, &matid[g], 4);
            st[g].a = make_float4(v0[0], v0[1], v0[2], mbits);
            st[g].b = make_float4(v1[0], v1[1], v1[2], nn[0]);
            st[g].c = make_float4(v2[0], v2[1], v2[2], nn[1]);
            st[g].d = make_float4(nn[2], nn[3], nn[4], nn[5]);
            st[g].e = make_float4(nn[6], nn[7], nn[8], 0.0f);
        }
        d_shade_tri.upload(st.data(), st.size(), stream);
        if (has_image_tex) d_tc.upload(texcoords.data(), texcoords.size(), stream);
        // materials with constant textures resolved (MatDev)
        std::vector<MatDev> md(mats.size());
        for (size_t m = 0; m < mats.size(); m++) {
            const akr_material &x = mats[m];
            MatDev &d = md[m];
            std::memset(&d, 0, sizeof(d));
            akr::resolve_material(x, texs.data(), texs.size(), d);  // shade_simple.h
        }
        d_mats.upload(md.data(), md.size(), stream);
        n_mats = (int32_t)md.size();
        std::vector<TexDev> td(texs.size());
        for (size_t k = 0; k < texs.size(); k++) {
            const akr_texture &t = texs[k];
            TexDev &d = td[k];
            std::memset(&d, 0, sizeof(d));
            d.type = t.type;
            for (int c = 0; c < 3; c++) d.value[c] = t.value[c];
            if (t.type == AKR_TEX_IMAGE) {
                d.w = img_w[t.image];
                d.h = img_h[t.image];
                d.off = img_off[t.image];
            }
        }
        d_texs.upload(td.data(), td.size(), stream);
        d_images.upload(images.data(), images.size(), stream);
        d_mesh_base.upload(mesh_base.data(), mesh_base.size(), stream);
        // lights: AreaLight records + Distribution1D over `power` (common/distribution.h:46-64)
        std::vector<LightDev> ld;
        for (auto &l : lights) {
            if (l.geom_id < 0 || l.geom_id + 1 >= (int32_t)mesh_base.size())
                throw std::runtime_error("light geom_id out of range");
            uint64_t g = (uint64_t)mesh_base[l.geom_id] + (uint64_t)l.prim_id;
            if (l.prim_id < 0 || g >= mesh_base[l.geom_id + 1]) throw std::runtime_error("light prim_id out of range");
            int32_t m = matid[g];
            if (m < 0 || mats[m].type != AKR_MAT_EMISSIVE) throw std::runtime_error("light triangle is not emissive");
            LightDev x{};
            for (int k = 0; k < 3; k++) {
                const float *v = &verts[3 * (size_t)idx[3 * g + k]];
                x.v[3 * k + 0] = v[0];
                x.v[3 * k + 1] = v[1];
                x.v[3 * k + 2] = v[2];
                x.tc[2 * k + 0] = texcoords[6 * g + 2 * k + 0];
                x.tc[2 * k + 1] = texcoords[6 * g + 2 * k + 1];
            }
            akr::resolve_emission(texs.data(), texs.size(), mats[m].color, x);  // an image: color_img, Le 0
            // AreaLight::sample's triangle constants (light.h:58-71), in the device's f32 order:
            // lx = cross(v1 - v0, v2 - v0) (math.h:176-181), lng = lx / sqrt(dot(lx, lx)),
            // area_half = sqrt(dot(lx, lx)) * 0.5
            const float e1[3] = {x.v[3] - x.v[0], x.v[4] - x.v[1], x.v[5] - x.v[2]};
            const float e2[3] = {x.v[6] - x.v[0], x.v[7] - x.v[1], x.v[8] - x.v[2]};
            const float lx[3] = {(e1[1] * e2[2]) - (e1[2] * e2[1]), (e1[2] * e2[0]) - (e1[0] * e2[2]),
                                 (e1[0] * e2[1]) - (e1[1] * e2[0])};
            float dd = lx[0] * lx[0];
            dd += lx[1] * lx[1];
            dd += lx[2] * lx[2];
            const float len = std::sqrt(dd);
            for (int c = 0; c < 3; c++) x.lng[c] = lx[c] / len;
            x.area_half = len * 0.5f;
            ld.push_back(x);
        }
        n_lights = (int32_t)ld.size();
        std::vector<float> cdf(ld.size() + 1, 0.0f), func(power.begin(), power.end());
        const size_t n = ld.size();
        for (size_t i = 0; i < n; i++) cdf[i + 1] = cdf[i] + func[i] / n;
        func_int = n ? cdf[n] : 0.0f;
        if (func_int == 0) {
            for (uint32_t i = 1; i < n + 1; ++i) cdf[i] = float(i) / float(n);
        } else {
            for (uint32_t i = 1; i < n + 1; ++i) cdf[i] /= func_int;
        }
        for (size_t i = 0; i < n; i++) ld[i].sel_pdf = func[i] / (func_int * (float)n_lights);  // scene.h:85-89
        d_lights.upload(ld.data(), ld.size(), stream);
        d_cdf.upload(cdf.data(), cdf.size(), stream);
        // which shading build these tables allow: decided on the records just uploaded
        shade_simple = akr::shade_tables_simple(md.data(), md.size(), ld.data(), ld.size());
        // the selection pdf by triangle: what a BSDF-sampled ray that hits a listed triangle
        // weighs NEE's pdf of the same point with; uploaded when a session starts with option "mis"
        tri_sel.assign(matid.size(), 0.0f);
        for (size_t i = 0; i < n; i++)
            tri_sel[(size_t)mesh_base[lights[i].geom_id] + (size_t)lights[i].prim_id] += ld[i].sel_pdf;
        tri_sel_dirty = true;
        HIPCHK(hipStreamSynchronize(stream));
        scene_dirty = false;
    }

    void ensure_trace_grid() {
        if (trace_grid[0]) return;
        uint32_t mx = 0;
        for (int m = 0; m < 3; m++) {
            trace_grid[m] = (uint32_t)(n_cu * trace_blocks_per_cu(m));
            mx = std::max(mx, trace_grid[m]);
        }
        for (int d = 0; d < 3; d++)
            for (int k = 0; k < 8; k++) {  // every key without an environment; keys that share a build meet again
                const PathBuild b{d, false, (k & 4) != 0, (k & 2) != 0, (k & 1) != 0, false};
                uint32_t &g = path_grid[build_index(b)];
                if (!g) g = (uint32_t)(n_cu * path_blocks_per_cu(b));
                mx = std::max(mx, g);
            }
        ovf_threads = mx * kTraceBlock;
        d_ovf.reserve((size_t)ovf_threads * (kStackMax - kStackLds));
        d_ovf_side.reserve((size_t)ovf_threads * (kStackMax - kStackLds));
        d_work.reserve(kTraceWords);
    }

    void ensure_side_stream() {
        if (side) return;
        int least = 0, greatest = 0;  // numerically lower = higher priority
        HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIPCHK(hipStreamCreateWithPriority(&main_st, hipStreamNonBlocking, greatest));
        HIPCHK(hipStreamCreateWithPriority(&side, hipStreamNonBlocking, least));
        for (hipEvent_t *e : {&ev_fork, &ev_join, &ev_join_main, &ev_shade[0], &ev_shade[1], &ev_shadow[0], &ev_shadow[1], &ev_splat[0], &ev_splat[1]})
            HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
        HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&h_fault), sizeof(uint32_t),
                             hipHostMallocMapped | hipHostMallocCoherent));
        HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&d_fault_host), h_fault, 0));
        *reinterpret_cast<volatile uint32_t *>(h_fault) = 0;
    }

    // A raised fault word fails the call that sees it (and is cleared): the hang guard of a
    // persistent kernel stopped a wave, so that render's film is incomplete.  Called after the host
    // has waited for a render; a render_device without "verify" reports it at the next call.
    void check_fault(const char *which = "the render that raised it") {
        if (!h_fault) return;
        volatile uint32_t *f = reinterpret_cast<volatile uint32_t *>(h_fault);
        if (*f == 0) return;
        *f = 0;
        throw std::runtime_error(std::string("persistent path kernel: a wave stopped on its hang guard; the film of ") +
                                 which + " is incomplete");
    }
    // The last render_device ran without "verify" (no host wait): its fault, if any, is found by the
    // next call, which first waits for that render so the fault is not blamed on its own film.
    bool unchecked_render = false;

    uint32_t grid_for(int mode, uint64_t n) const {
        const uint64_t per_block = (uint64_t)kTraceBlock * (uint64_t)opt.rays_per_lane;
        uint64_t need = (n + per_block - 1) / per_block;
        uint64_t cap = trace_grid[mode];
        if (mode == TRACE_SHADOW) cap = std::max<uint64_t>(1, cap * (uint64_t)opt.shadow_grid_pct / 100);
        return (uint32_t)std::min<uint64_t>(need, cap);
    }

    void ensure_capacity(size_t n) {
        if (n <= cap) return;
        d_pixel.reserve(n);
        d_seed.reserve(n);
        d_slot0.reserve(n);
        d_slot1.reserve(n);
        d_ray0.reserve(2 * n);
        d_ray1.reserve(2 * n);
        d_state0.reserve(n);
        d_state1.reserve(n);
        d_hit.reserve(n);
        for (int k = 0; k < 2; k++) {
            d_sray[k].reserve(2 * n);
            d_scolor[k].reserve(n);
        }
        d_L[0].reserve(n);
        d_L[1].reserve(n);
        d_film.reserve(n);
        // the cost-ordered fetch's pilot buffers, with the rest: a first ordered
        // render then allocates nothing inside the caller's timed region
        for (int k = 0; k < 2; k++) {
            d_okey[k].reserve(n);
            d_oidx[k].reserve(n);
        }
        d_owork.reserve(kTraceWords);
        d_ocnt.reserve(3);
        d_steps_sum.reserve(1);
        d_gate.reserve(1);
        d_otmp.reserve(pixel_order_tmp_bytes((uint32_t)std::min<size_t>(n, UINT32_MAX)));
        d_pprobe.reserve(n);  // the tail pilot's and the path pilot's probe (no allocation in a render)
        cap = n;
    }

    // One trace launch: the 4-wide kernel (which traces its rare NaN-prone rays inline with the
    // exact BVH2 walk), or the BVH2 kernel when the "wide" option is off.
    void trace_launch(int mode, bool tight, const TraceArgs &t, uint64_t n_max, hipStream_t st) {
        launch_trace(mode, opt.count, tight, opt.wide, t, grid_for(mode, n_max), st);
    }

    TraceArgs trace_args(uint32_t *work) {
        TraceArgs t{};
        t.nodes = d_nodes.p;
        t.wide_nodes = reinterpret_cast<const float4 *>(d_wnodes.p);
        t.wide_leaves = reinterpret_cast<const float4 *>(d_wleaves.p);
        t.wide_root = wide_root_dev;
        // the lean slot test's slack is derived for frame origins and steps below 2^40
        t.lean = opt.lean && bvh4.max_abs <= 0x1p40f ? 1u : 0u;
        t.any_far_first = opt.any_far_first ? 1u : 0u;
        t.tris = d_tris.p;
        t.stack_ovf = d_ovf.p;
        t.ovf_threads = ovf_threads;
        t.counters = d_counters.p;
        t.work = work;
        t.mesh_base = d_mesh_base.p;
        t.n_meshes = (int32_t)mesh_base.size() - 1;
        return t;
    }

    void require_ready() {
        if (!accel_built) throw std::runtime_error("acceleration structure not built (call akr_hip_build_accel)");
        commit_scene();
        ensure_trace_grid();
        if (opt.count || opt.ray_steps) {
            if (!d_counters.p) {
                d_counters.reserve(3);
                HIPCHK(hipMemset(d_counters.p, 0, 3 * sizeof(TraceCounters)));
                d_pprof.reserve(1);
                HIPCHK(hipMemset(d_pprof.p, 0, sizeof(PathProfile)));
            }
        }
    }

    void trace(const float4 *rays, uint64_t n, akr_hit *hits, int any, hipStream_t st) {
        require_ready();
        if (n >= (1ull << 32)) throw std::runtime_error("too many rays in one batch");
        serialize(st);
        HIPCHK(hipMemsetAsync(d_work.p, 0, kTraceWords * sizeof(uint32_t), st));
        TraceArgs t = trace_args(d_work.p);
        t.rays = rays;
        t.n = (uint32_t)n;
        t.abi_hits = hits;
        int mode = any ? TRACE_ANY : TRACE_CLOSEST;
        if (opt.ray_steps) {
            d_steps.reserve(n);
            n_steps = n;
            t.ray_steps = d_steps.p;
            timed(any ? "trace_any" : "trace_closest", st,
                  [&] { launch_trace(mode, true, !opt.exact_cull, opt.wide, t, grid_for(mode, n), st); });
        } else {
            timed(any ? "trace_any" : "trace_closest", st, [&] { trace_launch(mode, !opt.exact_cull, t, n, st); });
        }
        HIPCHK(hipGetLastError());
        mark_done(st);
    }

    // Cost-ordered pixel fetch: d_oidx[1] = the slots of each XCD shard in order of
    // decreasing pilot cost (tile order within a cost class).  The pilot traces the camera ray of
    // every slot's first sample with the counting kernel into scratch counters; nothing it does
    // reaches the film, the sampler states or the context's statistics.
    void pixel_order(uint32_t N, hipStream_t ms, bool sum_steps = false) {
        // sized for the capacity by ensure_capacity (the sort's scratch grows with n), so no size
        // query runs per render
        if (d_okey[0].n < N || d_oidx[0].n < N) throw std::runtime_error("pixel order buffers not sized");
        const size_t tb = d_otmp.n;
        HIPCHK(hipMemsetAsync(d_owork.p, 0, kTraceWords * sizeof(uint32_t), ms));
        const uint32_t sub = (uint32_t)opt.path_order_sub, n_rays = (uint32_t)(((uint64_t)N + (1u << sub) - 1) >> sub);
        launch_pilot_rays(cam, d_pixel.p, n_rays, sub, d_ray0.p, ms);
        TraceArgs t = trace_args(d_owork.p);
        t.rays = d_ray0.p;
        t.n = n_rays;
        t.hits = d_hit.p;
        t.counters = d_ocnt.p;
        t.ray_steps = d_okey[1].p;
        t.step_cap = (uint32_t)opt.path_order_cap;
        // the steps-only build: no hits, no tallies (the counting build spilled and ran ~20 % longer)
        launch_trace(TRACE_PILOT, false, true, true, t, grid_for(TRACE_CLOSEST, n_rays), ms);
        if (sum_steps) HIPCHK(hipMemsetAsync(d_steps_sum.p, 0, sizeof(unsigned long long), ms));
        launch_order_keys(d_okey[1].p, N, (uint32_t)opt.path_order_shift, (uint32_t)(opt.path_order_classes - 1), sub,
                          d_okey[0].p, d_oidx[0].p, ms, sum_steps ? d_steps_sum.p : nullptr);
        sort_pixel_order(d_otmp.p, tb, d_okey[0].p, d_okey[1].p, d_oidx[0].p, d_oidx[1].p, N, ms);
        HIPCHK(hipGetLastError());
    }

    // A counting k_path render of S samples per slot (the render's own first samples: a slot's sampler
    // starts from its seed in every render) into the zeroed film, whose pixel probe d_pprobe then holds
    // each slot's closest-hit and shadow rays; the film is zeroed again for the render.  Nothing of it
    // reaches the context's statistics (scratch counters, no phase profile).
    // With an environment (option env_path) the counting environment kernel runs, so the ray counts are those of
    // the render the pilot ranks.
    void probe_render(const PathArgs &base, bool tab, uint32_t N, int S, hipStream_t ms) {
        if (d_pprobe.n < N) throw std::runtime_error("pilot probe buffer not sized");
        HIPCHK(hipMemsetAsync(d_owork.p, 0, kTraceWords * sizeof(uint32_t), ms));
        PathArgs pp = base;
        pp.spp = (uint32_t)S;
        pp.work = d_owork.p;
        pp.t.counters = d_ocnt.p;
        pp.prof = nullptr;
        pp.probe = d_pprobe.p;
        pp.probe_clock = 0;
        pp.order = nullptr;
        pp.fault_test = 0;
        pp.state_in = pp.state_out = nullptr;
        const bool envp = env_on();
        const uint32_t grid = (uint32_t)std::max<uint64_t>(
            1, std::min<uint64_t>(grid_of(PathBuild{PATH_PLAIN, false, tab, true, true, envp}),
                                  ((uint64_t)N + kTraceBlock - 1) / kTraceBlock));
        // counting: the general shading
        launch_path(PathBuild{PATH_PLAIN, true, tab, leaf_one_kernel, false, envp}, pp, envp ? env_rec(ms) : nullptr, grid, ms);
        HIPCHK(hipMemsetAsync(d_film.p, 0, (size_t)N * sizeof(float4), ms));
    }

    // The last render's form and pilot step sum, when they were left on the device (a gated launch):
    // waits for that render, then reads the gate word and the sum
    void resolve_form() {
        if (!form_pending && !pilot_sum_pending) return;
        if (done_recorded) HIPCHK(hipStreamWaitEvent(stream, ev_done, 0));
        unsigned long long sum = 0;
        uint32_t gate = 0;
        HIPCHK(hipMemcpyAsync(&sum, d_steps_sum.p, sizeof(sum), hipMemcpyDeviceToHost, stream));
        if (form_pending) HIPCHK(hipMemcpyAsync(&gate, d_gate.p, sizeof(gate), hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        last_pilot_steps = (int64_t)sum;
        if (form_pending) {
            if (gate > 1) throw std::runtime_error("render form gate holds " + std::to_string(gate));
            last_form = gate_forms[gate];
        }
        form_pending = pilot_sum_pending = false;
    }

    // Path pilot (option path_order_pilot_spp): slots ranked by the rays their first S samples take
    // (probe_render), in classes of 2^shift rays.
    void pixel_order_path(const PathArgs &base, bool tab, uint32_t N, int S, hipStream_t ms) {
        if (d_okey[0].n < N || d_oidx[0].n < N) throw std::runtime_error("pixel order buffers not sized");
        // S samples trace at most S * (2 max_depth + 1) rays (max(1, max_depth) closest-hit, max_depth shadow)
        const uint32_t max_rays = (uint32_t)S * (2u * (uint32_t)std::max(base.max_depth, 0) + 1u);
        probe_render(base, tab, N, S, ms);
        launch_probe_cost(d_pprobe.p, N, d_okey[1].p, ms);
        uint32_t shift = 0;
        while (((max_rays + 1u) >> shift) > (uint32_t)opt.path_order_classes) shift++;
        launch_order_keys(d_okey[1].p, N, shift, (uint32_t)(opt.path_order_classes - 1), 0, d_okey[0].p, d_oidx[0].p, ms);
        sort_pixel_order(d_otmp.p, d_otmp.n, d_okey[0].p, d_okey[1].p, d_oidx[0].p, d_oidx[1].p, N, ms);
        HIPCHK(hipGetLastError());
    }

    // Pixels of the tile list (tiles in order, row-major inside a tile) into d_pixel, expanded on
    // the device from the clipped tiles (the host loop over every pixel and the pageable upload of
    // its list cost 1.7 ms per 1080p render); sizes the queues and the per-pass counter sets.
    // Returns the pixel count.
    uint64_t setup_pixels(const akr_rect *tiles, int32_t n_tiles, size_t n_count_words, hipStream_t st) {
        require_ready();
        if (!cam_set) throw std::runtime_error("camera not set (call akr_hip_set_camera)");
        if (n_tiles < 0 || (n_tiles > 0 && !tiles)) throw std::runtime_error("invalid tile list");
        drop_session();
        h_pixel_ok = false;
        lay = layout_tiles(tiles, n_tiles, cam.width, cam.height, "render call");
        const uint64_t N = lay.n;
        serialize(st);
        ensure_capacity(N);  // before any upload: a reallocation drops contents
        d_counts.reserve(2 * n_count_words);  // two pass parities
        if (N == 0) return 0;
        ensure_side_stream();
        expand_layout(lay, d_tiles, d_pixel.p, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemsetAsync(d_film.p, 0, N * sizeof(float4), st));
        fork_streams(st);
        return N;
    }

    void fork_streams(hipStream_t st) {
        HIPCHK(hipEventRecord(ev_fork, st));  // both internal streams start after the caller's work
        HIPCHK(hipStreamWaitEvent(main_st, ev_fork, 0));
        HIPCHK(hipStreamWaitEvent(side, ev_fork, 0));
    }

    // setup_pixels for a continued render: the session's pixel list, film and sampler states stay as
    // they are (nothing is expanded, zeroed or reallocated); only the counters are sized and the
    // internal streams forked.  Returns the session's pixel count.
    uint64_t resume_pixels(size_t n_count_words, hipStream_t st) {
        const uint64_t N = require_session().n;
        require_ready();
        if (N != lay.n || N > cap) throw std::runtime_error("render session: the slot buffers changed");
        serialize(st);
        d_counts.reserve(2 * n_count_words);  // two pass parities
        if (N == 0) return 0;
        ensure_side_stream();
        fork_streams(st);
        return N;
    }

    // The last render's pixel list on the host (slot order), for the host-side film merges
    const std::vector<uint32_t> &host_pixels() {
        if (!h_pixel_ok) slot_pixels(lay, h_pixel);
        h_pixel_ok = true;
        return h_pixel;
    }

    // order `st` after the context's previous trace / render ("one context, one
    // order"), and record the end of this one
    void serialize(hipStream_t st) {
        if (done_recorded) HIPCHK(hipStreamWaitEvent(st, ev_done, 0));
    }
    void mark_done(hipStream_t st) {
        HIPCHK(hipEventRecord(ev_done, st));
        done_recorded = true;
    }

    // In-band check (option "verify"): every one of the N film slots holds exactly `spp` samples.
    // Runs on `st` after the render has been joined into it and waits for it on the host, so a
    // render_device with the check on returns only after the film is complete.
    // per_slot: the film of a session whose slots hold different counts: every weight against d_count
    void verify_weights(hipStream_t st, uint64_t N, int spp, bool per_slot = false) {
        if (!opt.verify || N == 0) return;
        if (per_slot && d_count.n < N) throw std::runtime_error("film check: the per-slot counts are missing");
        if (!h_check) {
            HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&h_check), sizeof(uint32_t),
                                 hipHostMallocMapped | hipHostMallocCoherent));
            HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&d_check_host), h_check, 0));
        }
        d_bad.reserve(1);
        *reinterpret_cast<volatile uint32_t *>(h_check) = kMappedSentinel;
        HIPCHK(hipMemsetAsync(d_bad.p, 0, sizeof(uint32_t), st));
        if (per_slot) launch_check_counts(d_film.p, d_count.p, (uint32_t)N, d_bad.p, st);
        else launch_check_weights(d_film.p, (uint32_t)N, (float)spp, d_bad.p, st);
        launch_store_word(d_bad.p, d_check_host, st);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
        check_fault();
        const uint32_t bad = read_mapped(h_check);
        if (bad == kMappedSentinel) throw std::runtime_error("film check: the device never reported its result");
        if (bad != 0)
            throw std::runtime_error("film check: " + std::to_string(bad) + " of " + std::to_string(N) +
                                     " pixels do not hold " +
                                     (per_slot ? std::string("their expected") : std::to_string(spp)) + " samples");
    }

    // ---- subset passes
    // The ascending list of the slots whose mask byte is non-zero into d_active: per-wave ballot counts,
    // their exclusive scan, the scatter.  Returns the list's length (the one host wait of a pass: 4 bytes).
    uint32_t compact_mask(const uint8_t *mask, uint32_t N, hipStream_t st) {
        if (N == 0) return 0;
        const uint32_t n_waves = (N + 63u) / 64u;
        d_active.reserve(N);
        d_wcount.reserve(n_waves);
        d_woff.reserve(n_waves);
        d_nactive.reserve(1);
        if (d_scan_tmp.n < scan_tmp_bytes(n_waves)) d_scan_tmp.reserve(scan_tmp_bytes(n_waves));
        timed("compact", st, [&] {
            launch_mask_count(mask, N, d_wcount.p, st);
            scan_exclusive_u32(d_scan_tmp.p, d_scan_tmp.n, d_wcount.p, d_woff.p, n_waves, st);
            launch_mask_compact(mask, N, d_woff.p, d_active.p, d_nactive.p, st);
        });
        HIPCHK(hipGetLastError());
        uint32_t m = 0;
        HIPCHK(hipMemcpyAsync(&m, d_nactive.p, sizeof(m), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (m > N) throw std::runtime_error("slot mask compaction: " + std::to_string(m) + " active of " + std::to_string(N));
        return m;
    }

    // smallest and largest expected count of the slots in d_active[0..m) (list) or of all N slots
    void count_range(bool list, uint32_t n, hipStream_t st, uint32_t &lo, uint32_t &hi) {
        d_crange.reserve(2);
        const uint32_t init[2] = {0xFFFFFFFFu, 0u};
        HIPCHK(hipMemcpyAsync(d_crange.p, init, sizeof(init), hipMemcpyHostToDevice, st));
        launch_count_range(d_count.p, list ? d_active.p : nullptr, n, d_crange.p, st);
        uint32_t out[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(out, d_crange.p, sizeof(out), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        lo = out[0];
        hi = out[1];
    }

    // spp more samples for the m slots listed in d_active (ascending), on `st`; updates the session's
    // counts.  m == N keeps a uniform session uniform.  `range`: recompute spp_min / spp_done of a
    // non-uniform session from the counts (the adaptive loop knows them and passes false).
    void render_subset(int32_t spp, uint32_t m, hipStream_t st, bool range = true) {
        Session &s = session;
        const uint64_t N = require_session().n;
        if (m == 0 || spp == 0) return;
        if (m > N) throw std::runtime_error("render session: more active slots than slots");
        uint32_t lo, hi;
        if (cap_needs_largest(s, spp)) {  // near the cap only: the largest count among the listed slots
            count_range(true, m, st, lo, hi);
            check_cap(hi, spp);
        }
        const akr_pt_params p = session_params(s, spp);
        if (!s.seeded) {  // no sample drawn yet: the slots left out keep their start state x + y * width
            launch_init_seed(d_pixel.p, (uint32_t)N, cam.width, d_seed.p, st);
            s.seeded = true;
        }
        if (m == N) {
            render(p, nullptr, 0, st, true);
        } else {
            if (s.uniform) {
                d_count.reserve(N);
                launch_fill_u32(d_count.p, (uint32_t)N, (uint32_t)s.spp_done, st);
            }
            render(p, nullptr, 0, st, true, d_active.p, m);
        }
        const SlotCounts counts = advance_subset(s, m, spp);
        if (counts == SlotCounts::None) return;
        launch_count_add(d_count.p, m == N ? nullptr : d_active.p, m, (uint32_t)spp, st);
        HIPCHK(hipGetLastError());
        if (counts == SlotCounts::AddAndRead && range) {
            count_range(false, (uint32_t)N, st, lo, hi);
            set_range(s, lo, hi);
        }
    }
    // host waits for both internal streams (before a DMA read-back of the film)
    void host_join() {
        if (side) HIPCHK(hipStreamSynchronize(side));
        if (main_st) HIPCHK(hipStreamSynchronize(main_st));
    }

    // the caller's stream sees every pass of both internal streams complete
    void join_streams(hipStream_t st) {
        // one event per internal stream: re-recording a single event before the caller's stream
        // has consumed the first wait must never be able to drop the side stream from the join
        HIPCHK(hipEventRecord(ev_join, side));
        HIPCHK(hipEventRecord(ev_join_main, main_st));
        HIPCHK(hipStreamWaitEvent(st, ev_join, 0));
        HIPCHK(hipStreamWaitEvent(st, ev_join_main, 0));
        HIPCHK(hipGetLastError());
    }

    RaygenArgs raygen_args(uint32_t N, float4 *L, uint32_t *count, bool first) const {
        RaygenArgs rg{};
        rg.cam = cam;
        rg.pixel = d_pixel.p;
        rg.n = N;
        rg.seed = d_seed.p;
        rg.L = L;
        rg.ray_out = d_ray0.p;
        rg.state_out = d_state0.p;
        rg.slot_out = d_slot0.p;
        rg.count_out = count;
        rg.first_pass = first;
        return rg;
    }

    // what render()'s prologue hands to render_path() / render_wavefront()
    struct Pass {
        akr_pt_params p;
        uint64_t N, M;           // the session's slots, and the slots this pass fetches
        const uint32_t *subset;  // the list of those (a masked continue), or nullptr: every slot
        bool cont, resume;       // resume: the slots' sampler states are the ones the last segment left
        bool tight;
        uint4 *probe;            // option "pixel_probe"
        size_t n_count_words;    // one pass's counter set
    };

    // cont: p.spp more samples for every slot of the session: the slots, their film sums
    // and (when the session is seeded) their sampler states are the ones the last segment left
    // subset (with cont): the pass draws its samples for the n_subset slots listed there only (a masked
    // continue): the same launches over a shorter fetch list, unranked
    uint64_t render(const akr_pt_params &p, const akr_rect *tiles, int32_t n_tiles, hipStream_t st, bool cont = false,
                    const uint32_t *subset = nullptr, uint64_t n_subset = 0) {
        if (p.spp < 0 || p.max_depth < 0) throw std::runtime_error("spp and max_depth must be >= 0");
        if (p.max_depth > 1000) throw std::runtime_error("max_depth too large");
        // counters per pass, each on its own 128-B line (atomics on one line serialise):
        // D ray-queue counts, D shadow-queue counts, 2 trace launches x kTraceWords per bounce;
        // two sets, alternating by pass, since consecutive passes overlap
        const int D = p.max_depth + 2;
        const size_t n_count_words = 2 * (size_t)D * kWorkStride + 2 * (size_t)D * kTraceWords;
        last_passes = 0;
        last_form = AKR_FORM_NONE;
        last_ordered = 0;
        last_shading = AKR_SHADING_NONE;
        form_pending = pilot_sum_pending = false;
        probe_ok = false;
        probe_n = 0;
        const bool resume = cont && require_session().seeded;  // else every slot starts from x + y * width
        const uint64_t N = cont ? resume_pixels(n_count_words, st) : setup_pixels(tiles, n_tiles, n_count_words, st);
        if (!cont) variance_begin(N, st);  // zeroed on st beside the render; the update follows the join below
        if (!cont) mis_begin(N, st);       // a continue keeps the session's value
        spec_begin(N);                     // the committed scene's, at every call
        if (N == 0) return 0;
        if (subset && (!cont || n_subset == 0 || n_subset > N)) throw std::runtime_error("render: invalid slot subset");
        const uint64_t M = subset ? n_subset : N;  // the slots this pass fetches
        if (unchecked_render) {  // a fault raised by an earlier render_device that ran without "verify"
            unchecked_render = false;
            if (done_recorded) HIPCHK(hipEventSynchronize(ev_done));
            check_fault("the previous render_device call (run without verify; reported by the next render)");
        }
        uint4 *probe_p = nullptr;  // option "pixel_probe"
        if (opt.probe()) {
            d_probe.reserve(N);
            HIPCHK(hipMemsetAsync(d_probe.p, 0, N * sizeof(uint4), main_st));
            probe_p = d_probe.p;
            probe_n = N;
            probe_ok = true;
        }
        const bool tight = !(opt.exact_cull || (p.flags & AKR_PT_EXACT_CULL));
        const Pass pass{p, N, M, subset, cont, resume, tight, probe_p, n_count_words};
        // Persistent path kernel: every sample of every pixel in one launch.  It
        // runs the lean wide traversal only; the reference cull, the BVH2 kernel and a wide view whose
        // frames exceed the lean test's bounds keep the wavefront form.
        // auto: the persistent kernel for scenes whose shading is constant Diffuse / Emissive; Glossy,
        // Mix or image textures diverge inside the traversal waves, and the wavefront's separate shade
        // kernel measured faster there (textured hall 11.5 vs 16.0 ms per 4K spp)
        const bool use_path = opt.path_kernel == 1 || (opt.path_kernel == 2 && (int64_t)M <= opt.path_auto_pixels &&
                                                       (simple_shading || opt.path_auto_complex));
        // an environment light is shaded by the wavefront's k_shade_env, whatever `path`
        // says: the precedent exact_cull and a non-lean view set; under option env_path it no longer decides,
        // and render_path() runs k_path's environment build
        // and so does option "mis": its kernels are the wavefront's
        const bool env_wavefront = env_on() && !opt.env_path;
        // and so does a scene that holds a Mirror or a Glass: k_shade_spec and its forms
        // and so does an active thin lens: k_raygen_lens is the wavefront's
        if (use_path && tight && opt.wide && trace_args(nullptr).lean && !env_wavefront && !mis_on && !spec_on &&
            !lens_active()) {
            if (p.spp > 0) render_path(pass);
            last_passes = 1;
        } else {
            render_wavefront(pass);
        }
        join_streams(st);
        if (p.spp > 0) variance_update(N, st);
        return N;
    }

    // the first ordered render of a context runs the pilot once on a few pixels: its kernels (and
    // rocPRIM's) are loaded then, not inside a later ordered render
    void warm_order(uint64_t N, hipStream_t ms) {
        if (order_warm) return;
        pixel_order((uint32_t)std::min<uint64_t>(N, 64), ms);
        order_warm = true;
    }

    // The persistent half of render(): the pilot plan_path() (path_plan.h) asks for, then
    // the one or two launches it lists
    void render_path(const Pass &r) {
        const akr_pt_params &p = r.p;
        const uint64_t N = r.N;
        hipStream_t ms = main_st;
        HIPCHK(hipMemsetAsync(d_counts.p, 0, kWorkWords * sizeof(uint32_t), ms));
        PathArgs pa{};
        pa.t = trace_args(nullptr);
        pa.sc = scene_dev();
        pa.cam = cam;
        pa.pixel = d_pixel.p;
        pa.film = d_film.p;
        pa.work = d_counts.p;
        pa.n_pix = (uint32_t)r.M;
        pa.spp = (uint32_t)p.spp;
        pa.max_depth = p.max_depth;
        pa.ray_clamp = p.ray_clamp;
        pa.prof = opt.count ? d_pprof.p : nullptr;
        if (opt.count && opt.count_lines) {
            auto span = [](const void *p, size_t bytes) {
                const uint64_t a = (uint64_t)p;
                return (uint32_t)(bytes ? ((a + bytes - 1) >> 7) - (a >> 7) + 1 : 0);
            };
            lines_span[0] = 0;
            lines_span[1] = span(d_wnodes.p, d_wnodes.n * sizeof(akr_bvh4_node));
            lines_span[2] = lines_span[1] + span(d_wleaves.p, d_wleaves.n * sizeof(float4));
            lines_span[3] = lines_span[2] + span(d_shade_tri.p, d_shade_tri.n * sizeof(ShadeTri));
            d_lines.reserve(lines_span[3] / 32 + 1);
            HIPCHK(hipMemsetAsync(d_lines.p, 0, (lines_span[3] / 32 + 1) * sizeof(uint32_t), ms));
            pa.lines = d_lines.p;
            for (int k = 0; k < 4; k++) pa.lines_span[k] = lines_span[k];
        }
        pa.probe = r.probe;
        pa.fault = d_fault_host;
        pa.fault_test = opt.fault_test ? 1u : 0u;
        pa.probe_clock = opt.probe_clock() ? 1u : 0u;
        pa.spec_depth = (uint32_t)opt.path_spec_depth;
        pa.state_in = r.resume ? d_seed.p : nullptr;  // in place: a slot is fetched by one lane per launch
        pa.state_out = d_seed.p;
        pa.min_wait = (uint32_t)(opt.path_min_wait > 0 ? opt.path_min_wait : 40);
        pa.pop_keep = (uint32_t)opt.path_pop_keep;
        pa.pop_rounds = (uint32_t)opt.path_pop_rounds;
        // the shading's material / light / CDF tables in LDS when they fit
        const bool tab = opt.path_tab && path_tab_fits(n_mats, n_lights);
        // the shading build: the simple one where the committed tables allow it; the
        // counting builds run the general one on every scene
        const bool simple = shade_simple && !opt.count;
        PathPlanIn in;
        in.N = N;
        in.M = r.M;
        in.spp = p.spp;
        in.max_depth = p.max_depth;
        in.cont = r.cont;
        in.subset = r.subset != nullptr;
        in.n_tris = n_tris();
        in.bvh_dev_bytes = bvh_dev_bytes;
        // an environment (option env_path): k_path's build for it alone, unless option
        // env_forms lets the rule decide as it does without one; each kind's environment kernel then carries
        // the plan out
        const bool envp = env_on();
        in.plain_only = env_plain_only(envp, opt);
        // plain_only: the rule plans no kind but PATH_PLAIN, whose build stands in for every kind's
        auto build = [&](int kind) {
            return PathBuild{in.plain_only ? PATH_PLAIN : kind, opt.count, tab, leaf_one_kernel, simple, envp};
        };
        for (int k = 0; k < 3; k++) in.grid[k] = grid_of(build(k));
        in.block = kTraceBlock;
        const PathPlan pl = plan_path(in, opt);
        last_ppl1000 = pl.ppl1000;
        last_pilot_rays = pl.pilot_rays;
        last_pilot_steps = -1;
        if (opt.path_order != 0) warm_order(N, ms);
        if (pl.pilot) {
            if (pl.path_pilot)
                timed("pilot", ms, [&] { pixel_order_path(pa, tab, (uint32_t)N, opt.path_order_pilot_spp, ms); });
            else
                timed("pilot", ms, [&] { pixel_order((uint32_t)N, ms, pl.want_steps); });
        }
        // The rule's tail test reads the pilot's step sum, which is on the device: no host wait
        // inside the render.  k_pick_form writes a gate word from the sum, and both
        // candidate kernels are launched back to back, each exiting at once unless the gate
        // names it; the form that ran is read back only when akr_hip_render_form asks.
        if (pl.gated)
            launch_pick_form(d_steps_sum.p, (unsigned long long)opt.path_tail_steps * (uint64_t)pl.pilot_rays, d_gate.p, ms);
        PathArgs args[2] = {pa, pa};
        for (int k = 0; k < pl.n_launch; k++) {
            const PathLaunch &l = pl.launch[k];
            PathArgs &x = args[k];
            if (l.contrib_lanes) {
                d_contrib.reserve((size_t)18 * l.contrib_lanes);  // 16 NEE slots + the waiting ray
                x.contrib = d_contrib.p;
            }
            x.mix = l.mix;
            x.order = l.list == LIST_PILOT ? d_oidx[1].p : (l.list == LIST_SUBSET ? r.subset : nullptr);
            x.order_mode = l.order_mode;
            x.prio = l.prio;
            if (pl.gated) {
                x.gate = d_gate.p;
                x.gate_want = (uint32_t)k;
            }
        }
        const AKR_GLOBAL EnvDev *erec = envp ? env_rec(ms) : nullptr;  // copied before the timed launch, once per upload
        timed("path", ms, [&] {  // one timed record: a gated launch that exits at once adds microseconds
            for (int k = 0; k < pl.n_launch; k++) launch_path(build(pl.launch[k].kind), args[k], erec, pl.launch[k].grid, ms);
        });
        HIPCHK(hipGetLastError());
        last_shading = simple ? AKR_SHADING_SIMPLE : AKR_SHADING_GENERAL;
        form_pending = pl.gated;
        pilot_sum_pending = pl.want_steps && !pl.gated;  // the step sum is read back on request
        if (pl.gated) std::copy(pl.gate_forms, pl.gate_forms + 2, gate_forms);
        last_form = pl.last_form;
        last_ordered = pl.last_ordered;
        // a subset pass wrote the probe of its slots only: the others keep the state they had
        if (r.subset && r.probe)
            launch_probe_fill(d_seed.p, (uint32_t)N, r.probe, AKR_PROBE_SEED | (opt.count ? AKR_PROBE_RAYS : 0u), ms);
    }

    // The wavefront half of render(): raygen -> {closest-hit -> shade -> shadow}^depth -> splat per sample pass
    void render_wavefront(const Pass &r) {
        const akr_pt_params &p = r.p;
        const uint64_t N = r.N, M = r.M;
        const uint32_t *subset = r.subset;
        const bool resume = r.resume, tight = r.tight;
        uint4 *probe_p = r.probe;
        const size_t n_count_words = r.n_count_words;
        const int D = p.max_depth + 2;
        hipStream_t ms = main_st;
        const SceneDev sd = scene_dev();
        if (p.spp > 0) last_form = AKR_FORM_WAVEFRONT;
        if (p.spp > 0) last_shading = AKR_SHADING_GENERAL;
        const int nb_plain = p.max_depth == 0 ? 1 : p.max_depth;  // the trace at depth == max_depth can
                                                                   // add nothing: skipped
        // with a Mirror or a Glass it can: a ray that left a delta lobe at the last scattering vertex may still
        // meet an emitter or the sky.  Only such rays are queued for it (shade_hit_tab, SPEC), DESIGN.md §3.19
        const int nb = spec_on && p.max_depth > 0 ? p.max_depth + 1 : nb_plain;
        const bool with_E = mis_on || spec_on;  // the terminal accumulator and k_splat_mis
        int64_t g = 0;  // bounce index over all passes: shadow queues alternate by its parity
        const uint32_t *worder = nullptr;  // the cost order of the camera rays (option wave_order)
        if (opt.wave_order && opt.path_order != 0 && !subset && p.spp >= order_min_spp(opt, N) && N >= 2) {
            warm_order(N, ms);
            timed("pilot", ms, [&] { pixel_order((uint32_t)N, ms); });
            worder = d_oidx[1].p;
        }
        last_ordered = worder ? 1 : 0;
        for (int s = 0; s < p.spp; s++) {
            const int ps = s & 1;
            last_passes++;
            uint32_t *cnt = d_counts.p + (size_t)ps * n_count_words;
            auto qcount = [&](int b) { return cnt + (size_t)b * kWorkStride; };
            auto scount = [&](int b) { return cnt + (size_t)(D + b) * kWorkStride; };
            auto work = [&](int b, int k) { return cnt + 2 * (size_t)D * kWorkStride + (size_t)(2 * b + k) * kTraceWords; };
            float4 *L = d_L[ps].p;
            // L[ps] and the counter set were last used by pass s - 2, whose splat ends its side-stream work
            if (s >= 2) HIPCHK(hipStreamWaitEvent(ms, ev_splat[ps], 0));
            HIPCHK(hipMemsetAsync(cnt, 0, n_count_words * sizeof(uint32_t), ms));
            if (with_E) HIPCHK(hipMemsetAsync(d_E[ps].p, 0, N * sizeof(float4), ms));  // like L[ps]: free since pass s - 2
            RaygenArgs rg = raygen_args((uint32_t)M, L, qcount(0), s == 0 && !resume);
            rg.probe = probe_p;
            rg.order = subset ? subset : worder;
            timed("raygen", ms, [&] { raygen_launch(rg, ms); });
            for (int b = 0; b < nb; b++, g++) {
                const bool odd = b & 1;
                const int sq = (int)(g & 1);
                TraceArgs t = trace_args(work(b, 0));
                t.rays = odd ? d_ray1.p : d_ray0.p;
                t.count = qcount(b);
                t.hits = d_hit.p;
                timed("trace_closest", ms, [&] { trace_launch(TRACE_CLOSEST, tight, t, M, ms); });
                // shade refills shadow queue g % 2: the shadow trace of bounce g - 2 must be done
                if (g >= 2) HIPCHK(hipStreamWaitEvent(ms, ev_shadow[sq], 0));
                ShadeArgs sh{};
                sh.sc = sd;
                sh.ray_in = odd ? d_ray1.p : d_ray0.p;
                sh.state_in = odd ? d_state1.p : d_state0.p;
                sh.slot_in = odd ? d_slot1.p : d_slot0.p;
                sh.hit_in = d_hit.p;
                sh.count_in = qcount(b);
                sh.ray_out = odd ? d_ray0.p : d_ray1.p;
                sh.state_out = odd ? d_state0.p : d_state1.p;
                sh.slot_out = odd ? d_slot0.p : d_slot1.p;
                sh.count_out = qcount(b + 1);
                sh.shadow_ray = d_sray[sq].p;
                sh.shadow_color = d_scolor[sq].p;
                sh.shadow_count = scount(b);
                sh.seed = d_seed.p;
                sh.L = L;  // written at depth 0 only, before any shadow trace of the pass
                sh.depth = b;
                sh.max_depth = p.max_depth;
                sh.last = b >= nb_plain - 1;
                sh.probe = probe_p;
                // MIS: the terminal term goes to E[ps], never to L, which the side stream's shadow trace of the
                // bounce before may be adding to; one queue entry per slot per launch, so E needs no atomic
                MisDev md{};
                md.carry_in = odd ? d_carry[1].p : d_carry[0].p;
                md.carry_out = odd ? d_carry[0].p : d_carry[1].p;
                md.tri_sel = (decltype(md.tri_sel))d_tri_sel.p;  // device code sees it as a global pointer
                md.E = d_E[ps].p;
                // a Mirror or a Glass in the scene: the specular forms; the via_delta bit rides in md's carried
                // record under MIS and in a flag queue of its own otherwise
                SpecDev sv{};
                sv.flag_in = odd ? d_spec_flag[1].p : d_spec_flag[0].p;
                sv.flag_out = odd ? d_spec_flag[0].p : d_spec_flag[1].p;
                sv.E = d_E[ps].p;
                timed("shade", ms, [&] { launch_shade(ShadeBuild{env_on(), mis_on, spec_on}, sh, &env, &md, &sv, (uint32_t)M, ms); });
                HIPCHK(hipEventRecord(ev_shade[sq], ms));
                HIPCHK(hipStreamWaitEvent(side, ev_shade[sq], 0));
                if (b < p.max_depth) {
                    TraceArgs ts = trace_args(work(b, 1));
                    ts.stack_ovf = d_ovf_side.p;  // concurrent with a main-stream trace
                    ts.rays = d_sray[sq].p;
                    ts.count = scount(b);
                    ts.shadow_color = d_scolor[sq].p;
                    ts.L = L;
                    // option serial_shadow (measurement): on the main stream, so the launch is timed alone
                    hipStream_t sst = opt.serial_shadow ? ms : side;
                    timed("trace_shadow", sst, [&] { trace_launch(TRACE_SHADOW, tight, ts, M, sst); });
                }
                if (opt.serial_shadow) {
                    HIPCHK(hipEventRecord(ev_shadow[sq], ms));
                    HIPCHK(hipStreamWaitEvent(side, ev_shadow[sq], 0));
                } else {
                    HIPCHK(hipEventRecord(ev_shadow[sq], side));
                }
            }
            // Tile::add_sample on the side stream, after the pass's last shadow trace: the next
            // pass (its own L and counters) proceeds on the main stream meanwhile
            SplatArgs sp{};
            sp.L = L;
            sp.film = d_film.p;
            sp.n = (uint32_t)M;
            sp.ray_clamp = p.ray_clamp;
            sp.order = subset;
            if (with_E) timed("splat", side, [&] { launch_splat_mis(SplatMisArgs{sp, d_E[ps].p}, (uint32_t)M, side); });
            else timed("splat", side, [&] { launch_splat(sp, (uint32_t)M, side); });
            HIPCHK(hipEventRecord(ev_splat[ps], side));
        }
        // the last shade of every pass ran on the main stream and left each slot's sampler state
        if (probe_p && p.spp > 0) launch_probe_seed(d_seed.p, (uint32_t)N, probe_p, ms);
    }

    // cpu::AmbientOcclusion::render (kernel/integrators/cpu/integrator.cpp:40-87) as one wavefront
    // pass per sample: raygen -> closest-hit trace -> k_ao_shade on the main stream, then the AO
    // rays and splat on the side stream (overlapping the next pass, as in render()).  occlude = +inf
    // makes "closest hit with t < occlude" plain occlusion (any hit in (Eps, inf)): a shadow-mode
    // trace adds 1 to L when unoccluded.  Any other occlude traces the AO rays closest-hit and
    // compares t (an any-hit trace bounded by tmax = occlude could differ from the reference by
    // float rounding in the box tests near t = occlude).
    uint64_t render_ao(const akr_ao_params &p, const akr_rect *tiles, int32_t n_tiles, hipStream_t st) {
        if (p.spp < 0) throw std::runtime_error("spp must be >= 0");
        // per pass: camera-queue count, AO-queue count, then 2 trace launches x kTraceWords
        const size_t n_count_words = 2 * (size_t)kWorkStride + 2 * (size_t)kTraceWords;
        probe_ok = false;
        probe_n = 0;
        const uint64_t N = setup_pixels(tiles, n_tiles, n_count_words, st);
        if (N == 0) return 0;
        const bool shadow_mode = std::isinf(p.occlude) && p.occlude > 0;
        if (!shadow_mode)
            for (int k = 0; k < 2; k++) d_ao_slot[k].reserve(N);
        hipStream_t ms = main_st;
        const bool tight = !(opt.exact_cull || (p.flags & AKR_PT_EXACT_CULL));
        for (int s = 0; s < p.spp; s++) {
            const int ps = s & 1;
            uint32_t *cnt = d_counts.p + (size_t)ps * n_count_words;
            uint32_t *qcount = cnt, *acount = cnt + kWorkStride;
            uint32_t *work0 = cnt + 2 * kWorkStride, *work1 = work0 + kTraceWords;
            float4 *L = d_L[ps].p;
            // L[ps], the AO queue ps and the counter set were last used by pass s - 2 (ends with its splat)
            if (s >= 2) HIPCHK(hipStreamWaitEvent(ms, ev_splat[ps], 0));
            HIPCHK(hipMemsetAsync(cnt, 0, n_count_words * sizeof(uint32_t), ms));
            const RaygenArgs rg = raygen_args((uint32_t)N, L, qcount, s == 0);
            timed("raygen", ms, [&] { raygen_launch(rg, ms); });
            TraceArgs t = trace_args(work0);
            t.rays = d_ray0.p;
            t.count = qcount;
            t.hits = d_hit.p;
            timed("trace_closest", ms, [&] { trace_launch(TRACE_CLOSEST, tight, t, N, ms); });
            AoShadeArgs sh{};
            sh.tri = d_shade_tri.p;
            sh.hit_in = d_hit.p;
            sh.slot_in = d_slot0.p;
            sh.state_in = d_state0.p;
            sh.count_in = qcount;
            sh.seed = d_seed.p;
            sh.ray_out = d_sray[ps].p;
            sh.color_out = shadow_mode ? d_scolor[ps].p : nullptr;
            sh.slot_out = shadow_mode ? nullptr : d_ao_slot[ps].p;
            sh.count_out = acount;
            timed("ao_shade", ms, [&] { launch_ao_shade(sh, (uint32_t)N, ms); });
            HIPCHK(hipEventRecord(ev_shade[ps], ms));
            HIPCHK(hipStreamWaitEvent(side, ev_shade[ps], 0));
            TraceArgs ts = trace_args(work1);
            ts.stack_ovf = d_ovf_side.p;  // concurrent with the next pass's main-stream trace
            ts.rays = d_sray[ps].p;
            ts.count = acount;
            if (shadow_mode) {
                ts.shadow_color = d_scolor[ps].p;
                ts.L = L;
                timed("trace_shadow", side, [&] { trace_launch(TRACE_SHADOW, tight, ts, N, side); });
            } else {
                ts.hits = d_scolor[ps].p;  // the colour queue is free in this mode: AO hits
                timed("trace_ao_closest", side, [&] { trace_launch(TRACE_CLOSEST, tight, ts, N, side); });
                AoResolveArgs rs{d_scolor[ps].p, d_ao_slot[ps].p, acount, L, p.occlude};
                timed("ao_resolve", side, [&] { launch_ao_resolve(rs, (uint32_t)N, side); });
            }
            SplatArgs sp{};
            sp.L = L;
            sp.film = d_film.p;
            sp.n = (uint32_t)N;
            sp.ray_clamp = 0.0f;  // Tile::add_sample(p, L, 1) unclamped (integrator.cpp:78)
            timed("splat", side, [&] { launch_splat(sp, (uint32_t)N, side); });
            HIPCHK(hipEventRecord(ev_splat[ps], side));
        }
        join_streams(st);
        return N;
    }

    // ---- feature pass and film filter.  Both keep the session: the pass has its own
    // tile list, pixel list, chain states and accumulators, and borrows only the ray and hit queues (when
    // they are large enough: growing them would reallocate the session's film with them), the traversal
    // overflow stack and the standalone trace's fetch counters.
    TileLayout ft_lay;
    DBuf<uint4> d_ft_tiles;
    DBuf<uint32_t> d_ft_pixel, d_ft_seed;
    DBuf<float4> d_ft_acc, d_ft_ray, d_ft_hit;
    DBuf<float4> d_dn_guide, d_dn_I[2];
    DBuf<float> d_dn_in, d_dn_out;

    // spp camera samples of every slot of `tiles` into d_ft_acc (3 float4 per slot) on `st`; returns the slots
    uint64_t render_features(const akr_feature_params &p, const akr_rect *tiles, int32_t n_tiles, hipStream_t st) {
        if (p.spp < 1) throw std::runtime_error("feature pass: spp must be >= 1");
        if (p.flags & ~AKR_PT_EXACT_CULL) throw std::runtime_error("feature pass: flags must be 0 or AKR_PT_EXACT_CULL");
        require_ready();
        if (!cam_set) throw std::runtime_error("camera not set (call akr_hip_set_camera)");
        if (n_tiles < 0 || (n_tiles > 0 && !tiles)) throw std::runtime_error("invalid tile list");
        ft_lay = layout_tiles(tiles, n_tiles, cam.width, cam.height, "feature pass");  // as setup_pixels lays them out
        const uint64_t N = ft_lay.n;
        serialize(st);
        if (N == 0) {
            mark_done(st);
            return 0;
        }
        d_ft_pixel.reserve(N);
        d_ft_seed.reserve(N);
        d_ft_acc.reserve(3 * N);
        float4 *rays = d_ray0.p, *hits = d_hit.p;
        if (N > cap) {
            d_ft_ray.reserve(2 * N);
            d_ft_hit.reserve(N);
            rays = d_ft_ray.p;
            hits = d_ft_hit.p;
        }
        expand_layout(ft_lay, d_ft_tiles, d_ft_pixel.p, st);
        HIPCHK(hipMemsetAsync(d_ft_acc.p, 0, 3 * N * sizeof(float4), st));
        const bool tight = !(opt.exact_cull || (p.flags & AKR_PT_EXACT_CULL));
        for (int s = 0; s < p.spp; s++) {
            timed("feature_rays", st, [&] {
                if (lens_active()) launch_feature_rays_lens(cam, lens, d_ft_pixel.p, (uint32_t)N, d_ft_seed.p, s == 0, rays, st);
                else launch_feature_rays(cam, d_ft_pixel.p, (uint32_t)N, d_ft_seed.p, s == 0, rays, st);
            });
            HIPCHK(hipMemsetAsync(d_work.p, 0, kTraceWords * sizeof(uint32_t), st));
            TraceArgs t = trace_args(d_work.p);
            t.rays = rays;
            t.n = (uint32_t)N;
            t.hits = hits;
            timed("trace_closest", st, [&] { trace_launch(TRACE_CLOSEST, tight, t, N, st); });
            FeatureArgs fa{};
            fa.sc = scene_dev();
            fa.ray_in = rays;
            fa.hit_in = hits;
            fa.seed = d_ft_seed.p;
            fa.acc = d_ft_acc.p;
            fa.n = (uint32_t)N;
            timed("features", st, [&] { launch_feature_shade(fa, st); });
        }
        HIPCHK(hipGetLastError());
        mark_done(st);
        return N;
    }

    static void check_denoise(const akr_denoise_params *p, int32_t width, int32_t height) {
        if (!p) throw std::runtime_error("denoise: null parameters");
        if (width <= 0 || height <= 0) throw std::runtime_error("denoise: the frame is empty (W * H == 0)");
        if ((uint64_t)width * (uint64_t)height >= (1ull << 31)) throw std::runtime_error("denoise: too many pixels");
        if (p->iterations < 1 || p->iterations > 8) throw std::runtime_error("denoise: iterations must be in 1..8");
        if (p->normal_squarings < 0 || p->normal_squarings > 8)
            throw std::runtime_error("denoise: normal_squarings must be in 0..8");
        if (!(p->sigma_depth > 0.0f) || !(p->sigma_albedo > 0.0f))
            throw std::runtime_error("denoise: sigma_depth and sigma_albedo must be > 0");
        if (p->sigma_color != p->sigma_color) throw std::runtime_error("denoise: sigma_color is NaN");
        if (p->flags & ~AKR_DENOISE_NO_DEMODULATE) throw std::runtime_error("denoise: unknown flags");
    }

    // ---- the variance-guided filter
    DBuf<float4> d_dn_V[2];

    static void check_denoise_guided(const akr_denoise_guided_params *p, int32_t width, int32_t height) {
        if (!p) throw std::runtime_error("denoise: null parameters");
        check_denoise(&p->base, width, height);
        if (!(p->sigma_variance > 0.0f) || !std::isfinite(p->sigma_variance))
            throw std::runtime_error("denoise: sigma_variance must be > 0 and finite");
    }

    // The filter on frame-ordered device buffers, enqueued on `st`.  var: the guided form, with the frame-ordered
    // variance (vr, vg, vb, K) and its sigma: the same prep and finish around the guided iteration
    void denoise(const akr_denoise_params &p, int32_t width, int32_t height, const float *rad, const float *w,
                 const float *feat, const float *var, float sigma_variance, float *out, hipStream_t st) {
        const uint32_t n = (uint32_t)((uint64_t)width * (uint64_t)height);
        d_dn_guide.reserve(3 * (size_t)n);
        for (int k = 0; k < 2; k++) {
            d_dn_I[k].reserve(n);
            if (var) d_dn_V[k].reserve(n);
        }
        const bool dm = !(p.flags & AKR_DENOISE_NO_DEMODULATE);
        serialize(st);
        timed("denoise_prep", st, [&] { launch_denoise_prep(rad, w, feat, n, dm, d_dn_guide.p, d_dn_I[0].p, st); });
        if (var)
            timed("denoise_prep_variance", st,
                  [&] { launch_denoise_prep_variance(var, d_dn_guide.p, d_dn_I[0].p, n, dm, d_dn_V[0].p, st); });
        for (int i = 0; i < p.iterations; i++) {
            DenoiseGuidedArgs g{};
            DenoiseArgs &a = g.d;
            a.guide = d_dn_guide.p;
            a.in = d_dn_I[i & 1].p;
            a.out = d_dn_I[(i + 1) & 1].p;
            a.width = width;
            a.height = height;
            a.step = 1 << i;
            a.squarings = p.normal_squarings;
            a.color_stop = p.sigma_color > 0.0f ? 1 : 0;
            a.sigma_depth = p.sigma_depth;
            a.sigma_albedo = p.sigma_albedo;
            const float sc = p.sigma_color * (1.0f / (float)(1 << i));
            a.sc2 = sc * sc;
            if (!var) {
                timed("denoise", st, [&] { launch_denoise_atrous(a, st); });
                continue;
            }
            g.vin = d_dn_V[i & 1].p;
            g.vout = d_dn_V[(i + 1) & 1].p;
            g.sv3 = (3.0f * sigma_variance) * sigma_variance;
            timed("denoise_guided", st, [&] { launch_denoise_atrous_guided(g, st); });
        }
        timed("denoise_finish", st, [&] { launch_denoise_finish(d_dn_guide.p, d_dn_I[p.iterations & 1].p, n, dm, out, st); });
        HIPCHK(hipGetLastError());
        mark_done(st);
    }

    // The host form of both filters: the frame-ordered inputs staged on the device (`variance`: the guided
    // form's plane, behind the others), the filter, the result back
    void denoise_host(const akr_denoise_params &p, int32_t width, int32_t height, const float *radiance, const float *weight,
                      const float *features, const float *variance, float sigma_variance, float *out_rgb) {
        const size_t n = (size_t)width * (size_t)height;
        hipStream_t st = stream;
        serialize(st);  // the staging buffers are shared by every denoise of the context
        d_dn_in.reserve((variance ? 20 : 16) * n);
        d_dn_out.reserve(3 * n);
        float *d_rad = d_dn_in.p, *d_w = d_rad + 3 * n, *d_feat = d_rad + 4 * n, *d_var = variance ? d_rad + 16 * n : nullptr;
        HIPCHK(hipMemcpyAsync(d_rad, radiance, 3 * n * sizeof(float), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_w, weight, n * sizeof(float), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_feat, features, 12 * n * sizeof(float), hipMemcpyHostToDevice, st));
        if (variance) HIPCHK(hipMemcpyAsync(d_var, variance, 4 * n * sizeof(float), hipMemcpyHostToDevice, st));
        denoise(p, width, height, d_rad, d_w, d_feat, d_var, sigma_variance, d_dn_out.p, st);
        HIPCHK(hipMemcpyAsync(out_rgb, d_dn_out.p, 3 * n * sizeof(float), hipMemcpyDeviceToHost, st));
        mark_done(st);
        HIPCHK(hipStreamSynchronize(st));
    }
};

namespace {

// the caller's stream, or the context's own
hipStream_t stream_of(const akr_hip_ctx *ctx, void *stream) { return stream ? reinterpret_cast<hipStream_t>(stream) : ctx->stream; }

template <class F>
int guard(akr_hip_ctx *ctx, F &&f) {
    if (!ctx) return -1;
    try {
        HIPCHK(hipSetDevice(ctx->device));
        f();
        return 0;
    } catch (const std::exception &e) {
        ctx->err = e.what();
        return -1;
    } catch (...) {
        ctx->err = "unknown error";
        return -1;
    }
}

// One call that extends or starts a session, after its argument checks (include/akr_hip.h: a refused call
// changes nothing, a failure while rendering ends the session).  A body that throws Refused has changed
// nothing but perhaps the session record, which is put back; after any other failure the film may be partly
// extended, and there is no session; otherwise the session is what the body left.
template <class F>
void session_call(akr_hip_ctx *ctx, F &&body) {
    const Session before = ctx->session;
    try {
        body();
    } catch (const Refused &) {
        ctx->session = before;
        throw;
    } catch (...) {
        ctx->drop_session();
        throw;
    }
}

}  // namespace

extern "C" {

int akr_hip_api_version(void) { return AKR_HIP_API_VERSION; }

int akr_hip_device_count(int *n) {
    if (!n) return -1;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    *n = c;
    return 0;
}

int akr_hip_create(int device, akr_hip_ctx **out) {
    if (!out) return -1;
    *out = nullptr;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess || device < 0 || device >= c) return -2;
    std::unique_ptr<akr_hip_ctx> ctx(new (std::nothrow) akr_hip_ctx());
    if (!ctx) return -1;
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess) return -1;
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) return -1;
    if (hipEventCreateWithFlags(&ctx->ev_done, hipEventDisableTiming) != hipSuccess) return -1;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        ctx->n_cu = prop.multiProcessorCount;
    *out = ctx.release();
    return 0;
}

int akr_hip_destroy(akr_hip_ctx *ctx) {
    delete ctx;
    return 0;
}

const char *akr_hip_last_error(const akr_hip_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int akr_hip_set_option(akr_hip_ctx *ctx, const char *key, int64_t value) {
    return guard(ctx, [&] {
        const std::string why = set_option(ctx->opt, key, value);
        if (!why.empty()) throw std::runtime_error(why);
    });
}

int akr_hip_upload_mesh(akr_hip_ctx *ctx, const float *vertices, uint64_t n_vertices, const int32_t *indices,
                        const float *normals, const float *texcoords, const int32_t *material_indices,
                        uint64_t n_triangles, const int32_t *material_slots, int32_t n_slots, int32_t *geom_id) {
    return guard(ctx, [&] {
        if (n_triangles && (!vertices || !indices || !normals || !texcoords || !material_indices))
            throw std::runtime_error("null mesh array");
        if (ctx->n_tris() + n_triangles >= (1ull << 31)) throw std::runtime_error("scene too large");
        const uint64_t vb = ctx->verts.size() / 3;
        for (uint64_t i = 0; i < 3 * n_triangles; i++)
            if (indices[i] < 0 || (uint64_t)indices[i] >= n_vertices) throw std::runtime_error("vertex index out of range");
        for (uint64_t t = 0; t < n_triangles; t++) {
            int32_t m = material_indices[t];
            if (m >= n_slots) throw std::runtime_error("material index beyond the mesh's material list");
        }
        ctx->verts.insert(ctx->verts.end(), vertices, vertices + 3 * n_vertices);
        for (uint64_t i = 0; i < 3 * n_triangles; i++) ctx->idx.push_back((int32_t)(indices[i] + vb));
        ctx->normals.insert(ctx->normals.end(), normals, normals + 9 * n_triangles);
        ctx->texcoords.insert(ctx->texcoords.end(), texcoords, texcoords + 6 * n_triangles);
        for (uint64_t t = 0; t < n_triangles; t++) {
            int32_t m = material_indices[t];
            ctx->matid.push_back(m < 0 ? -1 : material_slots[m]);  // -1: no material (scene.h:73-76)
        }
        if (geom_id) *geom_id = (int32_t)ctx->mesh_base.size() - 1;
        ctx->mesh_base.push_back((uint32_t)ctx->n_tris());
        ctx->scene_dirty = true;
        ctx->drop_session();
        ctx->accel_built = false;
    });
}

int akr_hip_clear_meshes(akr_hip_ctx *ctx) {
    return guard(ctx, [&] {
        ctx->verts.clear();
        ctx->idx.clear();
        ctx->normals.clear();
        ctx->texcoords.clear();
        ctx->matid.clear();
        ctx->mesh_base.assign(1, 0u);
        ctx->scene_dirty = true;
        ctx->drop_session();
        ctx->accel_built = false;
    });
}

int akr_hip_upload_images(akr_hip_ctx *ctx, const float *rgba, const int32_t *widths, const int32_t *heights,
                          int32_t n_images) {
    return guard(ctx, [&] {
        ctx->images.clear();
        ctx->img_off.clear();
        ctx->img_w.clear();
        ctx->img_h.clear();
        int64_t off = 0;
        for (int i = 0; i < n_images; i++) {
            if (widths[i] <= 0 || heights[i] <= 0) throw std::runtime_error("empty image");
            ctx->img_off.push_back(off);
            ctx->img_w.push_back(widths[i]);
            ctx->img_h.push_back(heights[i]);
            off += 4 * (int64_t)widths[i] * heights[i];
        }
        ctx->images.assign(rgba, rgba + off);
        ctx->scene_dirty = true;
        ctx->drop_session();
    });
}

int akr_hip_upload_textures(akr_hip_ctx *ctx, const akr_texture *textures, int32_t n) {
    return guard(ctx, [&] {
        ctx->texs.assign(textures, textures + n);
        ctx->scene_dirty = true;
        ctx->drop_session();
    });
}

int akr_hip_upload_materials(akr_hip_ctx *ctx, const akr_material *materials, int32_t n) {
    return guard(ctx, [&] {
        ctx->mats.assign(materials, materials + n);
        ctx->scene_dirty = true;
        ctx->drop_session();
    });
}

int akr_hip_upload_lights(akr_hip_ctx *ctx, const akr_area_light *lights, int32_t n, const float *power) {
    return guard(ctx, [&] {
        if (n < 0 || (n > 0 && (!lights || !power))) throw std::runtime_error("invalid light list");
        ctx->lights.assign(lights, lights + n);
        ctx->power.assign(power, power + n);
        ctx->scene_dirty = true;
        ctx->drop_session();
    });
}

namespace {
// Distribution1D (common/distribution.h:46-64) over func[0..n): the sequential f32 sums, the CDF
// divided by the integral (or uniform when that is 0), and sample_discrete's pdf func / (integral * n)
// (0 for a function that is 0 everywhere, which no draw selects).  Returns the integral.
float env_dist1d(const float *func, int n, float *cdf, float *pdf) {
    const float fn = (float)n;
    cdf[0] = 0.0f;
    for (int i = 0; i < n; i++) cdf[i + 1] = cdf[i] + func[i] / fn;
    const float fi = cdf[n];
    for (int i = 1; i <= n; i++) cdf[i] = fi == 0.0f ? (float)i / fn : cdf[i] / fi;
    for (int i = 0; i < n; i++) pdf[i] = fi == 0.0f ? 0.0f : func[i] / (fi * fn);
    return fi;
}
// |q|_2 of the octahedron's point over (x, y) of the square: env_decode's len (kernels.hip), same operations
float env_len(float x, float y) {
    const float z = (1.0f - std::fabs(x)) - std::fabs(y);
    if (z < 0.0f) {
        const float fx = (1.0f - std::fabs(y)) * (x < 0.0f ? -1.0f : 1.0f);
        const float fy = (1.0f - std::fabs(x)) * (y < 0.0f ? -1.0f : 1.0f);
        x = fx;
        y = fy;
    }
    float s = x * x;
    s += y * y;
    s += z * z;
    return std::sqrt(s);
}

void env_unit(akr_hip_ctx *ctx, bool sample, const float *in, uint64_t n, float *dir, float *rgb, float *pdf) {
    const EnvDev &env = ctx->require_env();
    if (n == 0) return;
    if (!in || !rgb || !pdf || (sample && !dir)) throw std::runtime_error("environment: null buffer");
    if (n > (1ull << 28)) throw std::runtime_error("environment: too many inputs in one call");
    const size_t k = sample ? 2 : 3;
    DBuf<float> d_in, d_out;  // out: dir (3n), rgb (3n), pdf (n)
    hipStream_t st = ctx->stream;
    ctx->serialize(st);
    d_in.upload(in, k * n, st);
    d_out.reserve(7 * n);
    EnvUnitArgs a{};
    a.env = env;
    a.in = d_in.p;
    a.n = (uint32_t)n;
    a.dir = d_out.p;
    a.rgb = d_out.p + 3 * n;
    a.pdf = d_out.p + 6 * n;
    launch_env_unit(sample, a, st);
    HIPCHK(hipGetLastError());
    if (sample) HIPCHK(hipMemcpyAsync(dir, a.dir, 3 * n * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(rgb, a.rgb, 3 * n * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(pdf, a.pdf, n * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
}
}  // namespace

int akr_hip_upload_environment(akr_hip_ctx *ctx, const akr_environment *e, const float *rgb) {
    return guard(ctx, [&] {
        // no render of this context may still read the tables that are replaced here
        if (ctx->done_recorded) HIPCHK(hipEventSynchronize(ctx->ev_done));
        ctx->drop_session();
        ctx->env_rec_stale = true;
        if (!rgb) {  // remove
            ctx->env = EnvDev{};
            return;
        }
        if (!e) throw std::runtime_error("environment: null description");
        const int n = e->resolution;
        if (n < 1 || n > 2048) throw std::runtime_error("environment: resolution must be in [1, 2048]");
        if (!(e->select_prob > 0.0f && e->select_prob < 1.0f))
            throw std::runtime_error("environment: select_prob must be inside (0, 1)");
        for (int c = 0; c < 3; c++)
            if (!std::isfinite(e->scale[c]) || e->scale[c] < 0.0f)
                throw std::runtime_error("environment: scale must be finite and not negative");
        for (int c = 0; c < 9; c++)
            if (!std::isfinite(e->world_to_env[c])) throw std::runtime_error("environment: world_to_env is not finite");
        const size_t nn = (size_t)n * n;
        for (size_t k = 0; k < 3 * nn; k++)
            if (!std::isfinite(rgb[k]) || rgb[k] < 0.0f)
                throw std::runtime_error("environment: texel " + std::to_string(k / 3) + " is negative or not finite");
        // f_ij = luminance(texel * scale) / |q_c|^3 at the texel's centre; one conditional per row, the
        // marginal over the rows' integrals (host: a device scan would round differently)
        const float fn = (float)n;
        const size_t o_mcdf = 0, o_mpdf = o_mcdf + n + 1, o_ccdf = o_mpdf + n, o_cpdf = o_ccdf + (size_t)n * (n + 1);
        std::vector<float> tab(o_cpdf + nn), func(n), rows(n);
        std::vector<float4> map(nn);
        for (int j = 0; j < n; j++) {
            const float yc = (((float)j + 0.5f) / fn) * 2.0f - 1.0f;
            for (int i = 0; i < n; i++) {
                const float xc = (((float)i + 0.5f) / fn) * 2.0f - 1.0f;
                const float *t = rgb + 3 * ((size_t)j * n + i);
                map[(size_t)j * n + i] = make_float4(t[0], t[1], t[2], 0.0f);
                float lum = (t[0] * e->scale[0]) * 0.2126f;  // Color::luminance, common/color.h:52-55
                lum += (t[1] * e->scale[1]) * 0.7152f;
                lum += (t[2] * e->scale[2]) * 0.0722f;
                const float len = env_len(xc, yc);
                func[i] = lum / ((len * len) * len);
            }
            rows[j] = env_dist1d(func.data(), n, &tab[o_ccdf + (size_t)j * (n + 1)], &tab[o_cpdf + (size_t)j * n]);
        }
        const float total = env_dist1d(rows.data(), n, &tab[o_mcdf], &tab[o_mpdf]);
        if (!(total > 0.0f) || !std::isfinite(total))
            throw std::runtime_error("environment: the map's luminance is zero everywhere (or overflows): nothing to sample");
        ctx->d_env_map.upload(map.data(), map.size(), ctx->stream);
        ctx->d_env_tab.upload(tab.data(), tab.size(), ctx->stream);
        HIPCHK(hipStreamSynchronize(ctx->stream));  // the staging vectors end here
        EnvDev d{};
        d.map = (decltype(d.map))ctx->d_env_map.p;
        const float *tp = ctx->d_env_tab.p;
        d.marg_cdf = (decltype(d.marg_cdf))(tp + o_mcdf);
        d.marg_pdf = (decltype(d.marg_pdf))(tp + o_mpdf);
        d.cond_cdf = (decltype(d.cond_cdf))(tp + o_ccdf);
        d.cond_pdf = (decltype(d.cond_pdf))(tp + o_cpdf);
        d.n = n;
        d.select_prob = e->select_prob;
        for (int c = 0; c < 3; c++) d.scale[c] = e->scale[c];
        for (int c = 0; c < 9; c++) d.R[c] = e->world_to_env[c];
        ctx->env = d;
    });
}

int akr_hip_environment_sample(akr_hip_ctx *ctx, const float *u, uint64_t n, float *dir, float *rgb, float *pdf) {
    return guard(ctx, [&] { env_unit(ctx, true, u, n, dir, rgb, pdf); });
}

int akr_hip_environment_eval(akr_hip_ctx *ctx, const float *dir, uint64_t n, float *rgb, float *pdf) {
    return guard(ctx, [&] { env_unit(ctx, false, dir, n, nullptr, rgb, pdf); });
}

namespace {
// An imported tree's triangle records must be this scene's triangles: each record equals the one
// the builders write for its gid (v0 and the f32 edges v1 - v0, v2 - v0, instance.h:49-50, bit for
// bit), and every scene triangle is referenced by some leaf.  Shading reads the context's own
// vertices, so a tree shared from another scene would otherwise render wrong geometry without an
// error.  O(n_tris) on `n_threads` threads.
void check_tris_match_mesh(const akr_hip_ctx *ctx, const akr_bvh_tri *tr, uint64_t n, int n_threads) {
    const uint64_t nt = ctx->n_tris();
    // relaxed atomics: several threads may mark the same triangle (SBVH duplicates), ADVICE r4
    std::unique_ptr<std::atomic<uint8_t>[]> covered(new std::atomic<uint8_t>[nt]);
    for (uint64_t g = 0; g < nt; g++) covered[g].store(0, std::memory_order_relaxed);
    const int T = n_threads > 0 ? std::min(n_threads, 64)
                                : (int)std::min(64u, std::max(1u, std::thread::hardware_concurrency()));
    std::vector<uint64_t> bad(T, UINT64_MAX);
    run_on_threads(T, [&](int t) {
        const uint64_t r0 = n * t / T, r1 = n * (t + 1) / T;
        for (uint64_t r = r0; r < r1; r++) {
            const uint32_t g = tr[r].gid;  // < nt: checked by validate_bvh2
            const float *v0 = &ctx->verts[3 * (size_t)ctx->idx[3 * (size_t)g + 0]];
            const float *v1 = &ctx->verts[3 * (size_t)ctx->idx[3 * (size_t)g + 1]];
            const float *v2 = &ctx->verts[3 * (size_t)ctx->idx[3 * (size_t)g + 2]];
            float want[9];
            for (int k = 0; k < 3; k++) {
                want[k] = v0[k];
                want[3 + k] = v1[k] - v0[k];
                want[6 + k] = v2[k] - v0[k];
            }
            const float got[9] = {tr[r].v0[0], tr[r].v0[1], tr[r].v0[2], tr[r].e1[0], tr[r].e1[1],
                                  tr[r].e1[2], tr[r].e2[0], tr[r].e2[1], tr[r].e2[2]};
            if (std::memcmp(want, got, sizeof(want)) != 0) {
                bad[t] = r;
                return;
            }
            covered[g].store(1, std::memory_order_relaxed);
        }
    });
    for (uint64_t r : bad)
        if (r != UINT64_MAX)
            throw std::runtime_error("imported BVH: triangle record " + std::to_string(r) + " (gid " +
                                     std::to_string(tr[r].gid) + ") does not match this scene's triangle");
    for (uint64_t g = 0; g < nt; g++)
        if (!covered[g].load(std::memory_order_relaxed))
            throw std::runtime_error("imported BVH: scene triangle " + std::to_string(g) + " is in no leaf");
}

// After the BVH2 of ctx->bvh exists (built or imported): the wide view, its device copy, the BVH2
// itself for the exact lane path, the accel info, and the scene's shading records.
void finish_accel(akr_hip_ctx *ctx, int n_threads) {
        auto &b = ctx->bvh;
        ctx->accel_built = false;  // set again only once every buffer below holds the new tree
        {
            Bvh4Output w;
            build_bvh4(b.nodes, w, n_threads, ctx->wide_collapse);
            if (w.nodes.size() >= kMaxWideNodes)
                throw std::runtime_error("scene too large: the wide view needs fewer than 2^26 nodes (about 100 M triangles)");
            ctx->bvh4 = std::move(w);
        }
        ctx->d_nodes.upload(b.nodes.data(), b.nodes.size(), ctx->stream);
        // Device copy of the wide view: each leaf record is followed by its triangles in one blob, so
        // the leaf phase fetches the exact box and the first triangle in one batch; leaf refs in the
        // wide nodes become float4 offsets into the blob.
        // Offsets by a serial prefix sum, then the records and their triangles are copied on
        // `n_threads` threads (the blob is ~1 GB on C3).
        const auto &leaves = ctx->bvh4.leaves;
        // (leaf_layout.h: the offsets, the size check and the references' one-triangle flag)
        const akr::LeafLayout lay = akr::leaf_layout(leaves.size(), (size_t)std::max(1, ctx->opt.leaf_align),
                                                     [&](size_t i) { return leaves[i].count; });
        const std::vector<uint32_t> &leaf_off = lay.offset;
        const size_t words = lay.words, pad = akr::kLeafBlobPad, align = (size_t)std::max(1, ctx->opt.leaf_align);
        std::unique_ptr<float4[]> blob(new float4[words + pad]);
        if (align > 1) std::memset(static_cast<void *>(blob.get()), 0, sizeof(float4) * (words + pad));  // the gaps
        else std::memset(static_cast<void *>(blob.get() + words), 0, sizeof(float4) * pad);
        const float4 *tri4 = reinterpret_cast<const float4 *>(b.tris.data());
        std::vector<akr_bvh4_node> wn = ctx->bvh4.nodes;
        auto remap = [&](uint32_t r) {
            if (r == AKR_CHILD_EMPTY || !(r & AKR_CHILD_LEAF)) return r;
            const uint32_t i = r & 0x7FFFFFFFu;
            return lay.ref(i, leaves[i].count);
        };
        const int nt = n_threads > 0 ? std::min(n_threads, 64)
                                       : (int)std::min(64u, std::max(1u, std::thread::hardware_concurrency()));
        auto fill = [&](int t) {
            const size_t l0 = leaves.size() * t / nt, l1 = leaves.size() * (t + 1) / nt;
            for (size_t i = l0; i < l1; i++) {
                const akr_bvh_leaf &l = leaves[i];
                float4 *o = blob.get() + leaf_off[i];
                float4 h0, h1;
                h0.x = l.lo[0], h0.y = l.lo[1], h0.z = l.lo[2], h0.w = l.hi[0];
                uint32_t fc[2] = {l.first, l.count};
                h1.x = l.hi[1], h1.y = l.hi[2];
                std::memcpy(&h1.z, &fc[0], 4);
                std::memcpy(&h1.w, &fc[1], 4);
                o[0] = h0;
                o[1] = h1;
                std::memcpy(o + 2, tri4 + 3 * (size_t)l.first, sizeof(float4) * 3 * (size_t)l.count);
            }
            const size_t n0 = wn.size() * t / nt, n1 = wn.size() * (t + 1) / nt;
            for (size_t i = n0; i < n1; i++)
                for (auto &c : wn[i].child) c = remap(c);
        };
        run_on_threads(nt, fill);
        ctx->wide_root_dev = remap(ctx->bvh4.root_ref);
        size_t n_one = 0;
        for (const akr_bvh_leaf &l : leaves) n_one += l.count == 1 ? 1 : 0;
        ctx->leaf_one_kernel = akr::leaf_one_pays(n_one, leaves.size());
        ctx->d_wnodes.reserve(1);  // never a null pointer, even for an empty scene
        ctx->d_wleaves.reserve(1);
        ctx->d_wnodes.upload(wn.data(), wn.size(), ctx->stream);
        ctx->d_wleaves.upload(blob.get(), words + pad, ctx->stream);
        // the uploaded tree's bytes (the DBufs' capacities only grow), for the form rule
        ctx->bvh_dev_bytes = (uint64_t)wn.size() * sizeof(akr_bvh4_node) + (uint64_t)(words + pad) * sizeof(float4);
        HIPCHK(hipStreamSynchronize(ctx->stream));  // before the host staging vectors go away
        ctx->d_tris.upload(reinterpret_cast<const float4 *>(b.tris.data()), 3 * b.tris.size(), ctx->stream);
        HIPCHK(hipStreamSynchronize(ctx->stream));
        ctx->info.n_nodes = b.nodes.size();
        ctx->info.n_tris = b.tris.size();
        ctx->info.max_depth = b.max_depth;
        ctx->info.max_leaf = b.max_leaf;
        ctx->info.build_ms = b.build_ms;
        ctx->info.sah_cost = b.sah_cost;
        ctx->accel_built = true;
        ctx->commit_scene();
}
}  // namespace

int akr_hip_build_accel(akr_hip_ctx *ctx, const akr_build_params *params) {
    return guard(ctx, [&] {
        akr_build_params p{};
        p.max_leaf_size = 4;
        p.n_bins = 32;
        p.traversal_cost = 1.0f;
        p.intersect_cost = 4.0f;
        if (params) p = *params;
        BvhInput in{ctx->verts.data(), ctx->idx.data(), ctx->n_tris()};
        ctx->drop_session();
        ctx->accel_built = false;  // until the new tree is on the device (a failure below leaves none)
        if (p.builder == AKR_BUILDER_LBVH) build_lbvh_gpu(in, ctx->bvh, ctx->stream);
        else if (p.builder == AKR_BUILDER_SAH || p.builder == AKR_BUILDER_SBVH) build_bvh(in, p, ctx->bvh);
        else throw std::runtime_error("unknown builder");
        if (p.wide_collapse != AKR_COLLAPSE_SAH && p.wide_collapse != AKR_COLLAPSE_BALANCED)
            throw std::runtime_error("unknown wide_collapse");
        ctx->wide_collapse = p.wide_collapse;
        finish_accel(ctx, p.n_threads);
    });
}

int akr_hip_import_accel(akr_hip_ctx *ctx, const void *nodes, uint64_t n_nodes, const void *tris, uint64_t n_tris,
                         int32_t n_threads) {
    return guard(ctx, [&] {
        if (!nodes || n_nodes == 0 || (n_tris && !tris)) throw std::runtime_error("null or empty BVH arrays");
        const auto *nd = reinterpret_cast<const akr_bvh_node *>(nodes);
        const auto *tr = reinterpret_cast<const akr_bvh_tri *>(tris);
        int max_leaf = 0;
        const int depth = validate_bvh2(nd, n_nodes, tr, n_tris, ctx->n_tris(), max_leaf);  // throws on bad input
        check_tris_match_mesh(ctx, tr, n_tris, n_threads);  // the records are this scene's triangles
        ctx->drop_session();
        ctx->accel_built = false;  // until the new tree is on the device (a failure below leaves none)
        BvhOutput &b = ctx->bvh;
        b.nodes.assign(nd, nd + n_nodes);
        b.tris.assign(tr, tr + n_tris);
        b.max_depth = depth;
        b.max_leaf = max_leaf;
        b.sah_cost = 0.0;  // not known for an imported tree
        b.build_ms = 0.0;
        ctx->wide_collapse = AKR_COLLAPSE_SAH;
        finish_accel(ctx, n_threads);
    });
}

int akr_hip_accel_info(akr_hip_ctx *ctx, akr_accel_info *info) {
    return guard(ctx, [&] {
        if (!ctx->accel_built) throw std::runtime_error("acceleration structure not built");
        *info = ctx->info;
    });
}

int akr_hip_accel_export(akr_hip_ctx *ctx, void *nodes, uint64_t node_bytes, void *tris, uint64_t tri_bytes) {
    return guard(ctx, [&] {
        if (!ctx->accel_built) throw std::runtime_error("acceleration structure not built");
        uint64_t nb = ctx->bvh.nodes.size() * sizeof(akr_bvh_node), tb = ctx->bvh.tris.size() * sizeof(akr_bvh_tri);
        if (node_bytes < nb || tri_bytes < tb) throw std::runtime_error("export buffers too small");
        std::memcpy(nodes, ctx->bvh.nodes.data(), nb);
        std::memcpy(tris, ctx->bvh.tris.data(), tb);
    });
}

int akr_hip_set_camera(akr_hip_ctx *ctx, const akr_camera *camera) {
    return guard(ctx, [&] {
        if (!camera) throw std::runtime_error("null camera");
        ctx->cam = make_camera(*camera);
        ctx->cam_set = true;
        ctx->drop_session();
    });
}

int akr_hip_set_lens(akr_hip_ctx *ctx, float lens_radius, float focal_distance) {
    return guard(ctx, [&] {
        // checked before anything is stored: a refused call leaves the lens and the session as they were
        if (!std::isfinite(lens_radius) || lens_radius < 0)
            throw std::runtime_error("set_lens: lens_radius must be finite and >= 0 (got " + std::to_string(lens_radius) + ")");
        if (!std::isfinite(focal_distance) || focal_distance < 0)
            throw std::runtime_error("set_lens: focal_distance must be finite and >= 0 (got " +
                                     std::to_string(focal_distance) + ")");
        ctx->lens = LensDev{lens_radius, focal_distance};
        ctx->drop_session();
    });
}

int akr_hip_lens(akr_hip_ctx *ctx, float *lens_radius, float *focal_distance, int32_t *active) {
    return guard(ctx, [&] {
        if (lens_radius) *lens_radius = ctx->lens.radius;
        if (focal_distance) *focal_distance = ctx->lens.focal;
        if (active) *active = ctx->lens_active() ? 1 : 0;
    });
}

int akr_hip_trace(akr_hip_ctx *ctx, const akr_ray *rays, uint64_t n, akr_hit *hits, int any_hit) {
    return guard(ctx, [&] {
        if (n == 0) return;
        if (!rays || !hits) throw std::runtime_error("null ray or hit buffer");
        static_assert(sizeof(akr_ray) == 2 * sizeof(float4), "akr_ray layout");
        ctx->d_trace_rays.upload(reinterpret_cast<const float4 *>(rays), 2 * n, ctx->stream);
        ctx->d_trace_hits.reserve(n);
        ctx->trace(ctx->d_trace_rays.p, n, ctx->d_trace_hits.p, any_hit, ctx->stream);
        HIPCHK(hipMemcpyAsync(hits, ctx->d_trace_hits.p, n * sizeof(akr_hit), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    });
}

int akr_hip_trace_device(akr_hip_ctx *ctx, const void *d_rays, uint64_t n, void *d_hits, int any_hit, void *stream) {
    return guard(ctx, [&] {
        if (n == 0) return;
        if (!d_rays || !d_hits) throw std::runtime_error("null ray or hit buffer");
        hipStream_t st = stream_of(ctx, stream);
        ctx->trace(reinterpret_cast<const float4 *>(d_rays), n, reinterpret_cast<akr_hit *>(d_hits), any_hit, st);
    });
}

int akr_hip_render_node(akr_hip_ctx *const *ctxs, int32_t n_ctx, const akr_pt_params *params, const akr_rect *tiles,
                        int32_t n_tiles, float *radiance, float *weight) {
    if (!ctxs || n_ctx < 1) return -1;
    for (int32_t k = 0; k < n_ctx; k++)
        if (!ctxs[k]) return -1;
    akr_hip_ctx *lead = ctxs[0];
    if (!params || !radiance || !weight || n_tiles < 0 || (n_tiles > 0 && !tiles)) {
        lead->err = "null or invalid argument";
        return -1;
    }
    for (int32_t k = 0; k < n_ctx; k++)
        for (int32_t j = 0; j < k; j++)
            if (ctxs[j] == ctxs[k]) {  // the per-context render threads would share one context
                lead->err = "a context is listed twice";
                return -1;
            }
    // tile j -> context j % n_ctx (interleaved, like the multi-process split of akari_amd/dist.py);
    // one host thread per context, each bound to its device by guard()
    std::vector<std::vector<akr_rect>> part(n_ctx);
    for (int32_t j = 0; j < n_tiles; j++) part[j % n_ctx].push_back(tiles[j]);
    std::vector<uint64_t> npix(n_ctx, 0);
    std::vector<int> status(n_ctx, 0);
    run_on_threads(n_ctx, [&](int k) {
        akr_hip_ctx *c = ctxs[k];
        status[k] = guard(c, [&] {
            hipStream_t st = c->stream;
            const uint64_t N = c->render(*params, part[k].data(), (int32_t)part[k].size(), st);
            c->verify_weights(st, N, params->spp);  // joins the render into st and checks it
            if (!c->opt.verify) {
                c->join_streams(st);
                HIPCHK(hipStreamSynchronize(st));
                c->check_fault();
            }
            c->mark_done(st);
            npix[k] = N;
        });
    });
    for (int32_t k = 0; k < n_ctx; k++)
        if (status[k] != 0) {
            if (k) lead->err = "context " + std::to_string(k) + ": " + ctxs[k]->err;
            return -1;
        }
    // Gather on the lead device (Film::merge_tile, core/film.h:85-95).  Every other context pushes its
    // packed film and pixel list into its own staging buffers on the lead device from its own stream
    // (device-to-device peer copies, over xGMI between GPUs), so the copies of all contexts run at
    // once; the lead stream waits for each context's copy event and k_merge_film adds the films into
    // the frame in context order (the host loop's order).  No host synchronisation until the frame
    // goes back to the host.
    return guard(lead, [&] {
        const int W = lead->cam.width, H = lead->cam.height;
        const uint64_t F = (uint64_t)W * (uint64_t)H;
        hipStream_t st = lead->stream;
        for (int32_t k = 1; k < n_ctx; k++)
            if (ctxs[k]->device != lead->device) {
                const hipError_t e = hipDeviceEnablePeerAccess(ctxs[k]->device, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIPCHK(e);
                (void)hipGetLastError();
            }
        lead->d_frame.reserve(4 * F);
        float *frad = lead->d_frame.p, *fw = lead->d_frame.p + 3 * F;
        HIPCHK(hipMemcpyAsync(frad, radiance, 3 * F * sizeof(float), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(fw, weight, F * sizeof(float), hipMemcpyHostToDevice, st));
        // a pixel listed r times by one context (overlapping tiles) goes to its r-th launch, so the
        // adds of a pixel stay in list order and no launch adds one pixel twice
        std::vector<uint32_t> seen(F, 0), all_order;
        std::vector<std::vector<std::pair<size_t, uint32_t>>> launches(n_ctx);  // (offset, count) per rank
        for (int32_t k = 0; k < n_ctx; k++) {
            const uint64_t N = npix[k];
            if (N == 0) continue;
            std::fill(seen.begin(), seen.end(), 0u);
            std::vector<std::vector<uint32_t>> rank;
            const std::vector<uint32_t> &pl = ctxs[k]->host_pixels();
            for (uint64_t i = 0; i < N; i++) {
                const uint32_t r = seen[frame_index(pl[i], W)]++;
                if (r >= rank.size()) rank.emplace_back();
                rank[r].push_back((uint32_t)i);
            }
            if (rank.size() == 1) {
                launches[k].push_back({SIZE_MAX, (uint32_t)N});  // identity order
                continue;
            }
            for (auto &ord : rank) {
                launches[k].push_back({all_order.size(), (uint32_t)ord.size()});
                all_order.insert(all_order.end(), ord.begin(), ord.end());
            }
        }
        if (!all_order.empty()) lead->d_gorder.upload(all_order.data(), all_order.size(), st);
        // the peer pushes: one staging pair per context on the lead device, each copy on its
        // context's stream after that context's render
        if (lead->g_film.size() < (size_t)n_ctx) {
            lead->g_film.resize(n_ctx);
            lead->g_pix.resize(n_ctx);
        }
        for (int32_t k = 1; k < n_ctx; k++) {
            akr_hip_ctx *c = ctxs[k];
            const uint64_t N = npix[k];
            if (N == 0 || c == lead) continue;
            if (!lead->g_film[k]) {
                lead->g_film[k].reset(new DBuf<float4>());
                lead->g_pix[k].reset(new DBuf<uint32_t>());
            }
            lead->g_film[k]->reserve(N);  // on the lead device (current)
            lead->g_pix[k]->reserve(N);
            HIPCHK(hipSetDevice(c->device));
            if (!c->ev_gather) HIPCHK(hipEventCreateWithFlags(&c->ev_gather, hipEventDisableTiming));
            HIPCHK(hipMemcpyPeerAsync(lead->g_film[k]->p, lead->device, c->d_film.p, c->device, N * sizeof(float4),
                                      c->stream));
            HIPCHK(hipMemcpyPeerAsync(lead->g_pix[k]->p, lead->device, c->d_pixel.p, c->device, N * sizeof(uint32_t),
                                      c->stream));
            HIPCHK(hipEventRecord(c->ev_gather, c->stream));
            c->mark_done(c->stream);  // the context's film is not reused before the copy is done
            HIPCHK(hipSetDevice(lead->device));
        }
        for (int32_t k = 0; k < n_ctx; k++) {
            akr_hip_ctx *c = ctxs[k];
            if (npix[k] == 0) continue;
            const float4 *film = c->d_film.p;
            const uint32_t *pix = c->d_pixel.p;
            if (c != lead) {
                HIPCHK(hipStreamWaitEvent(st, c->ev_gather, 0));
                film = lead->g_film[k]->p;
                pix = lead->g_pix[k]->p;
            }
            for (const auto &l : launches[k])
                launch_merge_film(film, pix, l.first == SIZE_MAX ? nullptr : lead->d_gorder.p + l.first, l.second, W,
                                  frad, fw, st);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(radiance, frad, 3 * F * sizeof(float), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(weight, fw, F * sizeof(float), hipMemcpyDeviceToHost, st));
        lead->mark_done(st);
        HIPCHK(hipStreamSynchronize(st));
        for (int32_t k = 1; k < n_ctx; k++)  // a context's next call orders after its copy anyway
            if (ctxs[k] != lead && npix[k]) {
                HIPCHK(hipSetDevice(ctxs[k]->device));
                HIPCHK(hipStreamSynchronize(ctxs[k]->stream));
            }
        HIPCHK(hipSetDevice(lead->device));
    });
}

namespace {
// Film::merge_tile (core/film.h:85-95) of the context's packed film into full-frame host buffers
// (per_slot: a session whose slots hold different counts, checked against its per-slot counts)
void merge_film(akr_hip_ctx *ctx, uint64_t N, int spp, float *radiance, float *weight, bool per_slot = false) {
    hipStream_t st = ctx->stream;
    if (N == 0) {
        ctx->mark_done(st);
        return;
    }
    // the render's last splat runs on the internal side stream: wait for both internal streams on
    // the host before the copy, rather than trusting the DMA engine to honour the caller stream's
    // cross-stream event waits (two flaky short-weight reads were seen, never reproduced)
    ctx->host_join();
    HIPCHK(hipStreamSynchronize(st));
    ctx->check_fault();
    ctx->verify_weights(st, N, spp, per_slot);
    std::vector<float4> film(N);
    std::vector<uint32_t> counts;
    if (per_slot && ctx->opt.verify) {
        counts.resize(N);
        HIPCHK(hipMemcpyAsync(counts.data(), ctx->d_count.p, N * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipMemcpyAsync(film.data(), ctx->d_film.p, N * sizeof(float4), hipMemcpyDeviceToHost, st));
    ctx->mark_done(st);
    HIPCHK(hipStreamSynchronize(st));
    if (ctx->opt.verify) {  // the read-back itself: every copied slot holds spp samples
        uint64_t bad = 0;
        for (uint64_t k = 0; k < N; k++) bad += film[k].w != (float)(per_slot ? counts[k] : (uint32_t)spp);
        if (bad) throw std::runtime_error("film read-back: " + std::to_string(bad) + " of " + std::to_string(N) +
                                          " pixels do not hold " +
                                          (per_slot ? std::string("their expected") : std::to_string(spp)) + " samples");
    }
    const int W = ctx->cam.width;
    const std::vector<uint32_t> &pl = ctx->host_pixels();
    for (uint64_t k = 0; k < N; k++) {
        const uint64_t pix = frame_index(pl[k], W);
        radiance[3 * pix + 0] += film[k].x;
        radiance[3 * pix + 1] += film[k].y;
        radiance[3 * pix + 2] += film[k].z;
        weight[pix] += film[k].w;
    }
}

// The same film to packed device buffers on `st`, overwriting them.  rendered: the call drew samples, whose
// fault, without "verify", the next render reports
void unpack_film(akr_hip_ctx *ctx, uint64_t N, int spp, float *d_radiance, float *d_weight, hipStream_t st, bool rendered,
                 bool per_slot = false) {
    ctx->timed("unpack", st, [&] { launch_unpack(ctx->d_film.p, (uint32_t)N, d_radiance, d_weight, st); });
    HIPCHK(hipGetLastError());
    ctx->verify_weights(st, N, spp, per_slot);
    if (rendered) ctx->unchecked_render = !ctx->opt.verify;
    ctx->mark_done(st);
}
}  // namespace

int akr_hip_render(akr_hip_ctx *ctx, const akr_pt_params *params, const akr_rect *tiles, int32_t n_tiles,
                   float *radiance, float *weight) {
    return guard(ctx, [&] {
        if (!params || !radiance || !weight) throw std::runtime_error("null argument");
        const uint64_t N = ctx->render(*params, tiles, n_tiles, ctx->stream);
        merge_film(ctx, N, params->spp, radiance, weight);
        open_session(ctx->session, *params, N, params->spp, params->spp > 0);
    });
}

int akr_hip_render_ao(akr_hip_ctx *ctx, const akr_ao_params *params, const akr_rect *tiles, int32_t n_tiles,
                      float *radiance, float *weight) {
    return guard(ctx, [&] {
        if (!params || !radiance || !weight) throw std::runtime_error("null argument");
        merge_film(ctx, ctx->render_ao(*params, tiles, n_tiles, ctx->stream), params->spp, radiance, weight);
    });
}

int akr_hip_render_features(akr_hip_ctx *ctx, const akr_feature_params *params, const akr_rect *tiles, int32_t n_tiles,
                            float *features) {
    return guard(ctx, [&] {
        if (!params || !features) throw std::runtime_error("null argument");
        hipStream_t st = ctx->stream;
        const uint64_t N = ctx->render_features(*params, tiles, n_tiles, st);
        if (N == 0) return;
        std::vector<float> rec(12 * N);
        HIPCHK(hipMemcpyAsync(rec.data(), ctx->d_ft_acc.p, rec.size() * sizeof(float), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        std::vector<uint32_t> pl;
        slot_pixels(ctx->ft_lay, pl);
        for (uint64_t i = 0; i < N; i++) {
            float *dst = features + 12 * frame_index(pl[i], ctx->cam.width);
            for (int c = 0; c < 12; c++) dst[c] += rec[12 * i + c];
        }
    });
}

int akr_hip_render_features_device(akr_hip_ctx *ctx, const akr_feature_params *params, const akr_rect *tiles,
                                   int32_t n_tiles, float *d_features, void *stream, uint64_t *n_pixels) {
    return guard(ctx, [&] {
        if (!params || !d_features) throw std::runtime_error("null argument");
        hipStream_t st = stream_of(ctx, stream);
        const uint64_t N = ctx->render_features(*params, tiles, n_tiles, st);
        if (n_pixels) *n_pixels = N;
        if (N == 0) return;
        HIPCHK(hipMemcpyAsync(d_features, ctx->d_ft_acc.p, 12 * N * sizeof(float), hipMemcpyDeviceToDevice, st));
        ctx->mark_done(st);
    });
}

int akr_hip_denoise(akr_hip_ctx *ctx, const akr_denoise_params *params, int32_t width, int32_t height,
                    const float *radiance, const float *weight, const float *features, float *out_rgb) {
    return guard(ctx, [&] {
        if (!radiance || !weight || !features || !out_rgb) throw std::runtime_error("denoise: null argument");
        akr_hip_ctx::check_denoise(params, width, height);
        ctx->denoise_host(*params, width, height, radiance, weight, features, nullptr, 0.0f, out_rgb);
    });
}

int akr_hip_denoise_device(akr_hip_ctx *ctx, const akr_denoise_params *params, int32_t width, int32_t height,
                           const float *d_radiance, const float *d_weight, const float *d_features, float *d_out_rgb,
                           void *stream) {
    return guard(ctx, [&] {
        if (!d_radiance || !d_weight || !d_features || !d_out_rgb) throw std::runtime_error("denoise: null argument");
        akr_hip_ctx::check_denoise(params, width, height);
        hipStream_t st = stream_of(ctx, stream);
        ctx->denoise(*params, width, height, d_radiance, d_weight, d_features, nullptr, 0.0f, d_out_rgb, st);
    });
}

int akr_hip_denoise_guided(akr_hip_ctx *ctx, const akr_denoise_guided_params *params, int32_t width, int32_t height,
                           const float *radiance, const float *weight, const float *features, const float *variance,
                           float *out_rgb) {
    return guard(ctx, [&] {
        if (!radiance || !weight || !features || !variance || !out_rgb) throw std::runtime_error("denoise: null argument");
        akr_hip_ctx::check_denoise_guided(params, width, height);
        ctx->denoise_host(params->base, width, height, radiance, weight, features, variance, params->sigma_variance, out_rgb);
    });
}

int akr_hip_denoise_guided_device(akr_hip_ctx *ctx, const akr_denoise_guided_params *params, int32_t width, int32_t height,
                                  const float *d_radiance, const float *d_weight, const float *d_features,
                                  const float *d_variance, float *d_out_rgb, void *stream) {
    return guard(ctx, [&] {
        if (!d_radiance || !d_weight || !d_features || !d_variance || !d_out_rgb)
            throw std::runtime_error("denoise: null argument");
        akr_hip_ctx::check_denoise_guided(params, width, height);
        hipStream_t st = stream_of(ctx, stream);
        ctx->denoise(params->base, width, height, d_radiance, d_weight, d_features, d_variance, params->sigma_variance, d_out_rgb, st);
    });
}

int akr_hip_render_variance(akr_hip_ctx *ctx, float *variance) {
    return guard(ctx, [&] {
        if (!variance) throw std::runtime_error("null argument");
        hipStream_t st = ctx->stream;
        const uint64_t n = ctx->require_variance();
        ctx->serialize(st);  // the staging buffer is shared by every export of the context
        ctx->d_var_out.reserve(4 * n);
        const uint64_t N = ctx->variance_resolve(ctx->d_var_out.p, st);
        if (N == 0) return;
        std::vector<float> rec(4 * N);
        HIPCHK(hipMemcpyAsync(rec.data(), ctx->d_var_out.p, rec.size() * sizeof(float), hipMemcpyDeviceToHost, st));
        ctx->mark_done(st);
        HIPCHK(hipStreamSynchronize(st));
        const int W = ctx->cam.width;
        const std::vector<uint32_t> &pl = ctx->host_pixels();
        for (uint64_t k = 0; k < N; k++) {
            const uint64_t pix = frame_index(pl[k], W);
            for (int c = 0; c < 4; c++) variance[4 * pix + c] += rec[4 * k + c];
        }
    });
}

int akr_hip_render_variance_device(akr_hip_ctx *ctx, float *d_variance, void *stream, uint64_t *n_pixels) {
    return guard(ctx, [&] {
        if (!d_variance) throw std::runtime_error("null argument");
        hipStream_t st = stream_of(ctx, stream);
        const uint64_t N = ctx->variance_resolve(d_variance, st);
        if (n_pixels) *n_pixels = N;
        ctx->mark_done(st);
    });
}

int akr_hip_render_device(akr_hip_ctx *ctx, const akr_pt_params *params, const akr_rect *tiles, int32_t n_tiles,
                          float *d_radiance, float *d_weight, void *stream, uint64_t *n_pixels) {
    return guard(ctx, [&] {
        if (!params || !d_radiance || !d_weight) throw std::runtime_error("null argument");
        hipStream_t st = stream_of(ctx, stream);
        const uint64_t N = ctx->render(*params, tiles, n_tiles, st);
        if (n_pixels) *n_pixels = N;
        unpack_film(ctx, N, params->spp, d_radiance, d_weight, st, true);
        open_session(ctx->session, *params, N, params->spp, params->spp > 0);
    });
}

namespace {
// The checks of a continue of `spp` samples for every slot
void check_continue(const akr_hip_ctx *ctx, int32_t spp, const void *radiance, const void *weight) {
    if (!radiance || !weight) throw std::runtime_error("null argument");
    const Session &s = ctx->require_session();
    if (spp < 0) throw std::runtime_error("spp must be >= 0");
    check_cap(s.spp_done, spp);
}

// spp more samples for every slot on `st`, and the per-slot counts of a non-uniform session with them
void continue_all(akr_hip_ctx *ctx, int32_t spp, hipStream_t st) {
    Session &s = ctx->session;
    if (spp == 0) return;
    ctx->render(session_params(s, spp), nullptr, 0, st, true);
    if (!s.uniform) launch_count_add(ctx->d_count.p, nullptr, (uint32_t)s.n, (uint32_t)spp, st);
    advance_all(s, spp);
}
}  // namespace

int akr_hip_render_continue(akr_hip_ctx *ctx, int32_t spp, float *radiance, float *weight) {
    return guard(ctx, [&] {
        check_continue(ctx, spp, radiance, weight);
        session_call(ctx, [&] {
            continue_all(ctx, spp, ctx->stream);
            const Session &s = ctx->session;
            merge_film(ctx, s.n, s.spp_done, radiance, weight, !s.uniform);
        });
    });
}

int akr_hip_render_continue_device(akr_hip_ctx *ctx, int32_t spp, float *d_radiance, float *d_weight, void *stream,
                                   uint64_t *n_pixels) {
    return guard(ctx, [&] {
        check_continue(ctx, spp, d_radiance, d_weight);
        hipStream_t st = stream_of(ctx, stream);
        session_call(ctx, [&] {
            if (spp == 0) ctx->serialize(st);
            continue_all(ctx, spp, st);
            const Session &s = ctx->session;
            if (n_pixels) *n_pixels = s.n;
            unpack_film(ctx, s.n, s.spp_done, d_radiance, d_weight, st, spp > 0, !s.uniform);
        });
    });
}

namespace {
// The checks of a masked continue, host and device form
void check_masked(const akr_hip_ctx *ctx, int32_t spp, const uint8_t *mask, uint64_t n, const void *radiance, const void *weight) {
    if (!radiance || !weight) throw std::runtime_error("null argument");
    const Session &s = ctx->require_session();
    if (spp < 0) throw std::runtime_error("spp must be >= 0");
    if (n != s.n)
        throw std::runtime_error("masked continue: the mask has " + std::to_string(n) + " bytes, the session has " +
                                 std::to_string(s.n) + " slots");
    if (n && !mask) throw std::runtime_error("null argument");
}

// spp more samples for the slots whose byte of the device mask is set
void continue_masked(akr_hip_ctx *ctx, int32_t spp, const uint8_t *d_mask, uint64_t n, hipStream_t st) {
    ctx->serialize(st);
    if (spp == 0 || n == 0) return;
    ctx->session.ad.on = false;
    const uint32_t m = ctx->compact_mask(d_mask, (uint32_t)n, st);
    ctx->render_subset(spp, m, st);
}
}  // namespace

int akr_hip_render_continue_masked(akr_hip_ctx *ctx, int32_t spp, const uint8_t *mask, uint64_t n, float *radiance,
                                   float *weight) {
    return guard(ctx, [&] {
        check_masked(ctx, spp, mask, n, radiance, weight);
        hipStream_t st = ctx->stream;
        if (n) {  // not yet rendering: a failed upload keeps the session
            ctx->serialize(st);
            ctx->d_mask.upload(mask, n, st);
        }
        session_call(ctx, [&] {
            continue_masked(ctx, spp, ctx->d_mask.p, n, st);
            const Session &s = ctx->session;
            merge_film(ctx, s.n, s.spp_done, radiance, weight, !s.uniform);
        });
    });
}

int akr_hip_render_continue_masked_device(akr_hip_ctx *ctx, int32_t spp, const uint8_t *d_mask, uint64_t n,
                                          float *d_radiance, float *d_weight, void *stream, uint64_t *n_pixels) {
    return guard(ctx, [&] {
        check_masked(ctx, spp, d_mask, n, d_radiance, d_weight);
        hipStream_t st = stream_of(ctx, stream);
        session_call(ctx, [&] {
            continue_masked(ctx, spp, d_mask, n, st);
            const Session &s = ctx->session;
            if (n_pixels) *n_pixels = s.n;
            unpack_film(ctx, s.n, s.spp_done, d_radiance, d_weight, st, spp > 0, !s.uniform);
        });
    });
}

int akr_hip_render_state_spp_range(akr_hip_ctx *ctx, int32_t *spp_min, int32_t *spp_max) {
    return guard(ctx, [&] {
        const Session &s = ctx->require_session();
        if (spp_min) *spp_min = s.uniform ? s.spp_done : s.spp_min;
        if (spp_max) *spp_max = s.spp_done;
    });
}

namespace {
void check_adaptive(const akr_pt_params *params, const akr_adaptive_params *ap) {
    if (!params || !ap) throw std::runtime_error("null argument");
    if (params->spp < 0 || params->max_depth < 0) throw std::runtime_error("spp and max_depth must be >= 0");
    if (ap->min_spp < 1) throw std::runtime_error("adaptive render: min_spp must be >= 1");
    if (ap->pass_spp < 0) throw std::runtime_error("adaptive render: pass_spp must be >= 0");
    if (!(ap->threshold >= 0.0f)) throw std::runtime_error("adaptive render: threshold must be >= 0 and not NaN");
    if (params->spp > kSessionSppCap) throw std::runtime_error("adaptive render: the cap exceeds 2^24 samples");
}

// The adaptive loop in two pieces, both on `st`.  adaptive_begin: min_spp for every
// slot (this starts the session) and the snapshot.  adaptive_step: one pass over the active strips and
// its test.  The run's state lives in the session (Session::ad); ad.more says whether a step remains.
uint64_t adaptive_begin(akr_hip_ctx *ctx, const akr_pt_params &params, const akr_adaptive_params &ap,
                        const akr_rect *tiles, int32_t n_tiles, hipStream_t st) {
    const int32_t cap = params.spp;
    akr_pt_params p0 = params;
    p0.spp = std::min(cap, ap.min_spp);
    const uint64_t N = ctx->render(p0, tiles, n_tiles, st);
    open_session(ctx->session, p0, N, p0.spp, p0.spp > 0);
    adaptive_open(ctx->session, cap, ap);
    const uint64_t n_strips = ctx->session.ad.info.strips;
    if (ctx->session.ad.more) {
        // the first pass is complete on the host before its film is copied (as merge_film waits before
        // its read-back); then the snapshot, every strip active, every slot masked
        ctx->host_join();
        HIPCHK(hipStreamSynchronize(st));
        ctx->check_fault();
        ctx->d_prev.reserve(N);
        ctx->d_mask.reserve(N);
        ctx->d_strip_active.reserve(n_strips);
        ctx->d_strip_err.reserve(n_strips);
        HIPCHK(hipMemcpyAsync(ctx->d_prev.p, ctx->d_film.p, N * sizeof(float4), hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemsetAsync(ctx->d_mask.p, 1, N, st));
        HIPCHK(hipMemsetAsync(ctx->d_strip_active.p, 1, n_strips, st));
        HIPCHK(hipMemsetAsync(ctx->d_strip_err.p, 0, n_strips * sizeof(float), st));
    }
    return N;
}

void adaptive_step(akr_hip_ctx *ctx, hipStream_t st) {
    Session &s = ctx->session;
    const Session::Adaptive &ad = s.ad;
    if (!ad.more) return;
    const uint32_t N = (uint32_t)s.n;
    const int32_t step = adaptive_pass_spp(ad);
    ctx->render_subset(step, ad.m, st, false);
    ctx->timed("adaptive_test", st, [&] {
        launch_adaptive_test(ctx->d_film.p, ctx->d_prev.p, N, ad.threshold, ctx->d_strip_err.p, ctx->d_strip_active.p,
                             ctx->d_mask.p, st);
    });
    HIPCHK(hipGetLastError());
    adaptive_advance(s, step, ctx->compact_mask(ctx->d_mask.p, N, st));  // the pass's one host read: the active count
}

uint64_t render_adaptive(akr_hip_ctx *ctx, const akr_pt_params &params, const akr_adaptive_params &ap,
                         const akr_rect *tiles, int32_t n_tiles, hipStream_t st, akr_adaptive_info *info) {
    const uint64_t N = adaptive_begin(ctx, params, ap, tiles, n_tiles, st);
    while (ctx->session.ad.more) adaptive_step(ctx, st);
    if (info) *info = ctx->session.ad.info;
    return N;
}
}  // namespace

int akr_hip_adaptive_begin(akr_hip_ctx *ctx, const akr_pt_params *params, const akr_adaptive_params *ap,
                           const akr_rect *tiles, int32_t n_tiles, akr_adaptive_info *info, int32_t *more) {
    return guard(ctx, [&] {
        check_adaptive(params, ap);
        hipStream_t st = ctx->stream;
        session_call(ctx, [&] {
            adaptive_begin(ctx, *params, *ap, tiles, n_tiles, st);
            const Session &s = ctx->session;
            ctx->verify_weights(st, s.n, s.spp_done);
            ctx->mark_done(st);
        });
        if (info) *info = ctx->session.ad.info;
        if (more) *more = ctx->session.ad.more ? 1 : 0;
    });
}

int akr_hip_adaptive_step(akr_hip_ctx *ctx, akr_adaptive_info *info, int32_t *more) {
    return guard(ctx, [&] {
        require_adaptive(ctx->session);
        hipStream_t st = ctx->stream;
        session_call(ctx, [&] {
            ctx->serialize(st);
            adaptive_step(ctx, st);
            const Session &s = ctx->session;
            ctx->verify_weights(st, s.n, s.spp_done, !s.uniform);
            ctx->mark_done(st);
        });
        if (info) *info = ctx->session.ad.info;
        if (more) *more = ctx->session.ad.more ? 1 : 0;
    });
}

int akr_hip_render_adaptive(akr_hip_ctx *ctx, const akr_pt_params *params, const akr_adaptive_params *ap,
                            const akr_rect *tiles, int32_t n_tiles, float *radiance, float *weight,
                            akr_adaptive_info *info) {
    return guard(ctx, [&] {
        check_adaptive(params, ap);
        if (!radiance || !weight) throw std::runtime_error("null argument");
        session_call(ctx, [&] {
            render_adaptive(ctx, *params, *ap, tiles, n_tiles, ctx->stream, info);
            const Session &s = ctx->session;
            merge_film(ctx, s.n, s.spp_done, radiance, weight, !s.uniform);
        });
    });
}

int akr_hip_render_adaptive_device(akr_hip_ctx *ctx, const akr_pt_params *params, const akr_adaptive_params *ap,
                                   const akr_rect *tiles, int32_t n_tiles, float *d_radiance, float *d_weight,
                                   void *stream, uint64_t *n_pixels, akr_adaptive_info *info) {
    return guard(ctx, [&] {
        check_adaptive(params, ap);
        if (!d_radiance || !d_weight) throw std::runtime_error("null argument");
        hipStream_t st = stream_of(ctx, stream);
        session_call(ctx, [&] {
            const uint64_t N = render_adaptive(ctx, *params, *ap, tiles, n_tiles, st, info);
            if (n_pixels) *n_pixels = N;
            const Session &s = ctx->session;
            unpack_film(ctx, s.n, s.spp_done, d_radiance, d_weight, st, true, !s.uniform);
        });
    });
}

int akr_hip_adaptive_error(akr_hip_ctx *ctx, float *strip_error, uint8_t *strip_active, uint64_t n_strips) {
    return guard(ctx, [&] {
        const Session &s = ctx->require_session();
        if (s.n_strips == 0) throw std::runtime_error("adaptive error: the session ran no convergence test");
        if (n_strips != s.n_strips)
            throw std::runtime_error("adaptive error: n_strips is " + std::to_string(n_strips) + ", the session has " +
                                     std::to_string(s.n_strips) + " strips");
        if (!strip_error || !strip_active) throw std::runtime_error("null argument");
        hipStream_t st = ctx->stream;
        ctx->serialize(st);
        HIPCHK(hipMemcpyAsync(strip_error, ctx->d_strip_err.p, n_strips * sizeof(float), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(strip_active, ctx->d_strip_active.p, n_strips, hipMemcpyDeviceToHost, st));
        ctx->mark_done(st);
        HIPCHK(hipStreamSynchronize(st));
    });
}

int akr_hip_render_state_info(akr_hip_ctx *ctx, akr_render_state_info *info) {
    return guard(ctx, [&] {
        if (!info) throw std::runtime_error("null argument");
        const Session &s = ctx->require_session();
        *info = akr_render_state_info{};
        info->n_pixels = s.n;
        info->spp_done = s.spp_done;
        info->max_depth = s.max_depth;
        info->ray_clamp = s.ray_clamp;
        info->flags = s.flags;
        info->width = ctx->cam.width;
        info->height = ctx->cam.height;
        info->n_tiles = (int32_t)ctx->lay.tiles.size();
    });
}

int akr_hip_render_state_export(akr_hip_ctx *ctx, uint32_t *sampler, float *film, uint64_t n) {
    return guard(ctx, [&] {
        const Session &s = ctx->require_session();
        if (n != s.n) throw std::runtime_error("render state export: n is " + std::to_string(n) + ", the session has " +
                                               std::to_string(s.n) + " slots");
        if (n == 0) return;
        if (!sampler || !film) throw std::runtime_error("null argument");
        hipStream_t st = ctx->stream;
        ctx->serialize(st);
        ctx->host_join();
        if (s.seeded) {
            HIPCHK(hipMemcpyAsync(sampler, ctx->d_seed.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        } else {  // no sample drawn yet: the slots' start states
            const int W = ctx->cam.width;
            const std::vector<uint32_t> &pl = ctx->host_pixels();
            for (uint64_t k = 0; k < n; k++) sampler[k] = (uint32_t)frame_index(pl[k], W);
        }
        HIPCHK(hipMemcpyAsync(film, ctx->d_film.p, n * sizeof(float4), hipMemcpyDeviceToHost, st));
        ctx->mark_done(st);
        HIPCHK(hipStreamSynchronize(st));
    });
}

int akr_hip_render_state_import(akr_hip_ctx *ctx, const akr_pt_params *params, const akr_rect *tiles, int32_t n_tiles,
                                const uint32_t *sampler, const float *film, uint64_t n) {
    return guard(ctx, [&] {
        if (!params) throw std::runtime_error("null argument");
        if (params->spp < 0 || params->max_depth < 0) throw std::runtime_error("spp and max_depth must be >= 0");
        if (params->max_depth > 1000) throw std::runtime_error("max_depth too large");
        if (params->spp > kSessionSppCap) throw std::runtime_error("render state import: spp exceeds 2^24");
        if (n && (!sampler || !film)) throw std::runtime_error("null argument");
        if (!ctx->cam_set) throw std::runtime_error("camera not set (call akr_hip_set_camera)");
        if (n_tiles < 0 || (n_tiles > 0 && !tiles)) throw std::runtime_error("invalid tile list");
        // validated before anything of the context changes: a refused import keeps the current session
        const uint64_t want = layout_tiles(tiles, n_tiles, ctx->cam.width, ctx->cam.height, "render call").n;
        if (n != want) throw std::runtime_error("render state import: n is " + std::to_string(n) + ", the tile list has " +
                                                std::to_string(want) + " pixels");
        for (uint64_t k = 0; k < n; k++)
            if (film[4 * k + 3] != (float)params->spp)
                throw std::runtime_error("render state import: slot " + std::to_string(k) + " holds weight " +
                                         std::to_string(film[4 * k + 3]) + ", not spp " + std::to_string(params->spp));
        hipStream_t st = ctx->stream;
        const uint64_t N = ctx->setup_pixels(tiles, n_tiles, 0, st);  // the slots, as a render lays them out
        if (N != n) throw std::runtime_error("render state import: slot count changed");
        if (N) {
            HIPCHK(hipMemcpyAsync(ctx->d_seed.p, sampler, N * sizeof(uint32_t), hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(ctx->d_film.p, film, N * sizeof(float4), hipMemcpyHostToDevice, st));
        }
        // the tracker takes the imported film as one batch: P = the film, K = 1 where the weight is positive
        ctx->variance_begin(N, st);
        ctx->variance_update(N, st);
        ctx->mis_begin(N, st);
        ctx->mark_done(st);
        HIPCHK(hipStreamSynchronize(st));  // the caller's arrays are free again
        ctx->probe_ok = false;
        ctx->probe_n = 0;
        open_session(ctx->session, *params, N, params->spp, true);
    });
}

struct akr_bvh_host {
    BvhOutput out;
    Bvh4Output wide;
    bool wide_built = false;
    int n_threads = 0;  // the build's thread count, used by the wide collapse too
    int collapse = AKR_COLLAPSE_SAH;
};

int akr_bvh_host_build(const float *vertices, uint64_t n_vertices, const int32_t *indices, uint64_t n_triangles,
                       const akr_build_params *params, akr_bvh_host **out, akr_accel_info *info) {
    if (!out) return -1;
    *out = nullptr;
    try {
        for (uint64_t i = 0; i < 3 * n_triangles; i++)
            if (indices[i] < 0 || (uint64_t)indices[i] >= n_vertices) return -1;
        akr_build_params p{};
        p.max_leaf_size = 4;
        p.n_bins = 32;
        p.traversal_cost = 1.0f;
        p.intersect_cost = 4.0f;
        if (params) p = *params;
        std::unique_ptr<akr_bvh_host> h(new akr_bvh_host());
        h->n_threads = p.n_threads;
        if (p.wide_collapse != AKR_COLLAPSE_SAH && p.wide_collapse != AKR_COLLAPSE_BALANCED) return -1;
        h->collapse = p.wide_collapse;
        BvhInput in{vertices, indices, n_triangles};
        build_bvh(in, p, h->out);
        if (info) {
            info->n_nodes = h->out.nodes.size();
            info->n_tris = h->out.tris.size();
            info->max_depth = h->out.max_depth;
            info->max_leaf = h->out.max_leaf;
            info->build_ms = h->out.build_ms;
            info->sah_cost = h->out.sah_cost;
        }
        *out = h.release();
        return 0;
    } catch (...) {
        return -1;
    }
}
const void *akr_bvh_host_nodes(const akr_bvh_host *h) { return h ? h->out.nodes.data() : nullptr; }
const void *akr_bvh_host_tris(const akr_bvh_host *h) { return h ? h->out.tris.data() : nullptr; }
void akr_bvh_host_free(akr_bvh_host *h) { delete h; }

int akr_bvh_validate(const void *nodes, uint64_t n_nodes, const void *tris, uint64_t n_tris, uint64_t n_scene_tris,
                     int32_t *max_depth) {
    try {
        if (!nodes || (n_tris && !tris)) return -1;
        int max_leaf = 0;
        const int d = validate_bvh2(reinterpret_cast<const akr_bvh_node *>(nodes), n_nodes,
                                    reinterpret_cast<const akr_bvh_tri *>(tris), n_tris, n_scene_tris, max_leaf);
        if (max_depth) *max_depth = d;
        return 0;
    } catch (...) {
        return -1;
    }
}

int akr_bvh_host_wide(akr_bvh_host *h, uint64_t *n_nodes, uint64_t *n_leaves, uint32_t *root_ref) {
    if (!h) return -1;
    try {
        if (!h->wide_built) {
            build_bvh4(h->out.nodes, h->wide, h->n_threads, h->collapse);
            h->wide_built = true;
        }
        if (n_nodes) *n_nodes = h->wide.nodes.size();
        if (n_leaves) *n_leaves = h->wide.leaves.size();
        if (root_ref) *root_ref = h->wide.root_ref;
        return 0;
    } catch (...) {
        return -1;
    }
}
const void *akr_bvh_host_wide_nodes(const akr_bvh_host *h) { return h ? h->wide.nodes.data() : nullptr; }
const void *akr_bvh_host_wide_leaves(const akr_bvh_host *h) { return h ? h->wide.leaves.data() : nullptr; }

int akr_hip_ray_steps(akr_hip_ctx *ctx, uint32_t *out, uint64_t n) {
    return guard(ctx, [&] {
        if (!ctx->opt.ray_steps || n > ctx->n_steps) throw std::runtime_error("no per-ray steps recorded for that many rays");
        if (n == 0) return;
        if (!out) throw std::runtime_error("null output");
        HIPCHK(hipMemcpyAsync(out, ctx->d_steps.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    });
}

int akr_hip_kernel_stats(akr_hip_ctx *ctx, akr_kernel_stat *out, int32_t max_n, int32_t *n) {
    return guard(ctx, [&] {
        ctx->flush_stats();
        int32_t k = 0;
        for (auto &kv : ctx->stat) {
            if (k < max_n && out) {
                akr_kernel_stat &s = out[k];
                std::memset(&s, 0, sizeof(s));
                std::strncpy(s.name, kv.first.c_str(), sizeof(s.name) - 1);
                s.launches = kv.second.launches;
                s.total_ms = kv.second.total;
                s.min_ms = kv.second.launches ? kv.second.mn : 0;
                s.max_ms = kv.second.mx;
            }
            k++;
        }
        if (n) *n = k;
    });
}

int akr_hip_trace_counts(akr_hip_ctx *ctx, akr_trace_counts *out) {
    return guard(ctx, [&] {
        std::memset(out, 0, sizeof(*out));
        if (!ctx->d_counters.p) return;
        HIPCHK(hipDeviceSynchronize());
        TraceCounters c[3];
        HIPCHK(hipMemcpy(c, ctx->d_counters.p, sizeof(c), hipMemcpyDeviceToHost));
        out->rays = c[0].rays + c[1].rays + c[2].rays;
        out->box_tests = c[0].box + c[1].box + c[2].box;
        out->tri_tests = c[0].tri + c[1].tri + c[2].tri;
        out->closest_rays = c[0].rays;
        out->shadow_rays = c[1].rays + c[2].rays;
        for (int m = 0; m < 3; m++) {
            out->per_mode[m][0] = c[m].rays;
            out->per_mode[m][1] = c[m].box;
            out->per_mode[m][2] = c[m].tri;
            out->lane_slots[m][0] = c[m].slots_trav;
            out->lane_slots[m][1] = c[m].slots_leaf;
            out->lane_slots[m][2] = c[m].slots_tri;
            out->lane_slots[m][3] = c[m].visits;
            out->deep_rays[m] = c[m].deep;
            out->leaf_tests[m] = c[m].leaves;
        }
    });
}

int akr_hip_path_profile(akr_hip_ctx *ctx, uint64_t *out, int32_t n) {
    return guard(ctx, [&] {
        if (!out || n < 0) throw std::runtime_error("null output");
        PathProfile q{};
        if (ctx->d_pprof.p) HIPCHK(hipMemcpy(&q, ctx->d_pprof.p, sizeof(q), hipMemcpyDeviceToHost));
        uint64_t v[] = {q.waves, q.outer, q.procs, q.trav_iters, q.t_proc, q.t_trav, q.t_leaf, q.t_total, q.t_max,
                        q.lanes_proc, q.t_shade, q.spec_started, q.spec_aborted, q.tv_issue, q.tv_wait,
                        q.tv_comp, q.tl_issue, q.tl_wait, q.tl_comp, q.tp_park, q.tp_next, q.tp_begin, q.tp_load,
                        q.leaf_phases, q.leaf_holders, 0, 0, 0,
                        // out[28..34]: k_path's pop site and push (PathProfile)
                        q.pop_iters, q.pop_rounds, q.pop_lane_rounds, q.pop_lanes, q.push_iters, q.push_slow,
                        q.push_would_fit};
        // out[25..27]: distinct 128-B lines of the wide nodes, the leaf blob and the shading records the
        // last render with count_lines read (k_path)
        if (n > 25 && ctx->opt.count_lines && ctx->d_lines.p && ctx->lines_span[3]) {
            std::vector<uint32_t> m(ctx->lines_span[3] / 32 + 1);
            HIPCHK(hipMemcpy(m.data(), ctx->d_lines.p, m.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
            for (int r = 0; r < 3; r++)
                for (uint32_t b = ctx->lines_span[r]; b < ctx->lines_span[r + 1]; b++)
                    v[25 + r] += (m[b >> 5] >> (b & 31u)) & 1u;
        }
        for (int32_t k = 0; k < n && k < (int32_t)(sizeof(v) / sizeof(v[0])); k++) out[k] = v[k];
    });
}

int akr_hip_render_info(akr_hip_ctx *ctx, int32_t *lanes, int32_t *passes) {
    return guard(ctx, [&] {
        if (lanes) *lanes = 1;  // one sample per pixel in flight (the lookahead lanes are gone)
        if (passes) *passes = ctx->last_passes;
    });
}

int akr_hip_render_form(akr_hip_ctx *ctx, int32_t *form, int32_t *ordered) {
    return guard(ctx, [&] {
        ctx->resolve_form();
        if (form) *form = ctx->last_form;
        if (ordered) *ordered = ctx->last_ordered;
    });
}

int akr_hip_render_shading(akr_hip_ctx *ctx, int32_t *shading) {
    return guard(ctx, [&] {
        if (shading) *shading = ctx->last_shading;
    });
}

int akr_hip_render_form_inputs(akr_hip_ctx *ctx, int64_t *pixels_per_lane_x1000, int64_t *pilot_rays,
                               int64_t *pilot_steps) {
    return guard(ctx, [&] {
        ctx->resolve_form();
        if (pixels_per_lane_x1000) *pixels_per_lane_x1000 = ctx->last_ppl1000;
        if (pilot_rays) *pilot_rays = ctx->last_pilot_rays;
        if (pilot_steps) *pilot_steps = ctx->last_pilot_steps;
    });
}

int akr_hip_reset_stats(akr_hip_ctx *ctx) {
    return guard(ctx, [&] {
        HIPCHK(hipDeviceSynchronize());
        ctx->flush_stats();
        ctx->stat.clear();
        if (ctx->d_counters.p) HIPCHK(hipMemset(ctx->d_counters.p, 0, 3 * sizeof(TraceCounters)));
        if (ctx->d_pprof.p) HIPCHK(hipMemset(ctx->d_pprof.p, 0, sizeof(PathProfile)));
    });
}

int akr_hip_synchronize(akr_hip_ctx *ctx) {
    return guard(ctx, [&] {
        HIPCHK(hipStreamSynchronize(ctx->stream));
        HIPCHK(hipDeviceSynchronize());
        ctx->check_fault();
    });
}

int akr_hip_pixel_probe(akr_hip_ctx *ctx, akr_pixel_probe *out, uint64_t n) {
    return guard(ctx, [&] {
        if (!ctx->probe_ok || n > ctx->probe_n)
            throw std::runtime_error("no pixel probe recorded for that many slots (option pixel_probe, path renders only)");
        if (n == 0) return;
        if (!out) throw std::runtime_error("null output");
        static_assert(sizeof(akr_pixel_probe) == sizeof(uint4), "akr_pixel_probe layout");
        ctx->host_join();
        HIPCHK(hipStreamSynchronize(ctx->stream));
        HIPCHK(hipMemcpyAsync(out, ctx->d_probe.p, n * sizeof(uint4), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    });
}

}  // extern "C"
