// denoise.hip — edge-avoiding a-trous filter of the film for gfx950 (the definition is
// the comment of akr_hip_denoise in include/akr_hip.h, and every line below follows its operation order:
// f32, unfused (the library is built with -ffp-contract=off), left to right).
//
// Three kernels over frame-ordered buffers of n = W * H pixels:
//   k_denoise_prep    film + feature sums -> the static guide record (3 float4: unit normal | depth,
//                     position | 0, albedo | 0) and I0 = (demodulated mean colour | state)
//   k_denoise_atrous  one 5x5 iteration at stride `step`, I_in -> I_out (ping-pong; the guide is read only)
//   k_denoise_finish  remodulates the last I into out_rgb
// The state in I.w is kInvalid (weight not > 0), kNoHits or kHits; an iteration copies it through.
//
// k_denoise_atrous maps a wave to 64 consecutive pixels of one row (64 x 4 workgroup), so every tap of a
// wave is one contiguous 1-KiB float4 read at every stride.  A tap's address is formed only after its
// pixel has been found inside the frame.
//
// Below them: the variance-guided iteration k_denoise_atrous_guided with its
// k_denoise_prep_variance, and the session's variance tracker k_variance_update / k_variance_resolve.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "akr_math.h"
#include "kernels.h"

namespace akr {

namespace {
constexpr float kInvalid = 0.0f, kNoHits = 1.0f, kHits = 2.0f;
constexpr int kDnX = 64, kDnY = 4;

__device__ __forceinline__ bool finite3(float4 v) {
    return fabsf(v.x) < kInf && fabsf(v.y) < kInf && fabsf(v.z) < kInf;  // false for NaN
}
// the per-channel demodulation factor
__device__ __forceinline__ float demod(bool on, float a) { return (on && a > 1e-3f) ? a : 1.0f; }
}  // namespace

__global__ __launch_bounds__(kBlock) void k_denoise_prep(const float *radiance, const float *weight, const float *features,
                                                         uint32_t n, int32_t demodulate, float4 *guide, float4 *I) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float w = weight[i];
    const bool valid = w > 0.0f;
    V3 c = v3(0.0f, 0.0f, 0.0f);
    if (valid) c = v3(radiance[3 * (size_t)i] / w, radiance[3 * (size_t)i + 1] / w, radiance[3 * (size_t)i + 2] / w);
    const float *f = features + 12 * (size_t)i;  // float loads: the caller's pointer need not be 16-B aligned
    const float4 f0 = make_float4(f[0], f[1], f[2], f[3]), f1 = make_float4(f[4], f[5], f[6], f[7]),
                 f2 = make_float4(f[8], f[9], f[10], f[11]);
    const float h = f0.w;
    V3 a = v3(0.0f, 0.0f, 0.0f), nn = a, x = a;
    float t = 0.0f;
    if (h > 0.0f) {
        a = v3(f0.x / h, f0.y / h, f0.z / h);
        nn = v3(f1.x / h, f1.y / h, f1.z / h);
        t = f1.w / h;
        x = v3(f2.x / h, f2.y / h, f2.z / h);
    }
    const float l = length(nn);
    const V3 nh = l > 0.0f ? divs(nn, l) : v3(0.0f, 0.0f, 0.0f);
    const bool dm = demodulate != 0;
    guide[3 * (size_t)i] = make_float4(nh.x, nh.y, nh.z, t);
    guide[3 * (size_t)i + 1] = make_float4(x.x, x.y, x.z, 0.0f);
    guide[3 * (size_t)i + 2] = make_float4(a.x, a.y, a.z, 0.0f);
    I[i] = make_float4(c.x / demod(dm, a.x), c.y / demod(dm, a.y), c.z / demod(dm, a.z),
                       !valid ? kInvalid : (h > 0.0f ? kHits : kNoHits));
}

__global__ __launch_bounds__(kDnX * kDnY) void k_denoise_atrous(DenoiseArgs a) {
    const int x = (int)(blockIdx.x * kDnX + threadIdx.x), y = (int)(blockIdx.y * kDnY + threadIdx.y);
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
    const float4 Ip = a.in[p];
    if (Ip.w == kInvalid) {
        a.out[p] = make_float4(0.0f, 0.0f, 0.0f, kInvalid);
        return;
    }
    if (!finite3(Ip)) {  // a non-finite pixel stays as it is (and no neighbour takes it as a tap)
        a.out[p] = Ip;
        return;
    }
    const float4 g0 = a.guide[3 * p], g1 = a.guide[3 * p + 1], g2 = a.guide[3 * p + 2];
    const V3 nh_p = v3(g0.x, g0.y, g0.z), x_p = v3(g1.x, g1.y, g1.z);
    const float zden = a.sigma_depth * g0.w;
    const bool hits_p = Ip.w == kHits;
    const float hk[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    float nr = 0.0f, ng = 0.0f, nb = 0.0f, den = 0.0f;
    for (int j = 0; j < 5; j++) {
        const int qy = y + (j - 2) * a.step;
        for (int k = 0; k < 5; k++) {
            const int qx = x + (k - 2) * a.step;
            if (qx < 0 || qx >= a.width || qy < 0 || qy >= a.height) continue;  // before any address is formed
            const size_t q = (size_t)qy * (size_t)a.width + (size_t)qx;
            const float4 Iq = a.in[q];
            if (Iq.w == kInvalid || !finite3(Iq)) continue;
            float g = 1.0f, wc = 1.0f;
            if (!(j == 2 && k == 2)) {
                const bool hits_q = Iq.w == kHits;
                if (hits_p && hits_q) {
                    const float4 q0 = a.guide[3 * q], q1 = a.guide[3 * q + 1], q2 = a.guide[3 * q + 2];
                    float wn = rmax(dot(nh_p, v3(q0.x, q0.y, q0.z)), 0.0f);
                    for (int s = 0; s < a.squarings; s++) wn = wn * wn;
                    const float wz = rmax(1.0f - fabsf(dot(nh_p, sub(v3(q1.x, q1.y, q1.z), x_p))) / zden, 0.0f);
                    float da = fabsf(q2.x - g2.x);
                    da += fabsf(q2.y - g2.y);
                    da += fabsf(q2.z - g2.z);
                    const float wa = rmax(1.0f - da / a.sigma_albedo, 0.0f);
                    g = wn * wz * wa;
                } else if (hits_p || hits_q) {
                    g = 0.0f;
                }
                if (a.color_stop) {
                    const V3 d = v3(Iq.x - Ip.x, Iq.y - Ip.y, Iq.z - Ip.z);
                    wc = 1.0f / (1.0f + dot(d, d) / a.sc2);
                }
            }
            const float w = ((hk[j] * hk[k]) * g) * wc;
            nr += w * Iq.x;
            ng += w * Iq.y;
            nb += w * Iq.z;
            den += w;
        }
    }
    a.out[p] = den > 0.0f ? make_float4(nr / den, ng / den, nb / den, Ip.w) : Ip;
}

__global__ __launch_bounds__(kBlock) void k_denoise_finish(const float4 *guide, const float4 *I, uint32_t n,
                                                           int32_t demodulate, float *out_rgb) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float4 v = I[i];
    float r = 0.0f, g = 0.0f, b = 0.0f;
    if (v.w != kInvalid) {
        const float4 a = guide[3 * (size_t)i + 2];
        const bool dm = demodulate != 0;
        r = v.x * demod(dm, a.x);
        g = v.y * demod(dm, a.y);
        b = v.z * demod(dm, a.z);
    }
    out_rgb[3 * (size_t)i] = r;
    out_rgb[3 * (size_t)i + 1] = g;
    out_rgb[3 * (size_t)i + 2] = b;
}

// ---- the variance-guided filter (the definition is the comment of akr_hip_denoise_guided).
// The variance travels in a ping-pong pair of its own, V = (variance of the demodulated mean | hv as 1 or 0),
// so the records of the kernels above are what they were.

// V0 from the frame-ordered (vr, vg, vb, K) of the tracker, after k_denoise_prep has written guide and I0
__global__ __launch_bounds__(kBlock) void k_denoise_prep_variance(const float *variance, const float4 *guide, const float4 *I,
                                                                  uint32_t n, int32_t demodulate, float4 *V) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float *v = variance + 4 * (size_t)i;  // float loads: the caller's pointer need not be 16-B aligned
    const float4 var = make_float4(v[0], v[1], v[2], v[3]);
    const bool hv = I[i].w != kInvalid && var.w >= 2.0f && finite3(var);
    float4 out = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (hv) {
        const float4 a = guide[3 * (size_t)i + 2];
        const bool dm = demodulate != 0;
        const float mx = demod(dm, a.x), my = demod(dm, a.y), mz = demod(dm, a.z);
        out = make_float4(var.x / (mx * mx), var.y / (my * my), var.z / (mz * mz), 1.0f);
    }
    V[i] = out;
}

// One guided iteration: k_denoise_atrous with the 3x3 prefilter of V at stride 1, the variance colour stop of
// pixels with hv, and the propagation of V through the tap weights.  Same wave shape: 64 consecutive pixels of
// one row, every tap of I, V and the guide a contiguous read; an address is formed only inside the frame.
__global__ __launch_bounds__(kDnX * kDnY) void k_denoise_atrous_guided(DenoiseGuidedArgs ga) {
    const DenoiseArgs &a = ga.d;
    const int x = (int)(blockIdx.x * kDnX + threadIdx.x), y = (int)(blockIdx.y * kDnY + threadIdx.y);
    if (x >= a.width || y >= a.height) return;
    const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
    const float4 Ip = a.in[p];
    const float4 Vp = ga.vin[p];
    if (Ip.w == kInvalid) {
        a.out[p] = make_float4(0.0f, 0.0f, 0.0f, kInvalid);
        ga.vout[p] = Vp;
        return;
    }
    if (!finite3(Ip)) {
        a.out[p] = Ip;
        ga.vout[p] = Vp;
        return;
    }
    const bool hv_p = Vp.w != 0.0f;
    float Gr = Vp.x, Gg = Vp.y, Gb = Vp.z;
    if (hv_p) {
        const float gk[3] = {1.0f / 4.0f, 1.0f / 2.0f, 1.0f / 4.0f};
        float gr = 0.0f, gg = 0.0f, gb = 0.0f, gd = 0.0f;
        for (int j = 0; j < 3; j++) {
            const int qy = y + (j - 1);
            for (int k = 0; k < 3; k++) {
                const int qx = x + (k - 1);
                if (qx < 0 || qx >= a.width || qy < 0 || qy >= a.height) continue;
                const float4 Vq = ga.vin[(size_t)qy * (size_t)a.width + (size_t)qx];
                if (Vq.w == 0.0f) continue;
                const float gw = gk[j] * gk[k];
                gr += gw * Vq.x;
                gg += gw * Vq.y;
                gb += gw * Vq.z;
                gd += gw;
            }
        }
        if (gd > 0.0f) {
            Gr = gr / gd;
            Gg = gg / gd;
            Gb = gb / gd;
        }
    }
    const float4 g0 = a.guide[3 * p], g1 = a.guide[3 * p + 1], g2 = a.guide[3 * p + 2];
    const V3 nh_p = v3(g0.x, g0.y, g0.z), x_p = v3(g1.x, g1.y, g1.z);
    const float zden = a.sigma_depth * g0.w;
    const bool hits_p = Ip.w == kHits;
    const float hk[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    float nr = 0.0f, ng = 0.0f, nb = 0.0f, den = 0.0f;
    float vr = 0.0f, vg = 0.0f, vb = 0.0f;
    for (int j = 0; j < 5; j++) {
        const int qy = y + (j - 2) * a.step;
        for (int k = 0; k < 5; k++) {
            const int qx = x + (k - 2) * a.step;
            if (qx < 0 || qx >= a.width || qy < 0 || qy >= a.height) continue;  // before any address is formed
            const size_t q = (size_t)qy * (size_t)a.width + (size_t)qx;
            const float4 Iq = a.in[q];
            if (Iq.w == kInvalid || !finite3(Iq)) continue;
            float g = 1.0f, wc = 1.0f;
            if (!(j == 2 && k == 2)) {
                const bool hits_q = Iq.w == kHits;
                if (hits_p && hits_q) {
                    const float4 q0 = a.guide[3 * q], q1 = a.guide[3 * q + 1], q2 = a.guide[3 * q + 2];
                    float wn = rmax(dot(nh_p, v3(q0.x, q0.y, q0.z)), 0.0f);
                    for (int s = 0; s < a.squarings; s++) wn = wn * wn;
                    const float wz = rmax(1.0f - fabsf(dot(nh_p, sub(v3(q1.x, q1.y, q1.z), x_p))) / zden, 0.0f);
                    float da = fabsf(q2.x - g2.x);
                    da += fabsf(q2.y - g2.y);
                    da += fabsf(q2.z - g2.z);
                    const float wa = rmax(1.0f - da / a.sigma_albedo, 0.0f);
                    g = wn * wz * wa;
                } else if (hits_p || hits_q) {
                    g = 0.0f;
                }
                const V3 d = v3(Iq.x - Ip.x, Iq.y - Ip.y, Iq.z - Ip.z);
                if (hv_p) {
                    const float er = (d.x * d.x) / (Gr + 1e-8f), eg = (d.y * d.y) / (Gg + 1e-8f),
                                eb = (d.z * d.z) / (Gb + 1e-8f);
                    const float r = ((er + eg) + eb) / ga.sv3;
                    wc = 1.0f / (1.0f + r);
                } else if (a.color_stop) {
                    wc = 1.0f / (1.0f + dot(d, d) / a.sc2);
                }
            }
            const float w = ((hk[j] * hk[k]) * g) * wc;
            nr += w * Iq.x;
            ng += w * Iq.y;
            nb += w * Iq.z;
            den += w;
            const float4 Vq = ga.vin[q];
            if (Vq.w != 0.0f) {  // a tap without hv carries no variance
                const float w2 = w * w;
                vr += w2 * Vq.x;
                vg += w2 * Vq.y;
                vb += w2 * Vq.z;
            }
        }
    }
    if (den > 0.0f) {
        const float d2 = den * den;
        a.out[p] = make_float4(nr / den, ng / den, nb / den, Ip.w);
        ga.vout[p] = make_float4(vr / d2, vg / d2, vb / d2, Vp.w);
    } else {
        a.out[p] = Ip;
        ga.vout[p] = Vp;
    }
}

// ---- the film variance tracker (the definition is the comment of akr_hip_render_variance).
// One thread per film slot, float4 records, nothing shared between threads.

// West's weighted incremental update on the batch means: the slots whose weight grew since their snapshot
// P take (F - P) as one batch of n = F.w - P.w samples; M = (M2r, M2g, M2b, K)
__global__ __launch_bounds__(kBlock) void k_variance_update(const float4 *film, uint32_t n, float4 *P, float4 *M) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float4 F = film[i], Pv = P[i];
    const float nb = F.w - Pv.w;
    if (!(nb > 0.0f)) return;
    float4 m = M[i];
    if (Pv.w > 0.0f) {
        const float s = (Pv.w * nb) / F.w;
        const float dr = (F.x - Pv.x) / nb - Pv.x / Pv.w, dg = (F.y - Pv.y) / nb - Pv.y / Pv.w,
                    db = (F.z - Pv.z) / nb - Pv.z / Pv.w;
        m.x = m.x + (dr * dr) * s;
        m.y = m.y + (dg * dg) * s;
        m.z = m.z + (db * db) * s;
    }
    m.w = m.w + 1.0f;
    M[i] = m;
    P[i] = F;
}

// (vr, vg, vb, K) per slot: the variance of the slot's mean for K >= 2, else 0; float stores (the caller's
// pointer need not be 16-B aligned)
__global__ __launch_bounds__(kBlock) void k_variance_resolve(const float4 *film, const float4 *M, uint32_t n, float *out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float4 m = M[i];
    float r = 0.0f, g = 0.0f, b = 0.0f;
    if (m.w >= 2.0f) {
        const float w = film[i].w, k1 = m.w - 1.0f;
        r = (m.x / k1) / w;
        g = (m.y / k1) / w;
        b = (m.z / k1) / w;
    }
    out[4 * (size_t)i] = r;
    out[4 * (size_t)i + 1] = g;
    out[4 * (size_t)i + 2] = b;
    out[4 * (size_t)i + 3] = m.w;
}

void launch_denoise_prep_variance(const float *variance, const float4 *guide, const float4 *I, uint32_t n, bool demodulate,
                                  float4 *V, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_denoise_prep_variance, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, variance, guide, I, n,
                       demodulate ? 1 : 0, V);
}
void launch_denoise_atrous_guided(const DenoiseGuidedArgs &a, hipStream_t st) {
    if (a.d.width <= 0 || a.d.height <= 0) return;
    const dim3 grid((uint32_t)((a.d.width + kDnX - 1) / kDnX), (uint32_t)((a.d.height + kDnY - 1) / kDnY));
    hipLaunchKernelGGL(k_denoise_atrous_guided, grid, dim3(kDnX, kDnY), 0, st, a);
}
void launch_variance_update(const float4 *film, uint32_t n, float4 *P, float4 *M, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_variance_update, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, film, n, P, M);
}
void launch_variance_resolve(const float4 *film, const float4 *M, uint32_t n, float *out, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_variance_resolve, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, film, M, n, out);
}

void launch_denoise_prep(const float *radiance, const float *weight, const float *features, uint32_t n, bool demodulate,
                         float4 *guide, float4 *I, hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_denoise_prep, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, radiance, weight, features, n,
                       demodulate ? 1 : 0, guide, I);
}
void launch_denoise_atrous(const DenoiseArgs &a, hipStream_t st) {
    if (a.width <= 0 || a.height <= 0) return;
    const dim3 grid((uint32_t)((a.width + kDnX - 1) / kDnX), (uint32_t)((a.height + kDnY - 1) / kDnY));
    hipLaunchKernelGGL(k_denoise_atrous, grid, dim3(kDnX, kDnY), 0, st, a);
}
void launch_denoise_finish(const float4 *guide, const float4 *I, uint32_t n, bool demodulate, float *out_rgb,
                           hipStream_t st) {
    if (n == 0) return;
    hipLaunchKernelGGL(k_denoise_finish, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, guide, I, n,
                       demodulate ? 1 : 0, out_rgb);
}

}  // namespace akr
