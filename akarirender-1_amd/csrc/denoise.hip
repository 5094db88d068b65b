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
