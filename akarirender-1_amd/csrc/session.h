// session.h — what a render session holds, and what it holds after each call that extends it
// (the rules are stated in include/akr_hip.h).  Plain C++, no HIP, so every
// transition is checked on the CPU (tests/cpp/session_check.cpp).  capi.hip owns the device side (the
// per-slot counts, the active list, the renders) and asks here what the session becomes.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "../../include/akr_hip.h"

namespace akr {

constexpr int32_t kSessionSppCap = 1 << 24;  // a slot's weight is an f32 count of its samples: exact up to 2^24

// A call refused before anything changed: the session stays as it was
struct Refused : std::runtime_error {
    using std::runtime_error::runtime_error;
};
[[noreturn]] inline void throw_cap(int32_t have, int32_t spp) {
    throw Refused("render session: " + std::to_string(have) + " + " + std::to_string(spp) +
                  " samples per slot exceed 2^24 (the weight is an f32 count)");
}

// The last path render, which akr_hip_render_continue extends.  seeded: the sampler states hold the state
// after each slot's last sample; false after a render of 0 spp, whose slots start from x + y * width.
struct Session {
    bool valid = false, seeded = false;
    uint64_t n = 0;
    int32_t spp_done = 0, max_depth = 0, flags = 0;
    float ray_clamp = 0.0f;
    // Slots that hold different sample counts (masked continues): spp_done is then the
    // largest count, spp_min the smallest, and the device holds every slot's expected count
    bool uniform = true;
    int32_t spp_min = 0;
    // the last adaptive render's strips, for akr_hip_adaptive_error (0: none)
    uint64_t n_strips = 0;
    // an adaptive render in progress (akr_hip_adaptive_begin / _step): every active strip holds
    // `total` samples, `m` slots are active; a continue that draws samples ends it (on = false)
    struct Adaptive {
        bool on = false, more = false, some_stopped = false;
        int32_t cap = 0, pass_spp = 0, total = 0;
        float threshold = 0.0f;
        uint32_t m = 0;
        akr_adaptive_info info{};
    } ad;
};

inline const Session &require_session(const Session &s) {
    if (!s.valid)
        throw std::runtime_error("no render session to continue (start one with akr_hip_render, akr_hip_render_device "
                                 "or akr_hip_render_state_import; scene, tree and camera changes and other renders end it)");
    return s;
}

inline void open_session(Session &s, const akr_pt_params &p, uint64_t N, int32_t spp_done, bool seeded) {
    s = Session{};
    s.valid = true;
    s.seeded = seeded;
    s.n = N;
    s.spp_done = spp_done;
    s.max_depth = p.max_depth;
    s.flags = p.flags;
    s.ray_clamp = p.ray_clamp;
    s.spp_min = spp_done;
}

// the session's parameters with `spp` more samples
inline akr_pt_params session_params(const Session &s, int32_t spp) {
    require_session(s);
    akr_pt_params p{};
    p.spp = spp;
    p.max_depth = s.max_depth;
    p.ray_clamp = s.ray_clamp;
    p.flags = s.flags;
    return p;
}

// ---- the 2^24 cap: it applies to the largest resulting count, and refuses before anything changes
// spp more samples on top of a largest count
inline void check_cap(int64_t largest, int32_t spp) {
    if (largest + spp > kSessionSppCap) throw_cap((int32_t)largest, spp);
}
// spp more samples for some of the slots.  A uniform session is checked here.  A non-uniform one can be
// refused only near the cap, by the largest count among the listed slots: true asks the caller to read
// that count and check_cap() it.
inline bool cap_needs_largest(const Session &s, int32_t spp) {
    if ((int64_t)s.spp_done + spp <= kSessionSppCap) return false;
    if (s.uniform) throw_cap(s.spp_done, spp);
    return true;
}

// ---- continues
// spp > 0 more samples for every slot (the per-slot counts of a non-uniform session advance with it)
inline void advance_all(Session &s, int32_t spp) {
    s.spp_done += spp;
    s.spp_min += spp;
    s.seeded = true;
    s.ad.on = false;
}

// what a subset pass leaves the per-slot counts to do
enum class SlotCounts {
    None,        // the session stays uniform: there are none
    Add,         // add spp to the listed slots' counts
    AddAndRead,  // and read the range back (set_range), unless the caller knows it (the adaptive loop)
};
// spp > 0 more samples for m > 0 of the session's slots.  m == n keeps a uniform session uniform; a
// uniform session that becomes non-uniform keeps its old count as the smallest.
inline SlotCounts advance_subset(Session &s, uint64_t m, int32_t spp) {
    if (s.uniform && m == s.n) {
        s.spp_done += spp;
        s.spp_min = s.spp_done;
        return SlotCounts::None;
    }
    if (!s.uniform) return SlotCounts::AddAndRead;
    s.uniform = false;
    s.spp_min = s.spp_done;
    s.spp_done += spp;
    return SlotCounts::Add;
}
inline void set_range(Session &s, uint32_t lo, uint32_t hi) {
    s.spp_min = (int32_t)lo;
    s.spp_done = (int32_t)hi;
}

// ---- the adaptive loop
inline const Session &require_adaptive(const Session &s) {
    if (!require_session(s).ad.on)
        throw std::runtime_error("adaptive step: the session is not an adaptive render in progress "
                                 "(start one with akr_hip_adaptive_begin; a continue with samples ends it)");
    return s;
}

// After the first pass (open_session with its min(cap, min_spp) samples): every slot active; `more`: a test
// and a pass remain
inline void adaptive_open(Session &s, int32_t cap, const akr_adaptive_params &ap) {
    Session::Adaptive &ad = s.ad;
    ad = Session::Adaptive{};
    ad.on = true;
    ad.cap = cap;
    ad.pass_spp = ap.pass_spp;
    ad.threshold = ap.threshold;
    ad.total = s.spp_done;
    ad.m = (uint32_t)s.n;
    ad.info.passes = 1;
    ad.info.spp_min = ad.info.spp_max = s.spp_done;
    ad.info.samples = s.n * (uint64_t)s.spp_done;
    ad.info.strips = (s.n + 63) / 64;
    ad.more = cap > ap.min_spp && s.n > 0;
    if (ad.more) s.n_strips = ad.info.strips;
}

// the next pass's samples: every active strip holds ad.total; the pass is clipped at the cap
inline int32_t adaptive_pass_spp(const Session::Adaptive &ad) {
    const int64_t want = ad.pass_spp > 0 ? (int64_t)ad.total + ad.pass_spp : 2 * (int64_t)ad.total;
    return (int32_t)(std::min<int64_t>(want, ad.cap) - ad.total);
}

// After a pass of `step` samples for the ad.m active slots and its test, which left m_after slots active
inline void adaptive_advance(Session &s, int32_t step, uint32_t m_after) {
    Session::Adaptive &ad = s.ad;
    akr_adaptive_info &out = ad.info;
    const uint32_t before = ad.m;
    ad.total += step;
    out.passes++;
    out.samples += (uint64_t)before * (uint64_t)step;
    ad.m = m_after;
    if (!ad.some_stopped) {  // no strip had stopped before this test: the smallest count follows the total
        out.spp_min = ad.total;
        if (ad.m < before) ad.some_stopped = true;
    }
    out.spp_max = ad.total;
    s.spp_done = out.spp_max;
    s.spp_min = out.spp_min;
    ad.more = ad.m > 0 && ad.total < ad.cap;
    // strips are 64 slots, but for a short last one
    out.strips_at_cap = ad.total >= ad.cap ? ((uint64_t)ad.m + 63) / 64 : 0;
}

}  // namespace akr
