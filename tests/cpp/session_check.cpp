// Drives csrc/session.h for tests/test_session_host.py: one session, one command per input line, and after
// each command one reply line: "<result> | <every field of the session>".  The commands do to the record
// what capi.hip's calls do around their device work:
//   open <n> <spp> <seeded>          a render of spp samples for n slots
//   all <spp>                        a continue for every slot: check_cap, advance_all
//   subset <m> <spp> <largest>       a masked continue for m slots, whose largest count is <largest>:
//                                    cap_needs_largest (then check_cap of <largest>), advance_subset
//   range <lo> <hi>                  set_range
//   adaptive <n> <cap> <min> <pass>  adaptive_begin: open with min(cap, min) samples, adaptive_open
//   step <m_after>                   adaptive_step: adaptive_pass_spp, advance_subset for the active slots,
//                                    adaptive_advance with the slots its test leaves active
//   params <spp>                     session_params
// result: "ok", "ok <value>", "refused <message>" (a Refused) or "error <message>".
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "session.h"

static void print_state(const akr::Session &s) {
    const akr::Session::Adaptive &a = s.ad;
    const akr_adaptive_info &i = a.info;
    std::printf(" | valid=%d seeded=%d n=%llu spp_done=%d max_depth=%d flags=%d ray_clamp=%g uniform=%d spp_min=%d n_strips=%llu "
                "on=%d more=%d some_stopped=%d cap=%d pass_spp=%d total=%d threshold=%g m=%u passes=%d info_min=%d info_max=%d "
                "samples=%llu strips=%llu strips_at_cap=%llu\n",
                s.valid, s.seeded, (unsigned long long)s.n, s.spp_done, s.max_depth, s.flags, s.ray_clamp, s.uniform, s.spp_min,
                (unsigned long long)s.n_strips, a.on, a.more, a.some_stopped, a.cap, a.pass_spp, a.total, a.threshold, a.m,
                i.passes, i.spp_min, i.spp_max, (unsigned long long)i.samples, (unsigned long long)i.strips,
                (unsigned long long)i.strips_at_cap);
}

int main() {
    akr::Session s;
    const akr_pt_params base{0, 5, 2.5f, 1};
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        try {
            if (cmd == "open") {
                unsigned long long n;
                int spp, seeded;
                in >> n >> spp >> seeded;
                akr::open_session(s, base, n, spp, seeded != 0);
                std::printf("ok");
            } else if (cmd == "all") {
                int spp;
                in >> spp;
                akr::check_cap(akr::require_session(s).spp_done, spp);
                if (spp > 0) akr::advance_all(s, spp);
                std::printf("ok");
            } else if (cmd == "subset") {
                unsigned long long m;
                int spp;
                long long largest;
                in >> m >> spp >> largest;
                const bool read = akr::cap_needs_largest(akr::require_session(s), spp);
                if (read) akr::check_cap(largest, spp);
                std::printf("ok %d%d", read ? 1 : 0, (int)akr::advance_subset(s, m, spp));
            } else if (cmd == "range") {
                unsigned lo, hi;
                in >> lo >> hi;
                akr::set_range(s, lo, hi);
                std::printf("ok");
            } else if (cmd == "adaptive") {
                unsigned long long n;
                int cap;
                akr_adaptive_params ap{};
                in >> n >> cap >> ap.min_spp >> ap.pass_spp;
                ap.threshold = 0.25f;
                const int first = std::min(cap, ap.min_spp);
                akr::open_session(s, base, n, first, first > 0);
                akr::adaptive_open(s, cap, ap);
                std::printf("ok");
            } else if (cmd == "step") {
                unsigned m_after;
                in >> m_after;
                if (!akr::require_adaptive(s).ad.more) {
                    std::printf("ok done");
                } else {
                    const int step = akr::adaptive_pass_spp(s.ad);
                    if (step > 0 && s.ad.m > 0) akr::advance_subset(s, s.ad.m, step);
                    akr::adaptive_advance(s, step, m_after);
                    std::printf("ok %d", step);
                }
            } else if (cmd == "params") {
                int spp;
                in >> spp;
                const akr_pt_params p = akr::session_params(s, spp);
                std::printf("ok %d,%d,%g,%d", p.spp, p.max_depth, p.ray_clamp, p.flags);
            } else {
                std::printf("error unknown command");
            }
        } catch (const akr::Refused &e) {
            std::printf("refused %s", e.what());
        } catch (const std::exception &e) {
            std::printf("error %s", e.what());
        }
        print_state(s);
    }
    return 0;
}
