// Drives the option table (csrc/options.h) from stdin; includes nothing but that HIP-free header.
//   table            -> one line per row: name kind lo hi default
//   reset            -> a fresh Options
//   set <key> <v>    -> "ok <value read back>" or "error <message>"
//   get <key>        -> "<value>", for stats / pixel_probe followed by their two derived booleans
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "options.h"

using namespace akr;

int main() {
    static const char *kinds[] = {"flag", "range", "floor", "pow2", "tri"};
    Options o;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream ss(line);
        std::string cmd, key;
        long long v = 0;
        ss >> cmd >> key >> v;
        if (cmd == "table") {
            const Options fresh;
            for (const OptionRow &r : kOptionTable)
                std::printf("%s %s %lld %lld %lld\n", r.name, kinds[r.kind], (long long)r.lo, (long long)r.hi,
                            (long long)get_option(fresh, r));
            std::printf("end\n");
        } else if (cmd == "reset") {
            o = Options();
        } else if (cmd == "set") {
            const std::string why = set_option(o, key.c_str(), v);
            if (why.empty()) std::printf("ok %lld\n", (long long)get_option(o, *find_option(key.c_str())));
            else std::printf("error %s\n", why.c_str());
        } else if (cmd == "get") {
            const OptionRow *r = find_option(key.c_str());
            if (!r) std::printf("error unknown\n");
            else if (key == "stats") std::printf("%lld %d %d\n", (long long)get_option(o, *r), (int)o.stats_on(), (int)o.stats_closest_only());
            else if (key == "pixel_probe") std::printf("%lld %d %d\n", (long long)get_option(o, *r), (int)o.probe(), (int)o.probe_clock());
            else std::printf("%lld\n", (long long)get_option(o, *r));
        }
    }
    return 0;
}
