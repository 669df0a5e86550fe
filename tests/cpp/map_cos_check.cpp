// csrc/lcm_map_host.h's map_cos_min, the host function that turns lcm_map_params.min_parallax_deg into the cosine the kernel
// compares with, as a stand-alone program: tests/test_map_limit_cases_host.py builds it with -fsanitize=address,undefined and
// asks it for the cosines of the doubles around an angle, to show that a min_parallax_deg exists whose cosine equals a record's
// cos_parallax bit for bit.  No device.
//   map_cos_check <bits of a positive double, hex> <first step> <last step>
// prints, for every double `step` bit patterns away from the given one, its pattern and that of map_cos_min of it.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "lcm_map_host.h"

int main(int argc, char** argv) {
    if (argc != 4) { std::printf("usage: map_cos_check <hex bits> <first step> <last step>\n"); return 2; }
    const uint64_t bits = std::strtoull(argv[1], nullptr, 16);
    const long first = std::strtol(argv[2], nullptr, 10), last = std::strtol(argv[3], nullptr, 10);
    if (first > last || last - first > 1000000) return 2;
    for (long s = first; s <= last; ++s) {
        const uint64_t b = bits + (uint64_t)(int64_t)s;
        double deg, c;
        std::memcpy(&deg, &b, sizeof(deg));
        if (!(deg > 0.0) || !(deg <= 180.0)) return 2;
        c = lcm::map_cos_min(deg);
        uint64_t cb;
        std::memcpy(&cb, &c, sizeof(cb));
        std::printf("%016" PRIx64 " %016" PRIx64 "\n", b, cb);
    }
    return 0;
}
