// fuse01_check — when the fused wavefront runs the camera bounce and the bounce
// after it in one launch (variant::bounce_path, csrc/mh_variant.hpp), on plain
// values, one line per case:
//   bounce_path | tables unfused max_depth fused_lds_bytes | two next next_buf | Gen Two of the first launch
// then the limits the rule is built from.  Plain C++17, no HIP:
// c++ -std=c++17 tools/fuse01_check.cpp -o fuse01_check.
// tests/test_fuse01_host.py holds the expected lines.
#include <cstdio>
#include <initializer_list>

#include "../mitsuba3-nasa_amd/csrc/mh_variant.hpp"

using namespace mh::variant;

int main() {
    printf("limits | %d %u %u %u\n", (int)MH_WF_FUSE01, kParkDwords, kParkBytes, kFuse01MaxLds);
    Facts f;
    f.packet_max_prims = 64;
    f.n_prims = 32;
    for (int tables = 0; tables < 2; ++tables)
        for (int unfused = 0; unfused < 2; ++unfused)
            for (uint32_t max_depth : {1u, 2u, 3u, 8u, 64u})
                for (uint32_t lds : {0u, 13856u, 16383u, 16384u, 16385u, 65536u}) {
                    f.tables = tables;
                    f.wf_unfused = unfused;
                    const BouncePath p = bounce_path(f, max_depth, lds);
                    printf("bounce_path | %d %d %u %u | %d %u %u |", tables, unfused, max_depth, lds, (int)p.two, p.next,
                           p.next_buf);
                    if (!bounce(true, p.two, [](auto... c) { (printf(" %d", (int)decltype(c)::value), ...); }))
                        printf(" none");
                    printf("\n");
                }
    // a launch after the first
    printf("later | | |");
    if (!bounce(false, false, [](auto... c) { (printf(" %d", (int)decltype(c)::value), ...); })) printf(" none");
    printf("\n");
    return 0;
}
