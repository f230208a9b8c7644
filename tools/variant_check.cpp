// variant_check — the host-only kernel-variant selectors (csrc/mh_variant.hpp)
// over the whole input space of every kernel family, one line per case:
//   family | the inputs | the key, where the family has one | what the selector hands to the launcher
// (integers, space separated).  Plain C++17, no HIP:
// c++ -std=c++17 tools/variant_check.cpp -o variant_check.
// tests/test_variant_host.py holds the expected lines.
#include <cstdio>
#include <initializer_list>

#include "../mitsuba3-nasa_amd/csrc/mh_variant.hpp"

using namespace mh::variant;

// "| key... | handed..." and the end of the line
static const auto print = [](auto... c) { (printf(" %d", (int)decltype(c)::value), ...); };
static void end(bool selected) { printf(selected ? "\n" : " none\n"); }
template <class K>
static void put(const K &key, std::initializer_list<int> key_values) {
    printf(" |");
    for (int v : key_values) printf(" %d", v);
    printf(" |");
    end(dispatch(key, print));
}

// every scene and environment: "lds n_prims tables vol_flags eng lane notab unfused"
template <class Fn>
static void each_facts(const char *family, Fn &&fn) {
    Facts f;
    f.packet_max_prims = 64;
    for (int lds = 0; lds < 2; ++lds)
        for (uint32_t n_prims : {0u, 1u, 64u, 65u})
            for (int tables = 0; tables < 2; ++tables)
                for (uint32_t vol_flags : {0u, 3u, 4u, 8u, 12u})
                    for (int eng = 0; eng < 4; ++eng)
                        for (int env = 0; env < 8; ++env) {
                            f.bvh_lds = lds;
                            f.n_prims = n_prims;
                            f.tables = tables;
                            f.vol_flags = vol_flags;
                            f.stream_eng = eng;
                            f.traversal_lane = env & 1;
                            f.vs_notab = env & 2;
                            f.wf_unfused = env & 4;
                            fn(f, [&] {
                                printf("%s | %d %u %d %u %d %d %d %d", family, lds, n_prims, tables, vol_flags, eng,
                                       env & 1, (env >> 1) & 1, (env >> 2) & 1);
                            });
                        }
}

int main() {
    each_facts("vol_sched", [](const Facts &f, auto head) {
        for (uint32_t type = 0; type < 4; ++type) {
            const VolSched k = vol_sched(f, type);
            head(), printf(" %u", type), put(k, {k.machine, k.home.lds, k.home.packet, k.home.tab});
        }
    });
    each_facts("vol_sched_bwd", [](const Facts &f, auto head) {
        for (int em = 0; em < 2; ++em) {
            const VolSched k = vol_sched_bwd(f, em);
            head(), printf(" %d", em), put(k, {k.machine, k.home.lds, k.home.packet, k.home.tab});
        }
    });
    each_facts("volwave", [](const Facts &f, auto head) {
        for (int first = 0; first < 2; ++first) {
            const VolKernel k = volwave(f, first);
            head(), printf(" %d", first), put(k, {k.fresh, k.ph, k.home.lds, k.home.packet, k.home.tab});
        }
    });
    each_facts("vol_lane", [](const Facts &f, auto head) {
        const VolKernel k = vol_lane(f);
        head(), put(k, {k.fresh, k.ph, k.home.lds, k.home.packet, k.home.tab});
    });
    each_facts("render", [](const Facts &f, auto head) {
        for (uint32_t type = 0; type < 6; ++type) head(), printf(" %u | |", type), end(render(f, type, print));
    });
    each_facts("render_forward", [](const Facts &f, auto head) {
        for (uint32_t type = 0; type < 6; ++type) head(), printf(" %u | |", type), end(render_forward(f, type, print));
    });
    each_facts("wf_trace", [](const Facts &f, auto head) {
        for (uint32_t n_rgb : {0u, 1u, 2u, 4u}) {
            const WfTrace k = wf_trace(f, n_rgb);
            head(), printf(" %u", n_rgb), put(k, {k.lds, k.packet, k.eng, k.nr1});
        }
    });
    each_facts("shade_prb", [](const Facts &f, auto head) {
        for (uint32_t n_rgb : {0u, 1u, 2u, 4u})
            for (int em = 0; em < 2; ++em) head(), printf(" %u %d | |", n_rgb, em), end(shade_prb(f, n_rgb, em, print));
    });
    each_facts("wf_fused", [](const Facts &f, auto head) { head(), printf(" | %d |\n", (int)wf_fused(f)); });
    for (int first = 0; first < 2; ++first)
        for (uint32_t n_rgb : {0u, 1u, 2u, 4u})
            for (int flags = 0; flags < 8; ++flags) {
                printf("bounce_prb | %d %u %d %d %d | |", first, n_rgb, flags & 1, (flags >> 1) & 1, (flags >> 2) & 1);
                end(bounce_prb(first, n_rgb, flags & 1, flags & 2, flags & 4, print));
            }
    for (uint32_t fmt = 0; fmt < 8; ++fmt) printf("develop | %u | |", fmt), end(develop(fmt, print));
    for (int det = 0; det < 2; ++det)
        for (int pass = det; pass <= 2 * det; ++pass)  // deterministic: the passes 1 and 2; else one launch
            for (int fits = 0; fits < 2; ++fits)
                printf("bitmap_scatter | %d %d %d | |", det, pass, fits), end(bitmap_scatter(det, pass, fits, print));
    return 0;
}
