// scene_check — the host-only scene build (csrc/mh_scene_build.hpp, mh_records.hpp)
// on descriptions and tables that tests/test_scene_host.py writes to files, one
// JSON line per case.  Plain C++17 with its own main; mh_bvh.cpp is linked for
// the BVH the key table and the pair records are made from:
//   hipcc -std=c++17 -ffp-contract=off tools/scene_check.cpp -x hip --offload-arch=gfx950 csrc/mh_bvh.cpp -lpthread
// The expected values live in the test, never here.
//
//   scene_check validate <desc>...           code and message of scene::validate
//   scene_check build <desc> <packet_max>    build_prims, the BVH's leaf order, key_table, pair_records, records
//   scene_check facts <desc> <node_bytes> <prim_bytes> <n_prims> <depth> <packet_max> <shade> <bvh4_off>
//                     <stream_stack> <stream_threads> <depth4>
//   scene_check phase_table <table>...       a table file: u32 n, n floats cost, n floats values
//   scene_check assemble                     the fixed media list of the test's docstring
//   scene_check check_blend                  scene::check_blend's rejections
//
// A description file is a mh_scene_desc, then 11 u64 byte counts (~0: NULL) of
// shapes, bsdfs, textures, emitters, media, positions, normals, texcoords,
// faces, texels, grid_data, then those tables one after the other.  Each table
// is copied into an allocation of exactly its size, so a read beyond it is an
// error under AddressSanitizer.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../mitsuba3-nasa_amd/csrc/mh_scene_build.hpp"

using namespace mh;

static std::vector<uint8_t> read_file(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    std::vector<uint8_t> b;
    uint8_t buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) b.insert(b.end(), buf, buf + n);
    fclose(f);
    return b;
}

struct Loaded {
    mh_scene_desc desc;
    std::unique_ptr<uint8_t[]> tables[11];
};
static void load(const char *path, Loaded &L) {
    const std::vector<uint8_t> b = read_file(path);
    if (b.size() < sizeof(mh_scene_desc) + 11 * 8) { fprintf(stderr, "%s: short file\n", path); exit(2); }
    memcpy(&L.desc, b.data(), sizeof(mh_scene_desc));
    uint64_t len[11];
    memcpy(len, b.data() + sizeof(mh_scene_desc), sizeof(len));
    size_t at = sizeof(mh_scene_desc) + sizeof(len);
    const void *p[11];
    for (int i = 0; i < 11; ++i) {
        p[i] = nullptr;
        if (len[i] == ~0ull) continue;
        if (at + len[i] > b.size()) { fprintf(stderr, "%s: short table\n", path); exit(2); }
        L.tables[i].reset(new uint8_t[len[i]]);
        memcpy(L.tables[i].get(), b.data() + at, len[i]);
        p[i] = L.tables[i].get();
        at += len[i];
    }
    mh_scene_desc &d = L.desc;
    d.shapes = (const mh_shape *)p[0]; d.bsdfs = (const mh_bsdf *)p[1]; d.textures = (const mh_texture *)p[2];
    d.emitters = (const mh_emitter *)p[3]; d.media = (const mh_medium *)p[4]; d.positions = (const float *)p[5];
    d.normals = (const float *)p[6]; d.texcoords = (const float *)p[7]; d.faces = (const uint32_t *)p[8];
    d.texels = (const float *)p[9]; d.grid_data = (const float *)p[10];
}

static std::string words(const void *p, size_t bytes) {  // as a list of u32
    std::string s = "[";
    for (size_t i = 0; i < bytes / 4; ++i) {
        uint32_t w;
        memcpy(&w, (const uint8_t *)p + 4 * i, 4);
        s += (i ? ", " : "") + std::to_string(w);
    }
    return s + "]";
}
template <class T>
static std::string words(const std::vector<T> &v) { return words(v.data(), v.size() * sizeof(T)); }

static std::string base(const char *path) {
    std::string s(path);
    const size_t i = s.find_last_of('/');
    return i == std::string::npos ? s : s.substr(i + 1);
}

static void print_error(const std::string &name, const scene::Error &e) {
    printf("{\"case\": \"%s\", \"code\": %d, \"failed\": %d, \"msg\": \"%s\"}\n", name.c_str(), e.code, (int)(bool)e, e.msg.c_str());
}

static int do_build(const char *path, uint32_t packet_max) {
    Loaded L;
    load(path, L);
    if (scene::Error e = scene::validate(L.desc)) { print_error(base(path), e); return 1; }
    const std::vector<BuildPrim> bp = scene::build_prims(L.desc);
    BvhOut bvh;
    build_bvh(bp, bvh, 4, 1.0f);
    const scene::Records R = scene::records(L.desc);
    std::vector<uint64_t> grid_offsets;
    for (const DMedium &m : R.media) grid_offsets.push_back(m.grid_offset);
    std::string go = "[";
    for (size_t i = 0; i < grid_offsets.size(); ++i) go += (i ? ", " : "") + std::to_string(grid_offsets[i]);
    printf("{\"case\": \"build\", \"prim_bytes\": %zu, \"prims\": %s, \"n_prims\": %u, \"n_nodes\": %u, \"bvh_prims\": %s, "
           "\"key_table\": %s, \"pairs\": %s, \"shapes\": %s, \"media\": %s, \"bsdf_type\": %s, \"bsdf_tex\": %s, "
           "\"textures\": %s, \"emitters\": %s, \"grid\": %s, \"grid_offsets\": %s]}\n",
           sizeof(BuildPrim), words(bp).c_str(), bvh.n_prims, bvh.n_nodes, words(bvh.prims).c_str(),
           words(scene::key_table(bvh)).c_str(), words(scene::pair_records(bvh, packet_max)).c_str(),
           words(R.shapes).c_str(), words(R.media).c_str(), words(R.bsdf_type).c_str(), words(R.bsdf_tex).c_str(),
           words(R.textures).c_str(), words(R.emitters).c_str(), words(R.grid).c_str(), go.c_str());
    return 0;
}

static int do_facts(char **a) {
    Loaded L;
    load(a[0], L);
    auto u = [&](int i) { return (uint32_t)strtoull(a[i], nullptr, 10); };
    scene::Limits lim;
    lim.packet_max_prims = u(5);
    lim.shade_records = u(6) != 0;
    lim.bvh4_off = u(7) != 0;
    lim.stream_stack = u(8);
    lim.stream_threads = u(9);
    const scene::Facts F = scene::facts(L.desc, strtoull(a[1], nullptr, 10), strtoull(a[2], nullptr, 10), u(3), u(4), lim);
    const TabLayout TL = tab_layout(L.desc.n_shapes, L.desc.n_bsdfs, L.desc.n_textures, L.desc.n_emitters, L.desc.n_vertices,
                                    L.desc.n_faces, L.desc.normals && L.desc.n_vertices, L.desc.texcoords && L.desc.n_vertices);
    const float fl[5] = {F.inv_width, F.inv_height, F.inv_n_emitters, F.n_emitters_f, F.env_pdf};
    const uint32_t wide = scene::wide_stack_size(F.stack_size, u(10));
    printf("{\"case\": \"facts\", \"vol_flags\": %u, \"tab_total\": %u, \"tab_bytes\": %u, \"lds_bytes_bvh\": %u, "
           "\"stack_size\": %u, \"too_deep\": %d, \"wide_bvh\": %d, \"shade_records\": %d, \"floats\": %s, "
           "\"wide_stack\": %u, \"ovf_words\": %zu, \"ovf_words_wide\": %zu}\n",
           F.vol_flags, TL.total, F.tab_bytes, F.lds_bytes_bvh, F.stack_size, (int)F.too_deep, (int)F.wide_bvh,
           (int)F.shade_records, words(fl, sizeof(fl)).c_str(), wide, scene::stack_overflow_words(F.stack_size, lim),
           scene::stack_overflow_words(wide, lim));
    return 0;
}

static void do_phase_table(const char *path) {
    const std::vector<uint8_t> b = read_file(path);
    uint32_t n;
    memcpy(&n, b.data(), 4);
    // exact-size copies: a read past a table is an error under AddressSanitizer
    std::vector<float> cost(n), values(n);
    memcpy(cost.data(), b.data() + 4, 4 * (size_t)n);
    memcpy(values.data(), b.data() + 4 + 4 * (size_t)n, 4 * (size_t)n);
    std::vector<PhaseRec> tab;
    uint32_t valid = 0;
    const scene::Error e = scene::phase_table("fn: ", n, cost.data(), values.data(), tab, valid);
    printf("{\"case\": \"%s\", \"code\": %d, \"msg\": \"%s\", \"valid\": %u, \"tab\": %s}\n", base(path).c_str(), e.code,
           e.msg.c_str(), valid, e ? "[]" : words(tab).c_str());
}

static std::vector<PhaseRec> table(std::vector<float> cost, std::vector<float> values, uint32_t &valid) {
    std::vector<PhaseRec> tab;
    if (scene::phase_table("fn: ", (uint32_t)cost.size(), cost.data(), values.data(), tab, valid)) exit(3);
    return tab;
}

static void print_assembled(const char *name, const std::vector<DMedium> &media, const std::vector<scene::BlendHost> &blends,
                            const scene::PhaseData &P, const scene::Error &e) {
    std::string m = "[", bl = "[";
    for (size_t i = 0; i < media.size(); ++i) {
        m += (i ? ", [" : "[") + std::to_string(media[i].tab_offset) + ", " + std::to_string(media[i].tab_n) + "]";
        const DBlend &r = blends[i].rec;
        DBlend in_all{};  // the record as the kernels find it, at the medium's tab_offset
        if (blends[i].set) memcpy(static_cast<void *>(&in_all), &P.all[media[i].tab_offset], sizeof(DBlend));
        bl += (i ? ", [" : "[") + std::to_string((int)blends[i].set) + ", " + std::to_string(r.tab_offset[0]) + ", " +
              std::to_string(r.tab_n[0]) + ", " + std::to_string(r.tab_offset[1]) + ", " + std::to_string(r.tab_n[1]) + ", " +
              std::to_string(r.grid_offset) + ", " + std::to_string(blends[i].set ? memcmp(&in_all, &r, sizeof(DBlend)) == 0 : 1) + "]";
    }
    const scene::Error c = scene::check_phase_tables("api", media, blends);
    printf("{\"case\": \"%s\", \"code\": %d, \"records\": %zu, \"grid_total\": %" PRIu64 ", \"media\": %s], \"blends\": %s], "
           "\"check_code\": %d, \"check_msg\": \"%s\"}\n",
           name, e.code, P.all.size(), P.grid_total, m.c_str(), bl.c_str(), c.code, c.msg.c_str());
}

// media: 0 tabulated (3 nodes); 1 blend (hg, tabulated); 2 and 3 blends with 4 x 4 x 4 and 5 x 3 x 2 weight
// grids; 4 tabulated without a table.  The media's own grids take 128 floats.
static void do_assemble() {
    std::vector<DMedium> media(5);
    for (DMedium &m : media) memset(&m, 0, sizeof(m));
    media[0].phase = media[4].phase = MH_PHASE_TABULATED;
    media[1].phase = media[2].phase = media[3].phase = MH_PHASE_BLEND;
    std::vector<std::vector<PhaseRec>> tabs(5);
    std::vector<scene::BlendHost> blends(5);
    const uint64_t grid_floats = 128;
    scene::PhaseData P;
    tabs[0] = table({-1.f, 0.f, 1.f}, {1.f, 2.f, 1.f}, media[0].tab_valid);
    mh_phase_blend b{};
    b.phase[0] = MH_PHASE_HG; b.g[0] = 0.5f; b.phase[1] = MH_PHASE_TABULATED; b.weight = 0.25f;
    if (scene::check_blend("fn: ", media, 1, &b)) exit(3);
    scene::set_blend(blends[1], b);
    scene::Error e = scene::assemble_phase_data("fn: ", media, tabs, blends, true, grid_floats, P);
    print_assembled("assemble_child_missing", media, blends, P, e);
    blends[1].tab[1] = table({-1.f, 1.f}, {1.f, 1.f}, blends[1].rec.tab_valid[1]);
    e = scene::assemble_phase_data("fn: ", media, tabs, blends, false, grid_floats, P);
    print_assembled("assemble_child_arrived", media, blends, P, e);
    std::vector<float> w(64, 0.5f);
    mh_phase_blend g{};
    g.phase[0] = MH_PHASE_ISOTROPIC; g.phase[1] = MH_PHASE_RAYLEIGH;
    g.grid_res[0] = g.grid_res[1] = g.grid_res[2] = 4;
    g.grid_data = w.data();
    if (scene::check_blend("fn: ", media, 2, &g)) exit(3);
    scene::set_blend(blends[2], g);
    w.assign(30, 0.75f);
    g.grid_res[0] = 5; g.grid_res[1] = 3; g.grid_res[2] = 2;
    g.grid_data = w.data();
    if (scene::check_blend("fn: ", media, 3, &g)) exit(3);
    scene::set_blend(blends[3], g);
    e = scene::assemble_phase_data("fn: ", media, tabs, blends, true, grid_floats, P);
    print_assembled("assemble_two_grids", media, blends, P, e);
    tabs[4] = table({-1.f, 1.f}, {0.f, 1.f}, media[4].tab_valid);
    e = scene::assemble_phase_data("fn: ", media, tabs, blends, false, grid_floats, P);
    print_assembled("assemble_all_ready", media, blends, P, e);
}

static void do_check_blend() {
    std::vector<DMedium> media(2);
    for (DMedium &m : media) memset(&m, 0, sizeof(m));
    media[0].phase = MH_PHASE_BLEND;
    media[1].phase = MH_PHASE_HG;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    std::vector<float> w(8, 0.5f);
    auto run = [&](const char *name, uint32_t medium, const mh_phase_blend *b) {
        print_error(name, scene::check_blend("fn: ", media, medium, b));
    };
    mh_phase_blend ok{};
    ok.phase[0] = MH_PHASE_HG; ok.g[0] = -0.3f; ok.phase[1] = MH_PHASE_TABULATED; ok.weight = 0.5f;
    run("blend_ok", 0, &ok);
    run("blend_null", 0, nullptr);
    run("blend_medium_range", 2, &ok);
    run("blend_not_blend", 1, &ok);
    mh_phase_blend b = ok;
    b.phase[1] = MH_PHASE_BLEND;
    run("blend_nested", 0, &b);
    b = ok; b.g[0] = 1.f;
    run("blend_g", 0, &b);
    b = ok; b.phase[0] = MH_PHASE_RAYLEIGH; b.g[0] = 0.1f;
    run("blend_rayleigh", 0, &b);
    b = ok; b.weight = nan;
    run("blend_weight", 0, &b);
    b = ok; b.grid_res[0] = 2; b.grid_res[1] = 2;
    run("blend_partial_res", 0, &b);
    b.grid_res[2] = 2;
    run("blend_null_grid", 0, &b);
    b.grid_data = w.data();
    run("blend_grid_ok", 0, &b);
    w[7] = nan;
    run("blend_grid_nan", 0, &b);
    w[7] = 0.f; b.grid_to_local[11] = nan;
    run("blend_transform_nan", 0, &b);
    b = ok; b.grid_res[0] = b.grid_res[1] = b.grid_res[2] = 4096; b.grid_data = w.data();  // 2^36 texels: refused before any read
    run("blend_grid_2_32", 0, &b);
}

int main(int argc, char **argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "validate") {
        for (int i = 2; i < argc; ++i) {
            Loaded L;
            load(argv[i], L);
            print_error(base(argv[i]), scene::validate(L.desc));
        }
        return 0;
    }
    if (mode == "build" && argc == 4) return do_build(argv[2], (uint32_t)atoi(argv[3]));
    if (mode == "facts" && argc == 13) return do_facts(argv + 2);
    if (mode == "phase_table") {
        for (int i = 2; i < argc; ++i) do_phase_table(argv[i]);
        return 0;
    }
    if (mode == "assemble") { do_assemble(); return 0; }
    if (mode == "check_blend") { do_check_blend(); return 0; }
    fprintf(stderr, "usage: see the head of tools/scene_check.cpp\n");
    return 2;
}
