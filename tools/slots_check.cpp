// slots_check — the host-only slot, meta-block and fixed-point layouts
// (csrc/mh_slots.hpp) on fixed cases, one JSON line per case.  Plain C++17, no
// HIP: c++ -std=c++17 tools/slots_check.cpp -o slots_check.
// tests/test_slots_host.py holds the expected values.
#include <cstdio>
#include <initializer_list>
#include <string>
#include <vector>

#include "../mitsuba3-nasa_amd/csrc/mh_slots.hpp"

using namespace mh;

template <class V>
static std::string list(const V &v, size_t n) {
    std::string s = "[";
    for (size_t i = 0; i < n; ++i) s += (i ? ", " : "") + std::to_string((long long)v[i]);
    return s + "]";
}
template <class V>
static std::string list(const V &v) { return list(v, v.size()); }

static void fx(const char *name, uint32_t bits) {
    printf("{\"case\": \"fx_exp_%s\", \"bits\": %u, \"S\": %d}\n", name, bits, slots::fx_exp(bits));
}

static void block(const char *name, std::vector<size_t> counts) {
    const slots::SlotBlock b = slots::slot_block(counts);
    size_t padded[kMaxParams];
    for (int k = 0; k < kMaxParams; ++k) padded[k] = slots::padded(counts[k]);
    printf("{\"case\": \"%s\", \"off\": %s, \"padded\": %s, \"total\": %zu, \"alloc_floats\": %zu, \"bmp_off\": %s, "
           "\"bmp_floats\": %u}\n",
           name, list(b.off, kMaxParams).c_str(), list(padded, kMaxParams).c_str(), b.total, b.alloc_floats(),
           list(b.bmp_off, kMaxBitmapParams).c_str(), b.bmp_floats);
}

static void meta(const char *name, size_t n_tex, size_t n_media, size_t n_emitters, uint32_t n_emitter_params) {
    const slots::MetaLayout o = slots::meta_layout(n_tex, n_media, n_emitters);
    printf("{\"case\": \"%s\", \"offsets\": [%zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu], \"emitter_off\": %u, "
           "\"contracts\": %d}\n",
           name, o.slot, o.is_rgb, o.bufs, o.sigma, o.albedo, o.phase, o.corner, o.emitter, o.size,
           o.emitter_off(n_emitter_params), (int)o.contracts_hold(n_media, n_emitter_params));
}

// textures 0, 2, 4, 5, 6: rgb; 1 (4 x 5 x 3), 3 (2 x 2 x 1), 7, 8, 9 (1 x 1 x 3): bitmaps;
// medium 0: homogeneous, HG; medium 1: a (2, 3, 4) grid, not HG; two emitters
static slots::SceneFacts scene() {
    slots::SceneFacts sc;
    for (int t = 0; t < 10; ++t) {
        const bool bitmap = t == 1 || t == 3 || t >= 7;
        sc.textures.push_back({bitmap ? (uint32_t)MH_TEX_BITMAP : (uint32_t)MH_TEX_RGB,
                               t == 1 ? (size_t)60 : t == 3 ? (size_t)4 : (size_t)3});
    }
    sc.media.push_back({MH_MEDIUM_HOMOGENEOUS, {0, 0, 0}, true});
    sc.media.push_back({MH_MEDIUM_HETEROGENEOUS, {2, 3, 4}, false});
    sc.n_emitters = 2;
    return sc;
}

static void build(const char *name, std::initializer_list<uint32_t> params, bool vol = true, const char *api = "mh_render_backward",
                  const char *method = "render_backward") {
    const std::vector<uint32_t> p(params);
    slots::Slots P;
    const slots::Error e = slots::build_slots(scene(), (uint32_t)p.size(), p.data(), vol, api, method, P);
    printf("{\"case\": \"%s\", \"code\": %d, \"failed\": %d, \"msg\": \"%s\"", name, e.code, (int)(bool)e, e.msg.c_str());
    if (!e) {
        uint32_t res[3 * kMaxParams];
        for (int k = 0; k < kMaxParams; ++k)
            for (int a = 0; a < 3; ++a) res[3 * k + a] = P.grid_res[k][a];
        printf(", \"slot_of_param\": %s, \"counts\": %s, \"is_rgb\": %s, \"slot_of_tex\": %s, \"sigma_slot\": %s, "
               "\"albedo_slot\": %s, \"phase_slot\": %s, \"emitter_slot\": %s, \"n_rgb\": %u, \"n_bmp\": %u, "
               "\"n_medium_params\": %u, \"n_emitter_params\": %u, \"n_phase_params\": %u, \"bmp_tex\": %u, "
               "\"grid_res\": %s",
               list(P.slot_of_param).c_str(), list(P.counts).c_str(), list(P.is_rgb).c_str(),
               list(P.slot_of_tex).c_str(), list(P.sigma_slot).c_str(), list(P.albedo_slot).c_str(),
               list(P.phase_slot).c_str(), list(P.emitter_slot).c_str(), P.n_rgb, P.n_bmp, P.n_medium_params,
               P.n_emitter_params, P.n_phase_params, P.bmp_tex, list(res, 3 * kMaxParams).c_str());
    }
    printf("}\n");
}

static void corner(const char *name, uint32_t x, uint32_t y, uint32_t z, bool fx_) {
    uint32_t res[kMaxParams][3] = {};
    res[kMaxRgbParams + 1][0] = x; res[kMaxRgbParams + 1][1] = y; res[kMaxRgbParams + 1][2] = z;
    const slots::CornerLayout c = slots::corner_layout(res, fx_);
    printf("{\"case\": \"%s\", \"use\": %s, \"off\": %s, \"values\": %zu, \"corner_floats\": %llu, \"bytes\": %zu, "
           "\"fits\": %d}\n",
           name, list(c.use, kMaxParams).c_str(), list(c.off, kMaxParams).c_str(), c.values,
           (unsigned long long)corner_floats(res[kMaxRgbParams + 1]), c.bytes(), (int)c.fits);
}

int main() {
    printf("{\"case\": \"constants\", \"max_rgb\": %d, \"max_bitmap\": %d, \"max_params\": %d, \"fx_max_off\": %u, "
           "\"fx_scale_off\": %u, \"fx_sum_off\": %u, \"fx_word_bytes\": %u}\n",
           kMaxRgbParams, kMaxBitmapParams, kMaxParams, kFxMaxOff, kFxScaleOff, kFxSumOff, kFxWordBytes);
    // ---- fx_exp: the float's bits ----
    fx("zero", 0u);
    fx("inf", 0x7f800000u);
    fx("nan", 0x7fc00000u);
    fx("one", 0x3f800000u);
    fx("two_31", 0x4f000000u);
    fx("denormal_min", 0x00000001u);
    fx("flt_max", 0x7f7fffffu);
    fx("three_quarters", 0x3f400000u);
    {   // maxima: grid 1.0, slot 0 nothing, slot 1 2^31, slot 4 FLT_MAX
        uint32_t mx[1 + kMaxParams] = {0x3f800000u, 0u, 0x4f000000u, 0u, 0u, 0x7f7fffffu, 0u, 0u, 0u};
        const slots::FxScales f = slots::fx_scales(mx);
        printf("{\"case\": \"fx_scales\", \"scale\": %.17g, \"inv\": %.17g, \"slot_scale\": [%.17g, %.17g, %.17g], "
               "\"slot_inv\": [%.17g, %.17g, %.17g], \"product\": %.17g}\n",
               f.scale, f.inv, f.slot_scale[0], f.slot_scale[1], f.slot_scale[4], f.slot_inv[0], f.slot_inv[1],
               f.slot_inv[4], f.slot_scale[4] * f.slot_inv[4]);
    }
    // ---- the slot block ----
    block("block_mixed", {3, 1, 0, 0, 10, 0, 0, 0});
    block("block_empty", {0, 0, 0, 0, 0, 0, 0, 0});
    block("block_bitmaps", {3, 0, 0, 0, 60, 4, 7, 1});
    // ---- the meta block ----
    meta("meta_3_2_1", 3, 2, 1, 1);
    meta("meta_empty", 0, 0, 0, 0);
    meta("meta_media_1", 1, 1, 0, 0);
    meta("meta_media_2", 1, 2, 0, 0);
    meta("meta_media_5", 1, 5, 3, 2);
    meta("meta_emitter_unlisted", 3, 2, 4, 0);
    {   // the image as the kernels read it: g slots as albedo_slot[n_media + m], the emitter table by its offset
        const std::vector<uint32_t> p = {MH_PARAM_MEDIUM_ALBEDO | 0u, MH_PARAM_MEDIUM_PHASE_G | 0u,
                                         MH_PARAM_EMITTER_RADIANCE | 1u};
        slots::Slots P;
        const slots::SceneFacts sc = scene();
        (void)slots::build_slots(sc, 3, p.data(), true, "a", "m", P);
        P.corner.assign(kMaxParams, nullptr);
        float *bufs[kMaxParams] = {};
        const slots::MetaLayout o = slots::meta_layout(sc.textures.size(), sc.media.size(), sc.n_emitters);
        const std::vector<uint8_t> img = slots::meta_image(o, P, bufs);
        const int32_t *albedo = reinterpret_cast<const int32_t *>(img.data() + o.albedo);
        const int32_t *em = reinterpret_cast<const int32_t *>(img.data() + o.slot + o.emitter_off(P.n_emitter_params));
        printf("{\"case\": \"meta_image\", \"size\": %zu, \"albedo\": [%d, %d], \"g_after_albedo\": [%d, %d], "
               "\"emitter_by_offset\": [%d, %d], \"contracts\": %d}\n",
               img.size(), albedo[0], albedo[1], albedo[2 + 0], albedo[2 + 1], em[0], em[1],
               (int)o.contracts_hold(sc.media.size(), P.n_emitter_params));
    }
    // ---- build_slots ----
    const uint32_t SIG = MH_PARAM_MEDIUM_SIGMA_T, ALB = MH_PARAM_MEDIUM_ALBEDO, EM = MH_PARAM_EMITTER_RADIANCE,
                   PHG = MH_PARAM_MEDIUM_PHASE_G;
    build("build_kinds", {0, 1, SIG | 0, SIG | 1, ALB | 0, PHG | 0});
    build("build_emitter", {EM | 1, 2, 3}, false);
    build("build_none", {});
    build("build_four_each", {0, 2, 4, 5, 1, 3, 7, 8});
    build("build_too_many_rgb", {0, 2, 4, 5, 6});
    build("build_too_many_small_mixed", {0, SIG | 0, ALB | 0, PHG | 0, EM | 0});
    build("build_too_many_bitmap", {1, 3, 7, 8, 9});
    build("build_too_many_large_mixed", {1, 3, 7, 8, SIG | 1});
    build("build_duplicate", {0, 0});
    build("build_duplicate_medium", {ALB | 1, SIG | 1, ALB | 1});
    build("build_texture_range", {10});
    build("build_medium_range", {SIG | 2});
    build("build_phase_range", {PHG | 2});
    build("build_emitter_range", {EM | 2});
    build("build_medium_not_vol", {ALB | 0}, false);
    build("build_phase_not_vol", {PHG | 0}, false, "mh_render_forward", "render_forward");
    build("build_phase_not_hg", {PHG | 1});
    build("build_unknown_kind", {0x50000000u});
    build("build_forward_names", {10}, true, "mh_render_forward", "render_forward");
    // ---- the corner blocks ----
    corner("corner_2_3_4", 2, 3, 4, false);
    corner("corner_2_3_4_fx", 2, 3, 4, true);
    corner("corner_two_32", 255, 255, 65535, false);          // 256 * 256 * 65536 = 2^32 corners
    corner("corner_below_two_32", 255, 255, 65534, true);     // used, but beyond 32 GiB
    corner("corner_16_gib", 511, 1023, 1023, false);          // 2^29 corners: 2^32 floats = 16 GiB
    corner("corner_32_gib_fx", 511, 1023, 1023, true);        // as int64: 32 GiB
    corner("corner_over_16_gib", 511, 1023, 1024, false);
    corner("corner_over_32_gib_fx", 511, 1023, 1024, true);
    corner("corner_none", 0, 0, 0, false);
    return 0;
}
