// mh_slots.hpp — the layouts the gradient calls share with their kernels,
// worked out from plain values (host only).
//
// mh_render_backward and mh_render_forward (mh_api.hip) assign every listed
// parameter a slot, lay the slots' buffers out in one block, describe them to
// the kernels in a meta block, and, with MH_FLAG_DETERMINISTIC, sum in int64
// fixed point through a few words whose offsets the kernels (mh_shading.hpp)
// know too.  All of that arithmetic is here: no HIP, no environment, no state,
// so it is checked without a GPU (tools/slots_check.cpp, tests/test_slots_host.py).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mitsuba_hip.h"

namespace mh {

constexpr int kMaxRgbParams = 4;     // constant-albedo gradient slots (register accumulators)
constexpr int kMaxBitmapParams = 4;  // bitmap gradient slots (global atomics)
constexpr int kMaxParams = kMaxRgbParams + kMaxBitmapParams;

// ---- the deterministic fixed-point words (mh_scene::fx_word, GradArgs::fx_max) ----
// u32 max[0] (the grid scatter) and max[1 + k] (slot k): the largest |item| of
// pass 1 as float bits; double scale[k] of slot k; int64 sums[3 k + c] of small
// slot k (acc_add_fx, bmp_add_fx, flush_small_slots)
constexpr uint32_t kFxMaxOff = 0, kFxScaleOff = 64, kFxSumOff = 192, kFxWordBytes = 512;
static_assert(kFxMaxOff + 4 * (1 + kMaxParams) <= kFxScaleOff && kFxScaleOff + 8 * kMaxParams <= kFxSumOff &&
                  kFxSumOff + 8 * 3 * kMaxRgbParams <= kFxWordBytes && kFxScaleOff % 8 == 0 && kFxSumOff % 8 == 0,
              "the maxima, scales and sums of the fixed-point words do not overlap");

// per-cell corner block of a grid sigma_t slot: 8 floats per cell of the padded grid
inline uint64_t corner_floats(const uint32_t res[3]) {
    return (uint64_t)(res[0] + 1) * (res[1] + 1) * (res[2] + 1) * 8u;
}

namespace slots {

// S with |item| * 2^S < 2^31 for the largest |item| (its float bits) of pass
// 1: round(item * 2^S) fits an int32, so 2^31 items sum in int64 without
// overflow.  Nothing recorded, or a non-finite maximum: 31.
inline int fx_exp(uint32_t bits) {
    float mx;
    memcpy(&mx, &bits, 4);
    int ex = 0;
    if (mx > 0.f && std::isfinite(mx)) (void)std::frexp(mx, &ex);  // mx < 2^ex
    return 31 - ex;
}
// the scales of pass 2 from pass 1's maxima words: the grid scatter's and each slot's
struct FxScales {
    double scale = 1.0, inv = 1.0;  // 2^S and 2^-S of max[0]
    double slot_scale[kMaxParams], slot_inv[kMaxParams];
    FxScales() { for (int k = 0; k < kMaxParams; ++k) slot_scale[k] = slot_inv[k] = 1.0; }
};
inline FxScales fx_scales(const uint32_t maxima[1 + kMaxParams]) {
    FxScales f;
    f.scale = std::ldexp(1.0, fx_exp(maxima[0]));
    f.inv = std::ldexp(1.0, -fx_exp(maxima[0]));
    for (int k = 0; k < kMaxParams; ++k) {
        f.slot_scale[k] = std::ldexp(1.0, fx_exp(maxima[1 + k]));
        f.slot_inv[k] = std::ldexp(1.0, -fx_exp(maxima[1 + k]));
    }
    return f;
}

// ---- differentiated parameters -> slots --------------------------------------
// small slots 0 .. n_rgb-1 (register accumulators): rgb textures, medium
// albedo, homogeneous sigma_t, emitter radiance, HG asymmetry; large slots
// kMaxRgbParams .. (global atomics / tangent arrays): bitmaps, grids
struct SceneFacts {
    struct Texture { uint32_t type; size_t floats; };                     // MH_TEX_*, w * h * channels
    struct Medium { uint32_t type; uint32_t grid_res[3]; bool hg; };      // MH_MEDIUM_*, phase == MH_PHASE_HG
    std::vector<Texture> textures;
    std::vector<Medium> media;
    size_t n_emitters = 0;
};
struct Slots {
    std::vector<int32_t> slot_of_tex, sigma_slot, albedo_slot, emitter_slot, phase_slot;
    std::vector<uint32_t> is_rgb;
    std::vector<size_t> counts;
    std::vector<uint32_t> slot_of_param;
    uint32_t n_rgb = 0, n_bmp = 0, n_medium_params = 0, n_emitter_params = 0, n_phase_params = 0, bmp_tex = 0;
    uint32_t grid_res[kMaxParams][3] = {};  // large sigma_t slots: the grid's resolution (x, y, z)
    std::vector<float *> corner;            // their corner blocks (upload_slots, corners = true)
    bool fx = false;                        // the blocks hold int64 fixed point (deterministic)
    std::vector<uint8_t> meta;  // host image of the meta block (uploaded by upload_slots when it changed)
};
struct Error {
    int code = MH_OK;
    std::string msg;
    explicit operator bool() const { return code != MH_OK; }
};

inline Error build_slots(const SceneFacts &sc, uint32_t n_params, const uint32_t *param_tex, bool vol, const char *api,
                         const char *method, Slots &P) {
    const std::string a(api), m(method);
    const size_t n_textures = sc.textures.size(), n_media = sc.media.size();
    P.slot_of_tex.assign(std::max<size_t>(n_textures, 1), -1);
    P.sigma_slot.assign(std::max<size_t>(n_media, 1), -1);
    P.albedo_slot = P.sigma_slot;
    P.phase_slot = P.sigma_slot;
    P.emitter_slot.assign(std::max<size_t>(sc.n_emitters, 1), -1);
    P.is_rgb.assign(kMaxParams, 0);
    P.counts.assign(kMaxParams, 0);
    P.slot_of_param.assign(n_params, 0);
    for (uint32_t k = 0; k < n_params; ++k) {
        const uint32_t kind = param_tex[k] & MH_PARAM_KIND_MASK, idx = param_tex[k] & ~MH_PARAM_KIND_MASK;
        int32_t *owner;
        bool small;
        size_t cnt;
        if (kind == 0) {
            if (idx >= n_textures) return {MH_ERR_INVALID_ARGUMENT, a + ": texture index out of bounds"};
            owner = &P.slot_of_tex[idx];
            small = sc.textures[idx].type == MH_TEX_RGB;
            cnt = small ? 3 : sc.textures[idx].floats;
        } else if (kind == MH_PARAM_MEDIUM_SIGMA_T || kind == MH_PARAM_MEDIUM_ALBEDO) {
            if (!vol) return {MH_ERR_UNSUPPORTED, m + "(): medium parameters require the 'prbvolpath' integrator"};
            if (idx >= n_media) return {MH_ERR_INVALID_ARGUMENT, a + ": medium index out of bounds"};
            const SceneFacts::Medium &md = sc.media[idx];
            ++P.n_medium_params;
            if (kind == MH_PARAM_MEDIUM_ALBEDO) {
                owner = &P.albedo_slot[idx]; small = true; cnt = 3;
            } else {
                owner = &P.sigma_slot[idx];
                small = md.type == MH_MEDIUM_HOMOGENEOUS;
                cnt = small ? 1 : (size_t)md.grid_res[0] * md.grid_res[1] * md.grid_res[2];
            }
        } else if (kind == MH_PARAM_MEDIUM_PHASE_G) {
            if (!vol) return {MH_ERR_UNSUPPORTED, m + "(): medium parameters require the 'prbvolpath' integrator"};
            if (idx >= n_media) return {MH_ERR_INVALID_ARGUMENT, a + ": medium index out of bounds"};
            if (!sc.media[idx].hg)
                return {MH_ERR_UNSUPPORTED, m + "(): MH_PARAM_MEDIUM_PHASE_G needs a medium whose phase function "
                                                "is MH_PHASE_HG (other phase functions' parameters are not "
                                                "differentiable)"};
            ++P.n_medium_params;
            ++P.n_phase_params;
            owner = &P.phase_slot[idx]; small = true; cnt = 1;
        } else if (kind == MH_PARAM_EMITTER_RADIANCE) {
            if (idx >= sc.n_emitters) return {MH_ERR_INVALID_ARGUMENT, a + ": emitter index out of bounds"};
            ++P.n_emitter_params;
            owner = &P.emitter_slot[idx]; small = true; cnt = 3;
        } else {
            return {MH_ERR_INVALID_ARGUMENT, a + ": unknown parameter kind"};
        }
        if (*owner >= 0) return {MH_ERR_INVALID_ARGUMENT, a + ": duplicate parameter"};
        int slot;
        if (small) {
            if (P.n_rgb >= (uint32_t)kMaxRgbParams) return {MH_ERR_UNSUPPORTED, a + ": too many rgb parameters"};
            slot = (int)P.n_rgb++;
            P.is_rgb[slot] = 1;
        } else {
            if (P.n_bmp >= (uint32_t)kMaxBitmapParams) return {MH_ERR_UNSUPPORTED, a + ": too many bitmap parameters"};
            slot = kMaxRgbParams + (int)P.n_bmp++;
            if (kind == 0) P.bmp_tex = idx;
        }
        P.counts[slot] = cnt;
        if (kind == MH_PARAM_MEDIUM_SIGMA_T && !small)
            for (int ax = 0; ax < 3; ++ax) P.grid_res[slot][ax] = sc.media[idx].grid_res[ax];
        *owner = slot;
        P.slot_of_param[k] = (uint32_t)slot;
    }
    return {};
}

// ---- the slot block (mh_scene::tmp_c) -----------------------------------------
// every slot's buffer padded to whole float4s, one after the other; the bitmap
// slots' part of it is the fused wavefront's texel block (WfBitmapArgs::off, n_floats)
struct SlotBlock {
    size_t off[kMaxParams] = {};  // floats
    size_t total = 0;             // floats, padded (the reduce's extent)
    uint32_t bmp_off[kMaxBitmapParams] = {};  // bitmap slot b from the first bitmap slot's buffer
    uint32_t bmp_floats = 0;
    size_t alloc_floats() const { return std::max<size_t>(total, 1); }  // never an empty allocation
};
inline size_t padded(size_t count) { return (count + 3) / 4 * 4; }
inline SlotBlock slot_block(const std::vector<size_t> &counts) {
    SlotBlock b;
    for (int k = 0; k < kMaxParams; ++k) {
        b.off[k] = b.total;
        b.total += padded(counts[k]);
    }
    for (int i = 0; i < kMaxBitmapParams; ++i) b.bmp_off[i] = (uint32_t)(b.off[kMaxRgbParams + i] - b.off[kMaxRgbParams]);
    b.bmp_floats = (uint32_t)(b.total - b.off[kMaxRgbParams]);
    return b;
}

// ---- the corner blocks (mh_scene::grid_corner) ----------------------------------
// a grid sigma_t slot scatters into a per-cell corner block when its padded
// grid has fewer than 2^32 corners; all blocks together at most 32 GiB, as
// floats (fx: int64, twice the bytes) at most 16 GiB
struct CornerLayout {
    bool use[kMaxParams] = {};
    size_t off[kMaxParams] = {};  // values
    size_t values = 0;
    size_t value_bytes = 4;
    bool fits = false;            // something to allocate, within the limits
    size_t bytes() const { return values * value_bytes; }
};
inline CornerLayout corner_layout(const uint32_t grid_res[kMaxParams][3], bool fx) {
    CornerLayout c;
    for (int k = 0; k < kMaxParams; ++k) {
        const uint32_t *r = grid_res[k];
        c.use[k] = r[0] && (uint64_t)(r[0] + 1) * (r[1] + 1) * (r[2] + 1) < (1ull << 32);
        c.off[k] = c.values;
        if (c.use[k]) c.values += corner_floats(r);
    }
    c.value_bytes = fx ? 8 : 4;
    c.fits = c.values && c.bytes() <= (32ull << 30) && (fx || c.values * 4 <= (16ull << 30));
    return c;
}

// ---- the meta block (mh_scene::grad_meta) -----------------------------------------
// slot_of_tex | is_rgb | bufs | sigma_slot | albedo_slot phase_slot | corner | emitter_slot
// byte offsets, each table 16-byte aligned but phase_slot: the kernels read the
// medium -> g slot table as albedo_slot[n_media + medium]
struct MetaLayout {
    size_t slot = 0, is_rgb = 0, bufs = 0, sigma = 0, albedo = 0, phase = 0, corner = 0, emitter = 0, size = 0;
    // GradArgs::emitter_off: the emitter table from slot_of_tex, 0 selecting
    // the kernel instances without the emitter terms
    uint32_t emitter_off(uint32_t n_emitter_params) const { return n_emitter_params ? (uint32_t)(emitter - slot) : 0u; }
    // what the kernels rely on: the g table exactly n_media entries after the
    // albedo table, and an emitter table that a non-zero offset can name
    bool contracts_hold(size_t n_media, uint32_t n_emitter_params) const {
        return (n_media == 0 || phase == albedo + n_media * 4) &&
               ((emitter_off(n_emitter_params) != 0) == (n_emitter_params != 0));
    }
};
// (a table of a scene without textures, media or emitters holds one entry)
inline MetaLayout meta_layout(size_t n_textures, size_t n_media, size_t n_emitters) {
    auto al16 = [](size_t x) { return (x + 15) / 16 * 16; };
    const size_t nt = std::max<size_t>(n_textures, 1), nm = std::max<size_t>(n_media, 1),
                 ne = std::max<size_t>(n_emitters, 1);
    MetaLayout o;
    o.slot = 0;
    o.is_rgb = al16(nt * 4);
    o.bufs = al16(o.is_rgb + kMaxParams * 4);
    o.sigma = al16(o.bufs + kMaxParams * 8);
    o.albedo = al16(o.sigma + nm * 4);
    o.phase = o.albedo + nm * 4;
    o.corner = al16(o.phase + nm * 4);
    o.emitter = al16(o.corner + kMaxParams * 8);
    o.size = al16(o.emitter + ne * 4);
    return o;
}
// the block's host image: P's tables (build_slots) and the slots' buffers
inline std::vector<uint8_t> meta_image(const MetaLayout &o, const Slots &P, float *const *bufs) {
    std::vector<uint8_t> meta(o.size, 0);
    memcpy(meta.data() + o.slot, P.slot_of_tex.data(), P.slot_of_tex.size() * 4);
    memcpy(meta.data() + o.is_rgb, P.is_rgb.data(), kMaxParams * 4);
    memcpy(meta.data() + o.bufs, bufs, kMaxParams * 8);
    memcpy(meta.data() + o.sigma, P.sigma_slot.data(), P.sigma_slot.size() * 4);
    memcpy(meta.data() + o.albedo, P.albedo_slot.data(), P.albedo_slot.size() * 4);
    memcpy(meta.data() + o.phase, P.phase_slot.data(), P.phase_slot.size() * 4);
    memcpy(meta.data() + o.corner, P.corner.data(), kMaxParams * 8);
    memcpy(meta.data() + o.emitter, P.emitter_slot.data(), P.emitter_slot.size() * 4);
    return meta;
}

}  // namespace slots
}  // namespace mh
