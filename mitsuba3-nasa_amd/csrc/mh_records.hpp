// mh_records.hpp — the table records of a device scene and the layouts the
// host builds them in, in plain C++17 (no HIP include).
//
// mh_device.hpp and mh_shading.hpp (hipcc, gfx950) read these records in the
// kernels; mh_scene_build.hpp (host only) fills them from a scene description.
// Both see one definition: what the kernels also call carries MH_HD, which is
// __host__ __device__ under hipcc and nothing for a host compiler.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/mitsuba_hip.h"

#ifdef __HIP__
#define MH_HD __host__ __device__ inline
#define MH_HD_FORCEINLINE __host__ __device__ inline __attribute__((always_inline))  // HIP's __forceinline__
#else
#define MH_HD inline
#define MH_HD_FORCEINLINE inline
#endif

namespace mh {

constexpr float kInv4Pi = 0.07957747154594766788f;

struct DShape {                 // shading-time shape record
    uint32_t type, bsdf, emitter, face_offset;
    uint32_t vertex_offset, has_normals, has_texcoords, pad;
    float to_world[12];
    float frame_s[4], frame_t[4], frame_n[4];
    float inv_area;
    uint32_t interior, exterior, pad3;  // media (MH_INVALID = none)
};

struct DTexture {
    uint32_t type, width, height, channels;
    uint64_t data_offset;
    uint32_t filter, wrap;
    float value[4];
    float to_uv[8];
};

struct DEmitter {
    uint32_t type, shape, pad0, pad1;
    float radiance[4];
    float direction[4];
    float center[3], radius;   // constant / directional: scene bounding sphere
};

// One record of a tabulated phase function's table (DScene::phase_tab; built
// by mh_scene_set_phase_table from IrregularContinuousDistribution's nodes,
// pdf and cdf, distr_1d.h:916-978).  A medium's table is a header
// {integral, normalization, range.x, range.y} at tab_offset, then one record
// per node i at tab_offset + 1 + i: {nodes[i], pdf[i], cdf[i - 1] (0 for
// i == 0), cdf[i] (cdf[n - 2] for the last node)}, then one more record with
// x = +inf that a search for a value beyond the range may read.  Interval i
// is records i and i + 1: one 32-byte fetch after the search.
struct alignas(16) PhaseRec { float x, y, c_prev, c; };

struct DMedium {
    uint32_t type, phase, flags;
    uint32_t tab_offset;                  // tabulated phase: first record (the header) in DScene::phase_tab;
                                          // blend: where its DBlend starts there
    float g, scale, maj, sigma_t_const;   // maj = scale * max(grid) (heterogeneous.cpp:163)
    float albedo[4];
    uint32_t res[4];
    uint64_t grid_offset;   // first float of the medium's bricked grid (grid_index)
    uint32_t tab_n;         // tabulated phase: nodes (0: no table yet); blend: 1 once it is attached
    uint32_t tab_valid;     // its first | last << 16 interval with positive mass (m_valid)
    float to_local[12];
    float bbox_min[4], bbox_max[4];
    static constexpr bool kFarLookups = false;  // grid_setup: sigma_t is looked up inside the medium's box only
};

// A MH_PHASE_BLEND medium's phase function (BlendPhaseFunction,
// src/phase/blendphase.cpp, two children; mh_scene_set_phase_blend): the
// children as the fields of DMedium that phase_eval / phase_sample read, and
// weight_0 -- a constant, or (has_grid) a one-channel grid of its own in
// DScene::grid, read by grid_eval through res / grid_offset / to_local.  It
// lies in DScene::phase_tab at DMedium::tab_offset, in the place of 8 records,
// ahead of its tabulated children's tables: DScene keeps its size (the
// kernels of scenes without a blend keep their registers), and k_vol_sched
// stages it into LDS with the tables.
struct alignas(16) DBlend {
    uint32_t phase[2];
    float g[2];
    uint32_t tab_offset[2], tab_n[2], tab_valid[2];   // tabulated children: as DMedium's
    float weight;
    uint32_t has_grid;
    uint32_t res[4];
    uint64_t grid_offset, pad;
    float to_local[12];
    static constexpr bool kFarLookups = true;   // grid_setup: looked up outside its box (the medium's scatter points)
};
static_assert(sizeof(DBlend) == 8 * sizeof(PhaseRec), "a DBlend takes 8 records of DScene::phase_tab");
constexpr uint32_t kBlendRecs = 8;

// the kernels index these tables by record: their sizes are part of the device layout
static_assert(sizeof(DShape) == 144 && sizeof(DTexture) == 80 && sizeof(DEmitter) == 64, "shading table records");
static_assert(sizeof(PhaseRec) == 16 && sizeof(DMedium) == 160 && sizeof(DBlend) == 128, "medium and phase records");

// PRBVolpathIntegrator.prepare_scene (prbvolpath.py:76-89), from the media of the shapes
constexpr uint32_t kVolHandleNull = 1u;       // some medium is heterogeneous
constexpr uint32_t kVolNeeHomogeneous = 2u;   // some medium is homogeneous
// not prepare_scene's: some medium's phase function is rayleigh or tabulated
// (launch_vol_sched: volpath's machine with those branches; else the one without)
constexpr uint32_t kVolPhaseExt = 4u;
// some medium's phase function is a blend: the kernels compiled with it (kPhBlend, mh_shading.hpp)
constexpr uint32_t kVolPhaseBlend = 8u;

// ---------------------------------------------------------------------------
// LDS staging of the small shading tables (mh_shading.hpp stage_tables):
// layout and size (host and device agree)
// ---------------------------------------------------------------------------
struct TabLayout {
    uint32_t shapes, bsdf_type, bsdf_tex, textures, emitters, positions, normals, texcoords, faces, total;
};
MH_HD TabLayout tab_layout(uint32_t n_shapes, uint32_t n_bsdfs, uint32_t n_textures,
                           uint32_t n_emitters, uint32_t n_vertices, uint32_t n_faces,
                           bool normals, bool texcoords) {
    auto al = [](uint32_t x) { return (x + 15u) & ~15u; };
    TabLayout L;
    uint32_t o = 0;
    L.shapes = o; o += al(n_shapes * (uint32_t)sizeof(DShape));
    L.bsdf_type = o; o += al(n_bsdfs * 4u);
    L.bsdf_tex = o; o += al(n_bsdfs * 4u);
    L.textures = o; o += al(n_textures * (uint32_t)sizeof(DTexture));
    L.emitters = o; o += al(n_emitters * (uint32_t)sizeof(DEmitter));
    L.positions = o; o += al(n_vertices * 12u);
    L.normals = o; o += normals ? al(n_vertices * 12u) : 0u;
    L.texcoords = o; o += texcoords ? al(n_vertices * 8u) : 0u;
    L.faces = o; o += al(n_faces * 12u);
    L.total = o;
    return L;
}

// Device layout of a density grid (the host API and gradients keep the
// reference's linear (z, y, x) layout; values are unchanged, so lookups are
// bit-exact either way).
//
// 4 x 4 x 4 bricks of 64 floats (256 B), bricks x-fastest, texels x-fastest
// inside a brick.  (Round 5 measured apron tiles -- every lookup in one
// 128-B line at 3.6x the texels -- as neutral: DESIGN.md section 9.)
MH_HD_FORCEINLINE uint64_t grid_index(int32_t x, int32_t y, int32_t z, int32_t rx, int32_t ry) {
    const uint32_t nbx = (uint32_t)(rx + 3) >> 2, nby = (uint32_t)(ry + 3) >> 2;
    const uint64_t brick = ((uint64_t)((uint32_t)z >> 2) * nby + ((uint32_t)y >> 2)) * nbx + ((uint32_t)x >> 2);
    return brick * 64u + ((((uint32_t)z & 3u) << 4) | (((uint32_t)y & 3u) << 2) | ((uint32_t)x & 3u));
}

// the device layout of a density grid (mh_shading.hpp grid_setup: 4^3
// bricks), in floats
inline uint64_t grid_bricked_size(const uint32_t res[3]) {
    return (uint64_t)((res[0] + 3) / 4) * ((res[1] + 3) / 4) * ((res[2] + 3) / 4) * 64u;
}

// linear (z, y, x) grid -> 4^3-brick device layout
inline void grid_to_bricks(const float *src, const uint32_t res[3], float *dst) {
    const int32_t rx = (int32_t)res[0], ry = (int32_t)res[1], rz = (int32_t)res[2];
    std::fill(dst, dst + grid_bricked_size(res), 0.f);
    for (int32_t z = 0; z < rz; ++z)
        for (int32_t y = 0; y < ry; ++y)
            for (int32_t x = 0; x < rx; ++x)
                dst[grid_index(x, y, z, rx, ry)] = src[((uint64_t)z * ry + y) * rx + x];
}

}  // namespace mh
