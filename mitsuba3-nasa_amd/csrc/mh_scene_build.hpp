// mh_scene_build.hpp — a device scene worked out from its description, on the
// host only.
//
// mh_scene_create (mh_api.hip) checks a mh_scene_desc, turns its shapes into
// BVH primitives, lays out the tables the kernels index, and decides what is
// staged into LDS and how deep the traversal stacks are; the phase-function
// calls (mh_scene_set_phase_*) build tables and blend records and place them
// in one buffer.  All of that arithmetic is here: no HIP, no environment, no
// state, results as code plus message, so it is checked without a GPU
// (tools/scene_check.cpp, tests/test_scene_host.py).  mh_api.hip keeps the HIP
// calls and whatever depends on an allocation having succeeded.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/mitsuba_hip.h"
#include "mh_records.hpp"
#include "mh_slots.hpp"

namespace mh {

// ---- BVH builder (host, binned SAH: mh_bvh.cpp) ----------------------------
struct BuildPrim {
    float lo[3], hi[3];   // world AABB
    float rec[12];        // Prim a/b/c payload
    uint32_t shape, prim, type;
};
struct BvhOut {
    std::vector<uint8_t> nodes;  // sizeof(Node) * n_nodes
    std::vector<uint8_t> prims;  // sizeof(Prim) * n_prims (reordered)
    uint32_t n_nodes = 0, n_prims = 0, depth = 0;
};
// max_leaf <= 31 (5-bit leaf count of the per-lane stream engine's stack entries)
void build_bvh(const std::vector<BuildPrim> &in, BvhOut &out, uint32_t max_leaf = 4, float trav_cost = 1.0f);
// BVH4 collapsed from a BVH2 (greedy: open the largest-area inner child until
// four children); depth4 = max Node4 nesting
void collapse_bvh4(const BvhOut &b2, std::vector<uint8_t> &nodes4, uint32_t &n4, uint32_t &depth4);
// the same BVH4 quantised (QNode4, children-contiguous order) + compact
// primitive records (PrimC); false when a box cannot be quantised
bool build_qbvh4(const BvhOut &b2, std::vector<uint8_t> &qnodes, std::vector<uint8_t> &primsc, uint32_t &n4,
                 uint32_t &depth4);

namespace scene {

using Error = slots::Error;

// a + b * c * d does not fit 64 bits
inline bool offset_wraps(uint64_t a, uint32_t b, uint32_t c, uint32_t d) {
    uint64_t n = 0;
    return __builtin_mul_overflow((uint64_t)b * c, (uint64_t)d, &n) || __builtin_add_overflow(a, n, &n);
}

// ---- mh_scene_create: what a description alone gets refused for ------------
// The first failure wins, in this order (a description with several faults
// reports the same one as ever):
//    1. film size
//    2. area emitters (rectangles only), in emitter order
//    3. per shape, in shape order: a mesh's ranges, then its face indices in
//       face order; or an unknown shape type
//    4. per shape, in shape order: the bsdf index, then the medium indices
//    5. per medium, in medium order: the grid's range, its 2^32 texel limit,
//       the HG asymmetry, an unknown phase function, a depolarised rayleigh
//    6. pixel format
//    7. sensor medium
//    8. per bsdf: a diffuse bsdf's texture index
//    9. per texture: a bitmap's range
// and then what used to be trusted (a wrong value reached the device as an
// index, or the host read through a null pointer), each with its own text:
//   10. a NULL table the host reads with a non-zero count: shapes, bsdfs,
//       textures, emitters, media; positions and faces when a mesh has faces;
//       grid_data when a medium is heterogeneous.  (1-9 skip what they cannot
//       read of such a table.  texels is only ever uploaded: NULL means zeros.)
//   11. per shape: the emitter index (MH_INVALID: none)
//   12. the environment emitter's index (MH_INVALID: none)
//   13. per mesh with faces: has_normals / has_texcoords without the array
//   14. per medium / texture: grid_offset + x * y * z and data_offset +
//       w * h * channels beyond 64 bits (5 and 9 compared the wrapped sums)
inline Error validate(const mh_scene_desc &d) {
    const auto invalid = [](const char *m) { return Error{MH_ERR_INVALID_ARGUMENT, std::string("mh_scene_create: ") + m}; };
    const auto unsupported = [](const char *m) { return Error{MH_ERR_UNSUPPORTED, std::string("mh_scene_create: ") + m}; };
    const uint32_t n_shapes = d.shapes ? d.n_shapes : 0, n_bsdfs = d.bsdfs ? d.n_bsdfs : 0,
                   n_textures = d.textures ? d.n_textures : 0, n_emitters = d.emitters ? d.n_emitters : 0,
                   n_media = d.media ? d.n_media : 0;
    if (d.sensor.width == 0 || d.sensor.height == 0) return invalid("film size must be positive");
    for (uint32_t i = 0; i < n_emitters; ++i) {
        const mh_emitter &e = d.emitters[i];
        if (e.type == MH_EMITTER_AREA &&
            (e.shape >= d.n_shapes || (d.shapes && d.shapes[e.shape].type != MH_SHAPE_RECTANGLE)))
            return unsupported("area emitters are supported on rectangles only");
    }
    bool mesh_faces = false, grids = false;
    for (uint32_t si = 0; si < n_shapes; ++si) {
        const mh_shape &sh = d.shapes[si];
        if (sh.type == MH_SHAPE_MESH) {
            if ((uint64_t)sh.face_offset + sh.face_count > d.n_faces ||
                (uint64_t)sh.vertex_offset + sh.vertex_count > d.n_vertices)
                return invalid("mesh range out of bounds");
            mesh_faces |= sh.face_count != 0;
            for (uint32_t f = 0; d.faces && f < sh.face_count; ++f) {
                const uint32_t *fi = d.faces + 3ull * (sh.face_offset + f);
                if (fi[0] >= sh.vertex_count || fi[1] >= sh.vertex_count || fi[2] >= sh.vertex_count)
                    return invalid("face index out of bounds");
            }
        } else if (sh.type != MH_SHAPE_RECTANGLE) {
            return unsupported("unknown shape type");
        }
    }
    for (uint32_t i = 0; i < n_shapes; ++i) {
        const mh_shape &a = d.shapes[i];
        if (a.bsdf >= d.n_bsdfs) return invalid("bsdf index out of bounds");
        if ((a.interior_medium != MH_INVALID && a.interior_medium >= d.n_media) ||
            (a.exterior_medium != MH_INVALID && a.exterior_medium >= d.n_media))
            return invalid("medium index out of bounds");
    }
    for (uint32_t i = 0; i < n_media; ++i) {
        const mh_medium &a = d.media[i];
        grids |= a.type == MH_MEDIUM_HETEROGENEOUS;
        if (a.type == MH_MEDIUM_HETEROGENEOUS &&
            (a.grid_res[0] == 0 || a.grid_res[1] == 0 || a.grid_res[2] == 0 ||
             a.grid_offset + (uint64_t)a.grid_res[0] * a.grid_res[1] * a.grid_res[2] > d.n_grid))
            return invalid("volume grid out of bounds");
        // grid_eval indexes a grid's bricked texels with 32-bit offsets
        if (a.type == MH_MEDIUM_HETEROGENEOUS && grid_bricked_size(a.grid_res) >= (1ull << 32))
            return unsupported("volume grid above 2^32 texels");
        if (a.phase == MH_PHASE_HG && !(a.g > -1.f && a.g < 1.f))
            return Error{MH_ERR_INVALID_ARGUMENT, "The asymmetry parameter must lie in the interval (-1, 1)!"};
        if (a.phase > MH_PHASE_BLEND) return invalid("unknown phase function");
        // rayleigh.cpp:124-126 returns a value that differs from the pdf when
        // depolarization != 0 (the sampling weight is then not 1)
        if (a.phase == MH_PHASE_RAYLEIGH && a.g != 0.f)
            return invalid("the rayleigh phase function is supported with depolarization = 0 only: "
                           "otherwise its value differs from its sampling density and the sampling weight is not 1, "
                           "which the volumetric integrators here do not carry");
    }
    if (d.sensor.pixel_format > MH_PIXEL_XYZA) return invalid("unknown pixel format");
    if (d.sensor.medium != MH_INVALID && d.sensor.medium >= d.n_media) return invalid("sensor medium index out of bounds");
    for (uint32_t i = 0; i < n_bsdfs; ++i)
        if (d.bsdfs[i].type == MH_BSDF_DIFFUSE && d.bsdfs[i].reflectance >= d.n_textures)
            return invalid("texture index out of bounds");
    for (uint32_t i = 0; i < n_textures; ++i) {
        const mh_texture &a = d.textures[i];
        if (a.type == MH_TEX_BITMAP && a.data_offset + (uint64_t)a.width * a.height * a.channels > d.n_texels)
            return invalid("bitmap data out of bounds");
    }
    // ---- formerly trusted ----
    const struct { const void *table; bool read; const char *text; } tables[] = {
        {d.shapes, d.n_shapes != 0, "shapes is NULL with n_shapes > 0"},
        {d.bsdfs, d.n_bsdfs != 0, "bsdfs is NULL with n_bsdfs > 0"},
        {d.textures, d.n_textures != 0, "textures is NULL with n_textures > 0"},
        {d.emitters, d.n_emitters != 0, "emitters is NULL with n_emitters > 0"},
        {d.media, d.n_media != 0, "media is NULL with n_media > 0"},
        {d.positions, mesh_faces, "positions is NULL but a mesh has faces"},
        {d.faces, mesh_faces, "faces is NULL but a mesh has faces"},
        {d.grid_data, grids, "grid_data is NULL but a medium is heterogeneous"},
    };
    for (const auto &t : tables)
        if (t.read && !t.table) return invalid(t.text);
    for (uint32_t i = 0; i < n_shapes; ++i)
        if (d.shapes[i].emitter != MH_INVALID && d.shapes[i].emitter >= d.n_emitters)
            return invalid("shape emitter index out of bounds");
    if (d.environment != MH_INVALID && d.environment >= d.n_emitters)
        return invalid("environment emitter index out of bounds");
    for (uint32_t i = 0; i < n_shapes; ++i) {
        const mh_shape &a = d.shapes[i];
        if (a.type != MH_SHAPE_MESH || a.face_count == 0) continue;
        if (a.has_normals && !d.normals) return invalid("a mesh has_normals but normals is NULL");
        if (a.has_texcoords && !d.texcoords) return invalid("a mesh has_texcoords but texcoords is NULL");
    }
    for (uint32_t i = 0; i < n_media; ++i) {
        const mh_medium &a = d.media[i];
        if (a.type == MH_MEDIUM_HETEROGENEOUS && offset_wraps(a.grid_offset, a.grid_res[0], a.grid_res[1], a.grid_res[2]))
            return invalid("volume grid range wraps 64 bits");
    }
    for (uint32_t i = 0; i < n_textures; ++i) {
        const mh_texture &a = d.textures[i];
        if (a.type == MH_TEX_BITMAP && offset_wraps(a.data_offset, a.width, a.height, a.channels))
            return invalid("bitmap data range wraps 64 bits");
    }
    return {};
}

// ---- primitives for the BVH (rectangles + mesh triangles), in shape order ----
// of a validated description.  Bit contracts of the traversal kernels: a
// rectangle's box is the min / max over its four corners of m0 * cx + m1 * cy +
// m3 per axis (two products, two additions, unfused); a triangle's record is
// v0, e1 = v1 - v0, e2 = v2 - v0 (mesh.h:437).
inline std::vector<BuildPrim> build_prims(const mh_scene_desc &d) {
    size_t n = 0;
    for (uint32_t si = 0; si < d.n_shapes; ++si)
        n += d.shapes[si].type == MH_SHAPE_MESH ? d.shapes[si].face_count : 1u;
    std::vector<BuildPrim> bp;
    bp.reserve(n);
    for (uint32_t si = 0; si < d.n_shapes; ++si) {
        const mh_shape &sh = d.shapes[si];
        if (sh.type == MH_SHAPE_RECTANGLE) {
            BuildPrim p{};
            const float *m = sh.to_world;
            for (int a = 0; a < 3; ++a) { p.lo[a] = INFINITY; p.hi[a] = -INFINITY; }
            const float cs[4][2] = {{-1, -1}, {-1, 1}, {1, -1}, {1, 1}};
            for (auto &c : cs) {
                for (int a = 0; a < 3; ++a) {
                    float q = m[4 * a + 0] * c[0] + m[4 * a + 1] * c[1] + m[4 * a + 3];
                    p.lo[a] = std::min(p.lo[a], q);
                    p.hi[a] = std::max(p.hi[a], q);
                }
            }
            memcpy(p.rec, sh.to_object, sizeof(float) * 12);
            p.shape = si;
            p.prim = MH_INVALID;
            p.type = MH_SHAPE_RECTANGLE;
            bp.push_back(p);
        } else {
            for (uint32_t f = 0; f < sh.face_count; ++f) {
                const uint32_t *fi = d.faces + 3ull * (sh.face_offset + f);
                const float *v[3];
                for (int k = 0; k < 3; ++k) v[k] = d.positions + 3ull * (sh.vertex_offset + fi[k]);
                BuildPrim p{};
                for (int a = 0; a < 3; ++a) {
                    p.lo[a] = std::min(v[0][a], std::min(v[1][a], v[2][a]));
                    p.hi[a] = std::max(v[0][a], std::max(v[1][a], v[2][a]));
                    p.rec[a] = v[0][a];
                    p.rec[4 + a] = v[1][a] - v[0][a];  // e1 (mesh.h:437)
                    p.rec[8 + a] = v[2][a] - v[0][a];  // e2
                }
                p.shape = si;
                p.prim = f;
                p.type = MH_SHAPE_MESH;
                bp.push_back(p);
            }
        }
    }
    return bp;
}

// A leaf-ordered primitive record (Prim, mh_device.hpp) is 16 dwords, the last
// four its info: shape, prim index, type, scene-order key.
constexpr size_t kPrimWords = 16, kPrimShape = 12, kPrimIndex = 13, kPrimKey = 15;

// scene-order key -> (shape, prim) of every primitive (the packet engine
// carries only the key of its running hit)
inline std::vector<uint32_t> key_table(const BvhOut &bvh) {
    std::vector<uint32_t> key_sp(2 * (size_t)bvh.n_prims);
    const uint32_t *w = reinterpret_cast<const uint32_t *>(bvh.prims.data());
    for (size_t i = 0; i < bvh.n_prims; ++i) {
        const uint32_t *q = w + kPrimWords * i;
        key_sp[2 * (size_t)q[kPrimKey]] = q[kPrimShape];
        key_sp[2 * (size_t)q[kPrimKey] + 1] = q[kPrimIndex];
    }
    return key_sp;
}

// pair records of the packet engine: record i interleaves the dwords of
// leaf-ordered primitives i and i + 1 (the last one with itself); only
// scenes small enough for that engine (packet_max primitives) get them
inline std::vector<uint32_t> pair_records(const BvhOut &bvh, uint32_t packet_max) {
    std::vector<uint32_t> pairs(bvh.n_prims <= packet_max ? 2 * kPrimWords * (size_t)bvh.n_prims : 0);
    const uint32_t *w = reinterpret_cast<const uint32_t *>(bvh.prims.data());
    for (uint32_t i = 0; i < pairs.size() / (2 * kPrimWords); ++i) {
        const uint32_t *a = w + kPrimWords * (size_t)i;
        const uint32_t *b = w + kPrimWords * (size_t)std::min(i + 1, bvh.n_prims - 1);
        for (size_t k = 0; k < kPrimWords; ++k) {
            pairs[2 * kPrimWords * (size_t)i + 2 * k] = a[k];
            pairs[2 * kPrimWords * (size_t)i + 2 * k + 1] = b[k];
        }
    }
    return pairs;
}

// ---- the tables the kernels index, from a validated description -------------
struct Records {
    std::vector<DShape> shapes;
    std::vector<DMedium> media;               // maj and the bricked grid_offset included; no phase data yet
    std::vector<uint32_t> bsdf_type, bsdf_tex;
    std::vector<DTexture> textures;
    std::vector<DEmitter> emitters;
    std::vector<float> grid;                  // the media's density grids in the 4^3-brick layout, one after the other
};
inline Records records(const mh_scene_desc &d) {
    Records R;
    R.shapes.resize(d.n_shapes);
    for (uint32_t i = 0; i < d.n_shapes; ++i) {
        const mh_shape &a = d.shapes[i];
        DShape &b = R.shapes[i];
        memset(&b, 0, sizeof(b));
        b.type = a.type; b.bsdf = a.bsdf; b.emitter = a.emitter; b.face_offset = a.face_offset;
        b.vertex_offset = a.vertex_offset; b.has_normals = a.has_normals; b.has_texcoords = a.has_texcoords;
        memcpy(b.to_world, a.to_world, sizeof(b.to_world));
        memcpy(b.frame_s, a.frame_s, 12);
        memcpy(b.frame_t, a.frame_t, 12);
        memcpy(b.frame_n, a.frame_n, 12);
        b.inv_area = a.inv_area;
        b.interior = a.interior_medium;
        b.exterior = a.exterior_medium;
    }
    // media (heterogeneous.cpp / homogeneous.cpp / grid.cpp)
    R.media.resize(d.n_media);
    for (uint32_t i = 0; i < d.n_media; ++i) {
        const mh_medium &a = d.media[i];
        DMedium &b = R.media[i];
        memset(&b, 0, sizeof(b));
        b.type = a.type; b.phase = a.phase; b.flags = a.flags;
        b.g = a.g; b.scale = a.scale; b.sigma_t_const = a.sigma_t_const;
        // m_max_density = m_scale * m_sigmat->max() (heterogeneous.cpp:163), in float
        b.maj = a.type == MH_MEDIUM_HOMOGENEOUS ? a.sigma_t_const * a.scale : a.scale * a.max_density;
        memcpy(b.albedo, a.albedo, 12);
        memcpy(b.res, a.grid_res, 12);
        memcpy(b.to_local, a.grid_to_local, sizeof(b.to_local));
        memcpy(b.bbox_min, a.bbox_min, 12);
        memcpy(b.bbox_max, a.bbox_max, 12);
        if (a.type != MH_MEDIUM_HETEROGENEOUS) continue;
        b.grid_offset = R.grid.size();
        R.grid.resize(R.grid.size() + grid_bricked_size(a.grid_res));
        grid_to_bricks(d.grid_data + a.grid_offset, a.grid_res, R.grid.data() + b.grid_offset);
    }
    R.bsdf_type.resize(d.n_bsdfs);
    R.bsdf_tex.resize(d.n_bsdfs);
    for (uint32_t i = 0; i < d.n_bsdfs; ++i) {
        R.bsdf_type[i] = d.bsdfs[i].type;
        R.bsdf_tex[i] = d.bsdfs[i].reflectance;
    }
    R.textures.resize(d.n_textures);
    for (uint32_t i = 0; i < d.n_textures; ++i) {
        const mh_texture &a = d.textures[i];
        DTexture &b = R.textures[i];
        memset(&b, 0, sizeof(b));
        b.type = a.type; b.width = a.width; b.height = a.height; b.channels = a.channels;
        b.data_offset = a.data_offset; b.filter = a.filter; b.wrap = a.wrap;
        memcpy(b.value, a.value, 12);
        memcpy(b.to_uv, a.to_uv, 24);
    }
    R.emitters.resize(d.n_emitters);
    for (uint32_t i = 0; i < d.n_emitters; ++i) {
        const mh_emitter &a = d.emitters[i];
        DEmitter &b = R.emitters[i];
        memset(&b, 0, sizeof(b));
        b.type = a.type;
        b.shape = a.shape;
        memcpy(b.radiance, a.radiance, 12);
        memcpy(b.direction, a.direction, 12);
        memcpy(b.center, a.scene_center, 12);
        b.radius = a.scene_radius;
    }
    return R;
}

// ---- what is staged where, and how deep the stacks are ------------------------
// what mh_scene_create reads of the build and the environment (its caller fills it)
struct Limits {
    uint32_t packet_max_prims = 0;   // wf_packet_max_prims()
    bool shade_records = false;      // wf_shade_records()
    bool bvh4_off = false;           // env::bvh4_off()
    uint32_t stream_stack = 20;      // env::stream_stack(20): the stream engine's LDS stack entries
    uint32_t stream_threads = 0;     // wf_blocks(CUs) * 256: the threads of the largest stream-kernel grid
};
constexpr size_t kTabLdsMax = 16384, kBvhLdsMax = 32768, kStackLdsMax = 65536;  // bytes
constexpr size_t kStackBlockBytes = 256 * 4;  // one stack entry of every thread of a 256-thread workgroup

struct Facts {
    uint32_t vol_flags = 0;       // kVol*
    uint32_t tab_bytes = 0;       // the shading tables' bytes when they are staged into LDS (<= 16 KiB), else 0
    uint32_t lds_bytes_bvh = 0;   // nodes + prims when they are staged into LDS (<= 32 KiB), else 0
    uint32_t stack_size = 0;      // BVH2 traversal stack entries per lane
    bool too_deep = false;        // that stack beside the staged BVH exceeds a workgroup's 64 KiB of LDS
    bool wide_bvh = false;        // the stream engine's wide BVH is attempted (the BVH stays in global memory)
    bool shade_records = false;   // the fused bounce kernels' shade records are built
    // divided on the host (correctly rounded, as the device's division)
    float inv_width = 0, inv_height = 0, inv_n_emitters = 0, n_emitters_f = 0, env_pdf = 0;
};
inline Facts facts(const mh_scene_desc &d, size_t bvh_node_bytes, size_t bvh_prim_bytes, uint32_t n_prims,
                   uint32_t bvh_depth, const Limits &lim) {
    Facts F;
    for (uint32_t i = 0; i < d.n_shapes; ++i)
        for (uint32_t mm : {d.shapes[i].interior_medium, d.shapes[i].exterior_medium})
            if (mm != MH_INVALID)
                F.vol_flags |= d.media[mm].type == MH_MEDIUM_HOMOGENEOUS ? kVolNeeHomogeneous : kVolHandleNull;
    for (uint32_t i = 0; i < d.n_media; ++i)
        if (d.media[i].phase == MH_PHASE_RAYLEIGH || d.media[i].phase == MH_PHASE_TABULATED)
            F.vol_flags |= kVolPhaseExt;
        else if (d.media[i].phase == MH_PHASE_BLEND)
            F.vol_flags |= kVolPhaseBlend;   // nothing renders until its blend is attached (check_phase_tables)
    const TabLayout TL = tab_layout(d.n_shapes, d.n_bsdfs, d.n_textures, d.n_emitters, d.n_vertices, d.n_faces,
                                    d.normals != nullptr && d.n_vertices, d.texcoords != nullptr && d.n_vertices);
    F.tab_bytes = TL.total <= kTabLdsMax ? TL.total : 0u;  // staged into LDS by the shade kernels
    const size_t bvh_bytes = bvh_node_bytes + bvh_prim_bytes;
    F.lds_bytes_bvh = bvh_bytes <= kBvhLdsMax ? (uint32_t)bvh_bytes : 0u;  // stage into LDS when small
    F.stack_size = bvh_depth + 2;
    F.too_deep = (size_t)F.stack_size * kStackBlockBytes + F.lds_bytes_bvh > kStackLdsMax;
    F.wide_bvh = F.lds_bytes_bvh == 0 && n_prims > 64 && !lim.bvh4_off;
    F.shade_records = lim.shade_records && n_prims <= lim.packet_max_prims && F.tab_bytes != 0;
    F.inv_width = 1.f / (float)d.sensor.width;
    F.inv_height = 1.f / (float)d.sensor.height;
    F.inv_n_emitters = 1.f / (float)d.n_emitters;  // inf for 0: never read then
    F.n_emitters_f = (float)d.n_emitters;
    F.env_pdf = kInv4Pi * F.inv_n_emitters;
    return F;
}
// a wide BVH of nesting depth4 beside a BVH2 stack of stack_size entries: the
// stack both need (3 * depth4 + 2 for the wide one), or 0 when it does not fit
// LDS and the scene keeps the BVH2
inline uint32_t wide_stack_size(uint32_t stack_size, uint32_t depth4) {
    const uint32_t both = std::max(stack_size, 3u * depth4 + 2u);
    return (size_t)both * kStackBlockBytes <= kStackLdsMax ? both : 0u;
}
// the stream engine's stack of a scene with a wide BVH: the first lim.stream_stack
// entries live in LDS, deeper ones in a global overflow region of one column per
// thread (the words to allocate; 0: the whole stack fits under the cap)
inline size_t stack_overflow_words(uint32_t stack_size, const Limits &lim) {
    return lim.stream_stack < stack_size ? (size_t)(stack_size - lim.stream_stack) * lim.stream_threads : 0;
}

// ---- phase functions ------------------------------------------------------------
// The table of a tabulated phase function: what IrregularContinuousDistribution
// ::compute_cdf_scalar builds (distr_1d.h:916-978) -- the interval integrals
// accumulated in double and stored as float, the first and last interval with
// positive mass, integral = cdf[valid.y], normalization = 1 / integral -- in
// the PhaseRec layout (mh_records.hpp).  valid = first | last << 16.
inline Error phase_table(const char *fn, uint32_t n, const float *cost, const float *values,
                         std::vector<PhaseRec> &tab, uint32_t &valid) {
    auto bad = [&](const char *why) { return Error{MH_ERR_INVALID_ARGUMENT, std::string(fn) + why}; };
    if (n < 2) return bad("IrregularContinuousDistribution: needs at least two entries!");
    if (n > 65536) return bad("more than 65536 entries");
    tab.assign((size_t)n + 2, PhaseRec{});
    uint32_t first = MH_INVALID, last = MH_INVALID;
    double integral = 0.;
    for (uint32_t i = 0; i < n; ++i) {
        if (!std::isfinite(cost[i]) || !std::isfinite(values[i])) return bad("entries must be finite");
        if (cost[i] < -1.f || cost[i] > 1.f) return bad("'cost' must lie in [-1, 1]");
        if (values[i] < 0.f) return bad("IrregularContinuousDistribution: entries must be non-negative!");
        PhaseRec &r = tab[1 + i];
        r.x = cost[i];
        r.y = values[i];
        r.c_prev = (float)integral;   // cdf[i - 1]; 0 for i == 0
        if (i + 1 < n) {
            if (!(cost[i + 1] > cost[i]))
                return bad("IrregularContinuousDistribution: node positions must be strictly increasing!");
            const double value = 0.5 * ((double)cost[i + 1] - (double)cost[i]) * ((double)values[i] + (double)values[i + 1]);
            integral += value;
            if (value > 0.) {
                if (first == MH_INVALID) first = i;
                last = i;
            }
        }
        r.c = (float)integral;        // cdf[i]; the last node repeats cdf[n - 2]
    }
    if (first == MH_INVALID) return bad("IrregularContinuousDistribution: no probability mass found!");
    const float total = tab[1 + last].c;   // m_integral = cdf[valid.y]
    if (!(total > 0.f) || !std::isfinite(1.f / total)) return bad("the table's integral is not a normal float");
    tab[0] = PhaseRec{total, 1.f / total, cost[0], cost[n - 1]};
    tab[1 + n] = PhaseRec{std::numeric_limits<float>::infinity(), 0.f, total, total};
    valid = first | (last << 16);
    return {};
}

// a MH_PHASE_BLEND medium's phase function on the host: its device record, its tabulated children's
// tables (they join DScene::phase_tab) and its weight grid in the bricked layout (it joins DScene::grid,
// after the media's own grids)
struct BlendHost {
    bool set = false;
    DBlend rec{};
    std::vector<PhaseRec> tab[2];
    std::vector<float> grid;
};

// a weight grid's n values: finite
inline bool all_finite(const float *v, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i])) return false;
    return true;
}

// mh_scene_set_phase_blend's arguments against the scene's media
inline Error check_blend(const char *fn, const std::vector<DMedium> &media, uint32_t medium, const mh_phase_blend *b) {
    auto bad = [&](const char *why) { return Error{MH_ERR_INVALID_ARGUMENT, std::string(fn) + why}; };
    if (!b) return bad("NULL argument");
    if (medium >= media.size()) return bad("medium index out of bounds");
    if (media[medium].phase != MH_PHASE_BLEND) return bad("the medium's phase function is not MH_PHASE_BLEND");
    for (int c = 0; c < 2; ++c) {
        if (b->phase[c] > MH_PHASE_TABULATED)
            return bad("a child must be MH_PHASE_ISOTROPIC, MH_PHASE_HG, MH_PHASE_RAYLEIGH or MH_PHASE_TABULATED "
                       "(a nested blend is not supported)");
        if (b->phase[c] == MH_PHASE_HG && !(b->g[c] > -1.f && b->g[c] < 1.f))
            return bad("The asymmetry parameter must lie in the interval (-1, 1)!");
        if (b->phase[c] == MH_PHASE_RAYLEIGH && b->g[c] != 0.f)
            return bad("a rayleigh child is supported with depolarization = 0 only");
    }
    if (b->grid_res[0] || b->grid_res[1] || b->grid_res[2]) {
        if (!b->grid_res[0] || !b->grid_res[1] || !b->grid_res[2]) return bad("a weight grid needs three non-zero resolutions");
        if (!b->grid_data) return bad("NULL weight grid data");
        if (grid_bricked_size(b->grid_res) >= (1ull << 32)) return bad("weight grid above 2^32 texels");
        const uint64_t n_grid = (uint64_t)b->grid_res[0] * b->grid_res[1] * b->grid_res[2];
        if (!all_finite(b->grid_data, n_grid) || !all_finite(b->grid_to_local, 12))
            return bad("the weight grid and its transform must be finite");
    } else if (!std::isfinite(b->weight)) {
        return bad("the weight must be finite");
    }
    return {};
}

// a checked blend into its host record (offsets: assemble_phase_data)
inline void set_blend(BlendHost &h, const mh_phase_blend &b) {
    const bool has_grid = b.grid_res[0] || b.grid_res[1] || b.grid_res[2];
    for (int c = 0; c < 2; ++c) {
        // a child that stays tabulated keeps its table (a second call: update() of a child's g or of the weight's form)
        if (!h.set || h.rec.phase[c] != MH_PHASE_TABULATED || b.phase[c] != MH_PHASE_TABULATED) {
            h.tab[c].clear();
            h.rec.tab_valid[c] = 0;
        }
        h.rec.phase[c] = b.phase[c];
        h.rec.g[c] = b.g[c];
    }
    h.set = true;
    h.rec.weight = has_grid ? 0.f : b.weight;
    h.rec.has_grid = has_grid ? 1u : 0u;
    memset(h.rec.res, 0, sizeof(h.rec.res));
    memset(h.rec.to_local, 0, sizeof(h.rec.to_local));
    h.rec.grid_offset = h.rec.pad = 0;
    h.grid.clear();
    if (has_grid) {
        memcpy(h.rec.res, b.grid_res, 12);
        memcpy(h.rec.to_local, b.grid_to_local, sizeof(h.rec.to_local));
        h.grid.resize(grid_bricked_size(b.grid_res));
        grid_to_bricks(b.grid_data, b.grid_res, h.grid.data());
    }
}

// The scene's phase data from its (edited) host copies: all tables -- the
// tabulated media's and the blends' tabulated children's -- and the blends'
// records (each ahead of its children's tables) in one array, `all`; the media
// records and the blends get their offsets into it, a blend medium's tab_n says
// whether it is ready (set, every tabulated child with its table), and, when
// `regrid`, the blends' weight grids get their offsets behind the grid_floats
// floats of the media's own grids (grid_total: the floats of both).
struct PhaseData {
    std::vector<PhaseRec> all;
    uint64_t grid_total = 0;
};
inline Error assemble_phase_data(const char *fn, std::vector<DMedium> &media, const std::vector<std::vector<PhaseRec>> &tabs,
                                 std::vector<BlendHost> &blends, bool regrid, uint64_t grid_floats, PhaseData &out) {
    std::vector<PhaseRec> &all = out.all;
    all.clear();
    out.grid_total = grid_floats;
    for (size_t m = 0; m < media.size(); ++m) {
        DMedium &b = media[m];
        if (!tabs[m].empty()) {
            b.tab_offset = (uint32_t)all.size();
            b.tab_n = (uint32_t)tabs[m].size() - 2u;
            all.insert(all.end(), tabs[m].begin(), tabs[m].end());
        }
        if (b.phase != MH_PHASE_BLEND) continue;
        BlendHost &h = blends[m];
        bool ready = h.set;
        const size_t at = all.size();
        if (h.set) all.resize(at + kBlendRecs);   // its DBlend: filled in below, once the children's offsets are known
        for (int c = 0; c < 2; ++c) {
            h.rec.tab_offset[c] = h.rec.tab_n[c] = 0;
            if (!h.set || h.rec.phase[c] != MH_PHASE_TABULATED) continue;
            if (h.tab[c].empty()) { ready = false; continue; }
            h.rec.tab_offset[c] = (uint32_t)all.size();
            h.rec.tab_n[c] = (uint32_t)h.tab[c].size() - 2u;
            all.insert(all.end(), h.tab[c].begin(), h.tab[c].end());
        }
        b.tab_offset = (uint32_t)at;
        b.tab_n = ready ? 1u : 0u;   // attached: check_phase_tables
        if (regrid && h.set && h.rec.has_grid) {
            h.rec.grid_offset = out.grid_total;
            out.grid_total += h.grid.size();
        }
        if (h.set) memcpy(static_cast<void *>(&all[at]), &h.rec, sizeof(DBlend));
    }
    if (all.size() * sizeof(PhaseRec) >= (1ull << 32))
        return Error{MH_ERR_UNSUPPORTED, std::string(fn) + "the phase tables exceed 4 GiB"};
    return {};
}

// a tabulated medium without its table, or a blend medium without its blend
// (or without a tabulated child's table): the kernels would read null data
inline Error check_phase_tables(const char *fn, const std::vector<DMedium> &media, const std::vector<BlendHost> &blends) {
    for (size_t m = 0; m < media.size(); ++m) {
        if (media[m].phase == MH_PHASE_TABULATED && media[m].tab_n == 0)
            return Error{MH_ERR_INVALID_ARGUMENT, std::string(fn) + ": medium " + std::to_string(m) +
                                                      " has a tabulated phase function but no table "
                                                      "(call mh_scene_set_phase_table after mh_scene_create)"};
        if (media[m].phase == MH_PHASE_BLEND && media[m].tab_n == 0)
            return Error{MH_ERR_INVALID_ARGUMENT,
                         std::string(fn) + ": medium " + std::to_string(m) +
                             (blends[m].set ? " has a blend phase function with a tabulated child but no table for it "
                                              "(call mh_scene_set_phase_blend_table after mh_scene_set_phase_blend)"
                                            : " has a blend phase function but no blend "
                                              "(call mh_scene_set_phase_blend after mh_scene_create)")};
    }
    return {};
}

}  // namespace scene
}  // namespace mh
