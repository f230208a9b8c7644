// mh_api.hip — C-ABI of the MI355X backend (include/mitsuba_hip.h).
//
// Host orchestration only: scene upload, BVH build, chunked launch of the
// render / splat / develop / PRB kernels on the scene's HIP stream.  There is
// no CPU fallback: every compute entry point requires a HIP device and fails
// with MH_ERR_NO_DEVICE otherwise.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include <rocprofiler-sdk-roctx/roctx.h>

#include "mh_device.hpp"
#include "mh_env.hpp"
#include "mh_internal.hpp"
#include "mh_plan.hpp"
#include "mh_shading.hpp"

// The reference's ProfilerPhase scopes (include/mitsuba/core/profiler.h:20-47,
// ScopedPhase -> ITT / NVTX ranges at :81-110) as roctx ranges around the host
// stages (rocprofv3 --marker-trace shows them beside the kernels).
struct ScopedPhase {
    explicit ScopedPhase(const char *name) { roctxRangePushA(name); }
    ~ScopedPhase() { roctxRangePop(); }
    ScopedPhase(const ScopedPhase &) = delete;
    ScopedPhase &operator=(const ScopedPhase &) = delete;
};

using namespace mh;

namespace {

thread_local std::string g_error;
thread_local bool g_call_issued = false;  // the current entry point has passed its argument checks

int set_error(int code, const std::string &msg) {
    g_error = msg;
    return code;
}

// a wait that failed in comm_wait has already reported why (a collective
// failed, its deadline passed, the communicator was aborted): MH_HIP keeps
// that message instead of replacing it by the HIP code's text
thread_local bool g_keep_error = false;

#define MH_HIP(expr)                                                                        \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            if (g_keep_error) {                                                             \
                g_keep_error = false;                                                       \
                return MH_ERR_HIP;                                                          \
            }                                                                               \
            return set_error(MH_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
        }                                                                                   \
    } while (0)

// device memory with one owner: move-only, freed with its owner (a scene's
// buffers with the scene)
struct DevBuf {
    void *ptr = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : ptr(o.ptr), bytes(o.bytes) { o.ptr = nullptr; o.bytes = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            release();
            ptr = o.ptr;
            bytes = o.bytes;
            o.ptr = nullptr;
            o.bytes = 0;
        }
        return *this;
    }
    ~DevBuf() { release(); }
    hipError_t alloc(size_t n) {
        if (n <= bytes && ptr) return hipSuccess;
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
        if (n == 0) return hipSuccess;
        hipError_t e = hipMalloc(&ptr, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
    template <typename T> T *as() const { return reinterpret_cast<T *>(ptr); }
};

uint32_t log2_exact(uint32_t v) {
    for (uint32_t k = 0; k < 32; ++k)
        if ((1u << k) == v) return k;
    return 32;
}

template <typename T>
hipError_t upload(DevBuf &b, const T *src, size_t count, hipStream_t st) {
    size_t bytes = sizeof(T) * count;
    if (bytes == 0) bytes = 16;  // keep a valid pointer
    hipError_t e = b.alloc(bytes);
    if (e != hipSuccess) return e;
    if (src && count) return hipMemcpyAsync(b.ptr, src, sizeof(T) * count, hipMemcpyHostToDevice, st);
    return hipMemsetAsync(b.ptr, 0, bytes, st);
}

// compute units of a device (256, an MI355X's, if the query fails)
int device_cus(int device) {
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    return cus;
}

}  // namespace

int mh_report_error(int code, const std::string &msg) { return set_error(code, msg); }

struct mh_scene {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    DScene S{};
    // device buffers
    DevBuf nodes, nodes4, primsc, stack_ovf, prims, prim_pairs, key_sp, shade_recs, shapes, bsdf_type, bsdf_tex, textures, emitters, positions, normals,
        texcoords, faces, texels, media, grid;
    DevBuf phase_tab;  // the tabulated phase functions' tables, one after the other (DScene::phase_tab)
    std::vector<std::vector<PhaseRec>> h_phase_tabs;  // per medium (empty: none set)
    // the MH_PHASE_BLEND media's phase functions (mh_scene_set_phase_blend): their tables join phase_tab, their
    // weight grids join `grid` after the grid_floats floats of the media's own grids
    using BlendHost = scene::BlendHost;
    std::vector<BlendHost> h_blends;  // per medium
    size_t grid_floats = 0;
    DevBuf work, film_tmp, film4, alpha_px, counters, grad_meta, tmp_a, tmp_b, tmp_c, tmp_d, tmp_e, weights_tmp;
    std::vector<uint8_t> meta_host;  // the bytes last uploaded to grad_meta (upload_slots)
    DevBuf wf_ws, wf_ctr;  // wavefront state (SoA) and per-chunk/bounce queue counters
    DevBuf wf_ws_prb, wf_partial, gw, wf_carry;  // wavefront PRB: dL / adjoint-factor planes, per-block gradient partials
    DevBuf wf_ws_bmp;  // wavefront PRB with a bitmap parameter: vertex records (WfBmp)
    DevBuf wf_ws_det;  // wavefront PRB, MH_FLAG_DETERMINISTIC: per-path gradient sums (WfDet)
    DevBuf pvp_log;    // prbvolpath backward: per-thread NEE-walk step logs (NeeLog)
    DevBuf pvp_main;   // prbvolpath backward: per-thread path logs of the single pass (MainLog)
    DevBuf pvp_ovf;    // prbvolpath backward on the scheduler: overflow lists + their counters
    DevBuf grid_corner;  // prbvolpath backward: per-cell corner blocks of the grid sigma_t slots
    DevBuf fx_word;      // its deterministic pre-pass: the largest |item| (float bits)
    DevBuf bmp_fx;       // the deterministic bitmap scatter's max word + int64 texel sums
    DevBuf replay_fx;    // the deterministic replay kernel: int64 mirror of the slot block (bitmap texels)
    // multi-GPU: the communicator of MH_FLAG_REDUCE (not owned), and the
    // buffers of the sharded entry points (slab W image, staged peer sums,
    // slab gradients)
    mh_comm *comm = nullptr;
    DevBuf shard_w, shard_tmp, shard_g;
    // host mirrors (parameter updates)
    std::vector<DTexture> h_textures;
    std::vector<mh_medium> h_media;
    std::vector<DMedium> h_dmedia;
    std::vector<DEmitter> h_emitters;
    uint32_t n_textures = 0, n_bsdfs = 0, n_shapes = 0, n_media = 0, pixel_format = MH_PIXEL_RGB;
    uint64_t n_texels = 0;
    uint32_t bvh_nodes = 0, bvh_prims = 0, bvh_depth = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<hipEvent_t> evpool;  // per-chunk timing events of mh_render
    // two-stream chunk pipeline of the bitmap PRB wavefront (fork_stream): odd
    // chunks run on stream2 with their own workspace
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    DevBuf wf_ws2, wf_ws_prb2, wf_ws_bmp2, wf_partial2, work2, wf_carry2;
    DevBuf stack_ovf2;  // the stream engine's stack overflow columns of stream2's launches
};

extern "C" {

const char *mh_last_error(void) { return g_error.c_str(); }
uint32_t mh_abi_version(void) { return MH_ABI_VERSION; }

int mh_device_count(int *count) {
    if (!count) return set_error(MH_ERR_INVALID_ARGUMENT, "mh_device_count: count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) n = 0;
    *count = n;
    return MH_OK;
}

static int require_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
        return set_error(MH_ERR_NO_DEVICE,
                         "mitsuba_hip: no HIP device available (hip_ad_rgb requires an MI355X; "
                         "there is no CPU fallback)");
    if (device < 0 || device >= n)
        return set_error(MH_ERR_INVALID_ARGUMENT, "mh_scene_create: device index out of bounds");
    return MH_OK;
}


static int fail(const scene::Error &e) { return set_error(e.code, e.msg); }

// ---- mh_scene_create: the steps, in the order it takes them (mh_scene_build.hpp holds the host arithmetic) ----

// what the host build reads of this library's kernels, the environment and the device
static scene::Limits scene_limits(int device) {
    scene::Limits lim;
    lim.packet_max_prims = wf_packet_max_prims();
    lim.shade_records = wf_shade_records();
    lim.bvh4_off = env::bvh4_off();
    lim.stream_stack = (uint32_t)env::stream_stack(20);
    lim.stream_threads = wf_blocks(device_cus(device)) * 256u;
    return lim;
}

// everything of a scene that is worked out before the device is touched
struct HostScene {
    BvhOut bvh;
    std::vector<uint32_t> key_sp, pairs;
    scene::Records rec;
    scene::Facts facts;
};

static int scene_host_build(const mh_scene_desc *desc, const scene::Limits &lim, HostScene &H) {
    {
        const std::vector<BuildPrim> bp = scene::build_prims(*desc);
        // Leaf size / SAH traversal cost per engine (measured, tools/exp_bvh_leaf.sh):
        // small scenes take the packet engine, where a wave tests every leaf some
        // lane reaches and node visits are the serial part -> few, large leaves
        // (12, C_t = 4); otherwise the per-lane engine (8, C_t = 2).  Leaf counts
        // <= 31 (5-bit field of the stream engine's stack entries); env overrides.
        const bool small = bp.size() <= 64;
        uint32_t max_leaf = (uint32_t)env::bvh_leaf(small ? 12 : 8);
        float ct = (float)env::bvh_ct(small ? 4.0 : 2.0);
        ScopedPhase accel_("InitAccel");
        build_bvh(bp, H.bvh, max_leaf, ct);
    }
    H.key_sp = scene::key_table(H.bvh);
    H.pairs = scene::pair_records(H.bvh, lim.packet_max_prims);
    H.rec = scene::records(*desc);
    H.facts = scene::facts(*desc, H.bvh.nodes.size(), H.bvh.prims.size(), H.bvh.n_prims, H.bvh.depth, lim);
    if (H.facts.too_deep)
        return set_error(MH_ERR_UNSUPPORTED, "mh_scene_create: BVH too deep for the LDS traversal stack");
    return MH_OK;
}

// the scene object on its stream (the caller's, or one of its own)
static int scene_open(int device, void *stream, mh_scene **out) {
    mh_scene *s = new (std::nothrow) mh_scene();
    if (!s) return set_error(MH_ERR_OUT_OF_MEMORY, "mh_scene_create: out of host memory");
    s->device = device;
    if (stream) {
        s->stream = (hipStream_t)stream;
    } else {
        if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) {
            delete s;
            return set_error(MH_ERR_HIP, "mh_scene_create: hipStreamCreate failed");
        }
        s->own_stream = true;
    }
    *out = s;
    return MH_OK;
}

// the BVH and the tables to the device; the host mirrors of what parameter updates edit
static int scene_upload(mh_scene *s, const mh_scene_desc *desc, HostScene &H) {
    hipStream_t st = s->stream;
    s->bvh_nodes = H.bvh.n_nodes;
    s->bvh_prims = H.bvh.n_prims;
    s->bvh_depth = H.bvh.depth;
    if (upload(s->nodes, H.bvh.nodes.data(), H.bvh.nodes.size(), st) != hipSuccess ||
        upload(s->prim_pairs, H.pairs.data(), H.pairs.size(), st) != hipSuccess ||
        upload(s->prims, H.bvh.prims.data(), H.bvh.prims.size(), st) != hipSuccess ||
        upload(s->key_sp, H.key_sp.data(), H.key_sp.size(), st) != hipSuccess)
        return set_error(MH_ERR_OUT_OF_MEMORY, "mh_scene_create: BVH upload failed");
    s->pixel_format = desc->sensor.pixel_format;
    s->h_media.assign(desc->media, desc->media + desc->n_media);
    s->h_dmedia = std::move(H.rec.media);
    s->h_phase_tabs.assign(desc->n_media, {});
    s->h_blends.assign(desc->n_media, {});
    s->h_textures = std::move(H.rec.textures);
    s->h_emitters = std::move(H.rec.emitters);
    s->grid_floats = H.rec.grid.size();
    s->n_media = desc->n_media;
    s->n_textures = desc->n_textures;
    s->n_bsdfs = desc->n_bsdfs;
    s->n_shapes = desc->n_shapes;
    s->n_texels = desc->n_texels;
    const scene::Records &R = H.rec;
    bool ok = upload(s->shapes, R.shapes.data(), R.shapes.size(), st) == hipSuccess &&
              upload(s->bsdf_type, R.bsdf_type.data(), R.bsdf_type.size(), st) == hipSuccess &&
              upload(s->bsdf_tex, R.bsdf_tex.data(), R.bsdf_tex.size(), st) == hipSuccess &&
              upload(s->textures, s->h_textures.data(), s->h_textures.size(), st) == hipSuccess &&
              upload(s->emitters, s->h_emitters.data(), s->h_emitters.size(), st) == hipSuccess &&
              upload(s->positions, desc->positions, 3ull * desc->n_vertices, st) == hipSuccess &&
              upload(s->normals, desc->normals, desc->normals ? 3ull * desc->n_vertices : 0, st) == hipSuccess &&
              upload(s->texcoords, desc->texcoords, desc->texcoords ? 2ull * desc->n_vertices : 0, st) == hipSuccess &&
              upload(s->faces, desc->faces, 3ull * desc->n_faces, st) == hipSuccess &&
              upload(s->texels, desc->texels, desc->n_texels, st) == hipSuccess &&
              upload(s->media, s->h_dmedia.data(), s->h_dmedia.size(), st) == hipSuccess &&
              upload(s->grid, R.grid.data(), R.grid.size(), st) == hipSuccess &&
              s->counters.alloc(256 + 1024) == hipSuccess;  // 32 counters + 8 work heads on own lines
    if (!ok) return set_error(MH_ERR_OUT_OF_MEMORY, "mh_scene_create: device upload failed");
    return MH_OK;
}

// the kernels' view of the uploaded scene (BVH2 only, the whole stack in LDS: scene_wide_bvh may change both)
static void scene_fill(mh_scene *s, const mh_scene_desc *desc, const HostScene &H) {
    const mh_sensor &sn = desc->sensor;
    const scene::Facts &F = H.facts;
    DScene &S = s->S;
    S.nodes = s->nodes.as<Node>();
    S.prims = s->prims.as<Prim>();
    S.key_sp = s->key_sp.as<uint2>();
    S.prim_pairs = s->prim_pairs.as<Prim>();
    S.shapes = s->shapes.as<DShape>();
    S.bsdf_type = s->bsdf_type.as<uint32_t>();
    S.bsdf_tex = s->bsdf_tex.as<uint32_t>();
    S.textures = s->textures.as<DTexture>();
    S.emitters = s->emitters.as<DEmitter>();
    S.positions = s->positions.as<float>();
    S.normals = desc->normals ? s->normals.as<float>() : nullptr;
    S.texcoords = desc->texcoords ? s->texcoords.as<float>() : nullptr;
    S.faces = s->faces.as<uint32_t>();
    S.texels = s->texels.as<float>();
    S.media = s->media.as<DMedium>();
    S.grid = s->grid.as<float>();
    S.phase_tab = nullptr;  // mh_scene_set_phase_table
    S.phase_tab_bytes = S.phase_lds_bytes = 0;
    S.n_media = desc->n_media;
    S.camera_medium = sn.medium;
    S.vol_flags = F.vol_flags;
    S.n_shapes = desc->n_shapes;
    S.n_bsdfs = desc->n_bsdfs;
    S.n_textures = desc->n_textures;
    S.n_vertices = desc->n_vertices;
    S.n_faces = desc->n_faces;
    S.tab_bytes = F.tab_bytes;
    S.n_nodes = H.bvh.n_nodes;
    S.n_prims = H.bvh.n_prims;
    S.n_emitters = desc->n_emitters;
    S.inv_n_emitters = F.inv_n_emitters;
    S.n_emitters_f = F.n_emitters_f;
    S.env_pdf = F.env_pdf;
    S.environment = desc->environment;
    S.stack_size = F.stack_size;
    S.lds_bytes_bvh = F.lds_bytes_bvh;
    S.nodes4 = nullptr;
    S.qnodes = nullptr;
    S.primsc = nullptr;
    S.stream_stack = S.stack_size;
    S.stack_ovf = nullptr;
    S.ovf_threads = 0;
    memcpy(S.cam_to_world, sn.to_world, sizeof(S.cam_to_world));
    memcpy(S.sample_to_camera, sn.sample_to_camera, sizeof(S.sample_to_camera));
    S.near_clip = sn.near_clip;
    S.far_clip = sn.far_clip;
    S.width = sn.width;
    S.height = sn.height;
    S.inv_width = F.inv_width;
    S.inv_height = F.inv_height;
    S.rfilter = sn.rfilter;
    S.rfilter_radius = sn.rfilter_radius;
    memcpy(S.filter_coeff, sn.filter_coeff, sizeof(S.filter_coeff));
    S.sampler_seed = sn.sampler_seed;
    S.shade_recs = nullptr;
}

// Wide BVH for the stream engine when the BVH lives in global memory
// (mh_bvh.cpp collapse_bvh4; MH_BVH4=0 keeps BVH2 everywhere): the float BVH4
// (round 1); MH_BVH4Q=1: the quantised BVH4 + compact primitives (round 4,
// measured slower so far: DESIGN.md §3).  A scene whose wide BVH does not fit
// or cannot be allocated keeps its BVH2.
static void scene_wide_bvh(mh_scene *s, const HostScene &H, const scene::Limits &lim) {
    DScene &S = s->S;
    hipStream_t st = s->stream;
    if (H.facts.wide_bvh) {
        std::vector<uint8_t> n4, pc;
        uint32_t cnt4 = 0, depth4 = 0;
        const bool quant = env::bvh4q() && build_qbvh4(H.bvh, n4, pc, cnt4, depth4);
        if (!quant) collapse_bvh4(H.bvh, n4, cnt4, depth4);
        const uint32_t stack = scene::wide_stack_size(S.stack_size, depth4);
        if (stack != 0 && upload(s->nodes4, n4.data(), n4.size(), st) == hipSuccess &&
            (!quant || upload(s->primsc, pc.data(), pc.size(), st) == hipSuccess)) {
            if (quant) {
                S.qnodes = reinterpret_cast<const QNode4 *>(s->nodes4.ptr);
                S.primsc = reinterpret_cast<const PrimC *>(s->primsc.ptr);
            } else {
                S.nodes4 = reinterpret_cast<const Node4 *>(s->nodes4.ptr);
                // MH_PRIMC=1: the compact 48-B triangle records with the float BVH4
                if (env::primc()) {
                    std::vector<uint8_t> qn, pc2;
                    uint32_t c2 = 0, d2 = 0;
                    if (build_qbvh4(H.bvh, qn, pc2, c2, d2) && upload(s->primsc, pc2.data(), pc2.size(), st) == hipSuccess)
                        S.primsc = reinterpret_cast<const PrimC *>(s->primsc.ptr);
                }
            }
            S.stack_size = stack;
        }
    }
    // The stream engine's stack (round 4): the bound 3 * depth4 + 2 of a
    // wide-BVH traversal (44-50 entries on 1M-4M triangles) put 48 KiB of LDS
    // stack in every 256-thread workgroup and held the trace kernels at 3
    // waves per SIMD; the stacks rays really build stay far shallower
    // (tools/qbvh_stats: at most 14 entries on those meshes).  So the first
    // kStreamStack entries live in LDS and deeper ones in a global overflow
    // region, one column per thread of the largest stream-kernel grid: exact
    // for any depth, and 6 waves per SIMD.  Same box, path 512^2 @ 64 on the
    // 1M / 4M-triangle meshes: 386 / 317 Msamples/s with the full LDS stack,
    // 522 / 434 capped at 12-20 entries (5 waves), 534-538 / 446-451 at 6
    // waves (MH_STREAM_WAVES).  MH_STREAM_STACK overrides the cap.
    S.stream_stack = S.stack_size;
    if (S.lds_bytes_bvh == 0 && (S.nodes4 || S.qnodes)) {
        const size_t words = scene::stack_overflow_words(S.stack_size, lim);
        if (words && upload(s->stack_ovf, (const uint32_t *)nullptr, words, st) == hipSuccess) {
            S.stream_stack = lim.stream_stack;
            S.stack_ovf = s->stack_ovf.as<uint32_t>();
            S.ovf_threads = lim.stream_threads;
        }
    }
}

// shade records of the fused bounce kernels, for the scenes those take (the packet engine's, with
// tables that fit LDS): built on the device from the tables uploaded above (same stream), once --
// no update call changes geometry, a shape's bsdf or emitter, or a bsdf's type or texture index
static int scene_shade_records(mh_scene *s, const HostScene &H) {
    if (!H.facts.shade_records) return MH_OK;
    if (upload(s->shade_recs, (const ShadeRec *)nullptr, H.bvh.n_prims, s->stream) != hipSuccess)
        return set_error(MH_ERR_OUT_OF_MEMORY, "mh_scene_create: shade record allocation failed");
    s->S.shade_recs = s->shade_recs.as<ShadeRec>();
    if (launch_build_shade_recs(s->S, s->shade_recs.as<ShadeRec>(), s->stream) != hipSuccess)
        return set_error(MH_ERR_HIP, "mh_scene_create: shade record kernel failed");
    return MH_OK;
}

static int scene_finish(mh_scene *s) {
    if (hipEventCreate(&s->ev0) != hipSuccess || hipEventCreate(&s->ev1) != hipSuccess)
        return set_error(MH_ERR_HIP, "mh_scene_create: hipEventCreate failed");
    if (hipStreamSynchronize(s->stream) != hipSuccess) return set_error(MH_ERR_HIP, "mh_scene_create: upload sync failed");
    return MH_OK;
}

int mh_scene_create(const mh_scene_desc *desc, int device, void *stream, mh_scene **out) {
    ScopedPhase phase_("InitScene");
    if (!desc || !out) return set_error(MH_ERR_INVALID_ARGUMENT, "mh_scene_create: NULL argument");
    if (desc->abi_version != MH_ABI_VERSION)
        return set_error(MH_ERR_INVALID_ARGUMENT, "mh_scene_create: ABI version mismatch");
    int rc = require_device(device);
    if (rc) return rc;
    if (scene::Error e = scene::validate(*desc)) return fail(e);
    MH_HIP(hipSetDevice(device));
    const scene::Limits lim = scene_limits(device);
    HostScene H;
    if ((rc = scene_host_build(desc, lim, H))) return rc;
    mh_scene *s = nullptr;
    if ((rc = scene_open(device, stream, &s))) return rc;
    rc = scene_upload(s, desc, H);
    if (!rc) {
        scene_fill(s, desc, H);
        scene_wide_bvh(s, H, lim);
        rc = scene_shade_records(s, H);
    }
    if (!rc) rc = scene_finish(s);
    if (rc) {
        mh_scene_destroy(s);  // (leaves the step's message in place)
        return rc;
    }
    *out = s;
    return MH_OK;
}

int mh_scene_destroy(mh_scene *s) {
    if (!s) return MH_OK;
    if (s->comm) comm_attach(s->comm, -1);
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    if (s->stream2) {
        (void)hipStreamSynchronize(s->stream2);
        (void)hipStreamDestroy(s->stream2);
    }
    if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
    if (s->ev_join) (void)hipEventDestroy(s->ev_join);
    for (hipEvent_t e : s->evpool) (void)hipEventDestroy(e);
    if (s->ev0) (void)hipEventDestroy(s->ev0);
    if (s->ev1) (void)hipEventDestroy(s->ev1);
    if (s->own_stream && s->stream) (void)hipStreamDestroy(s->stream);
    delete s;  // frees every DevBuf
    return MH_OK;
}

int mh_scene_set_stream(mh_scene *s, void *stream) {
    if (!s) return set_error(MH_ERR_INVALID_ARGUMENT, "mh_scene_set_stream: NULL scene");
    if (s->own_stream && s->stream == (hipStream_t)stream) return MH_OK;
    if (s->own_stream && s->stream) {
        (void)hipStreamSynchronize(s->stream);
        (void)hipStreamDestroy(s->stream);
    }
    s->own_stream = false;
    s->stream = (hipStream_t)stream;
    return MH_OK;
}

int mh_scene_bvh_info(mh_scene *s, uint32_t *n_nodes, uint32_t *n_prims, uint32_t *depth) {
    if (!s) return set_error(MH_ERR_INVALID_ARGUMENT, "mh_scene_bvh_info: NULL scene");
    if (n_nodes) *n_nodes = s->bvh_nodes;
    if (n_prims) *n_prims = s->bvh_prims;
    if (depth) *depth = s->bvh_depth;
    return MH_OK;
}

int mh_scene_update_rgb(mh_scene *s, uint32_t tex, const float value[3]) {
    if (!s || !value) return set_error(MH_ERR_INVALID_ARGUMENT, "mh_scene_update_rgb: NULL argument");
    if (tex >= s->n_textures || s->h_textures[tex].type != MH_TEX_RGB)
        return set_error(MH_ERR_INVALID_ARGUMENT, "mh_scene_update_rgb: not an rgb texture");
    MH_HIP(hipSetDevice(s->device));
    memcpy(s->h_textures[tex].value, value, 12);
    MH_HIP(hipMemcpyAsync(s->textures.as<DTexture>() + tex, &s->h_textures[tex], sizeof(DTexture),
                          hipMemcpyHostToDevice, s->stream));
    MH_HIP(hipStreamSynchronize(s->stream));
    return MH_OK;
}

// SceneParameters.update of an emitter's radiance / irradiance: the DEmitter
// table behind DScene::emitters (staged into LDS per launch, stage_tables)
int mh_scene_update_emitter(mh_scene *s, uint32_t emitter, const float radiance[3]) {
    if (!s || !radiance) return set_error(MH_ERR_INVALID_ARGUMENT, "mh_scene_update_emitter: NULL argument");
    if (emitter >= s->h_emitters.size())
        return set_error(MH_ERR_INVALID_ARGUMENT, "mh_scene_update_emitter: emitter index out of bounds");
    MH_HIP(hipSetDevice(s->device));
    memcpy(s->h_emitters[emitter].radiance, radiance, 12);
    MH_HIP(hipMemcpyAsync(s->emitters.as<DEmitter>() + emitter, &s->h_emitters[emitter], sizeof(DEmitter),
                          hipMemcpyHostToDevice, s->stream));
    MH_HIP(hipStreamSynchronize(s->stream));
    return MH_OK;
}

int mh_scene_update_texture(mh_scene *s, uint32_t tex, const float *data, uint64_t n) {
    if (!s || !data) return set_error(MH_ERR_INVALID_ARGUMENT, "mh_scene_update_texture: NULL argument");
    if (tex >= s->n_textures || s->h_textures[tex].type != MH_TEX_BITMAP)
        return set_error(MH_ERR_INVALID_ARGUMENT, "mh_scene_update_texture: not a bitmap texture");
    const DTexture &t = s->h_textures[tex];
    if (n != (uint64_t)t.width * t.height * t.channels)
        return set_error(MH_ERR_INVALID_ARGUMENT, "mh_scene_update_texture: size mismatch");
    MH_HIP(hipSetDevice(s->device));
    MH_HIP(hipMemcpyAsync(s->texels.as<float>() + t.data_offset, data, n * 4, hipMemcpyHostToDevice,
                          s->stream));
    MH_HIP(hipStreamSynchronize(s->stream));
    return MH_OK;
}

// SceneParameters.update of a medium's differentiable parameters
// (heterogeneous.cpp:169-178 / homogeneous.cpp:150-155): albedo, homogeneous
// sigma_t, heterogeneous sigma_t grid; the majorant is recomputed as
// parameters_changed does (m_max_density = scale * max(grid)).
int mh_scene_update_medium(mh_scene *s, uint32_t medium, const float *albedo, const float *sigma_t,
                           const float *grid, uint64_t n, uint32_t flags) {
    if (!s) return set_error(MH_ERR_INVALID_ARGUMENT, "mh_scene_update_medium: NULL scene");
    if (medium >= s->n_media) return set_error(MH_ERR_INVALID_ARGUMENT, "mh_scene_update_medium: medium index out of bounds");
    MH_HIP(hipSetDevice(s->device));
    mh_medium &a = s->h_media[medium];
    DMedium &b = s->h_dmedia[medium];
    if (albedo) {
        memcpy(a.albedo, albedo, 12);
        memcpy(b.albedo, albedo, 12);
    }
    if (sigma_t) {
        if (a.type != MH_MEDIUM_HOMOGENEOUS)
            return set_error(MH_ERR_INVALID_ARGUMENT, "mh_scene_update_medium: sigma_t value of a heterogeneous medium (use grid)");
        a.sigma_t_const = b.sigma_t_const = *sigma_t;
        b.maj = b.sigma_t_const * b.scale;
    }
    if (grid) {
        if (a.type != MH_MEDIUM_HETEROGENEOUS)
            return set_error(MH_ERR_INVALID_ARGUMENT, "mh_scene_update_medium: grid of a homogeneous medium");
        if (n != (uint64_t)a.grid_res[0] * a.grid_res[1] * a.grid_res[2])
            return set_error(MH_ERR_INVALID_ARGUMENT, "mh_scene_update_medium: size mismatch");
        // linear copy on the device (staging), then the max and the brick scatter
        MH_HIP(s->tmp_e.alloc(n * 4));
        float *lin = s->tmp_e.as<float>();
        MH_HIP(hipMemcpyAsync(lin, grid, n * 4, (flags & MH_FLAG_DEVICE_POINTERS) ? hipMemcpyDeviceToDevice
                                                                                 : hipMemcpyHostToDevice, s->stream));
        MH_HIP(launch_grid_to_bricks(lin, a.grid_res, s->grid.as<float>() + b.grid_offset, s->stream));
        MH_HIP(s->tmp_b.alloc(16));
        MH_HIP(launch_grid_max(lin, n, s->tmp_b.as<uint32_t>(), s->stream));
        uint32_t key = 0;
        MH_HIP(hipMemcpyAsync(&key, s->tmp_b.ptr, 4, hipMemcpyDeviceToHost, s->stream));
        MH_HIP(hipStreamSynchronize(s->stream));
        a.max_density = ordered_key_to_float(key);
        b.maj = b.scale * a.max_density;
    }
    MH_HIP(hipMemcpyAsync(s->media.as<DMedium>() + medium, &b, sizeof(DMedium), hipMemcpyHostToDevice, s->stream));
    MH_HIP(hipStreamSynchronize(s->stream));
    return MH_OK;
}

// SceneParameters.update of an `hg` medium's asymmetry (hg.cpp:61-63, and its
// constructor's range check): the host description, the host image of the
// device record and the device record itself.  Nothing changes on an error.
int mh_scene_update_medium_phase(mh_scene *s, uint32_t medium, float g) {
    if (!s) return set_error(MH_ERR_INVALID_ARGUMENT, "mh_scene_update_medium_phase: NULL scene");
    if (medium >= s->n_media)
        return set_error(MH_ERR_INVALID_ARGUMENT, "mh_scene_update_medium_phase: medium index out of bounds");
    if (s->h_dmedia[medium].phase != MH_PHASE_HG)
        return set_error(MH_ERR_INVALID_ARGUMENT, "mh_scene_update_medium_phase: the medium's phase function is not MH_PHASE_HG");
    if (!(g > -1.f && g < 1.f))
        return set_error(MH_ERR_INVALID_ARGUMENT, "The asymmetry parameter must lie in the interval (-1, 1)!");
    MH_HIP(hipSetDevice(s->device));
    DMedium b = s->h_dmedia[medium];
    b.g = g;
    MH_HIP(hipMemcpyAsync(s->media.as<DMedium>() + medium, &b, sizeof(DMedium), hipMemcpyHostToDevice, s->stream));
    MH_HIP(hipStreamSynchronize(s->stream));
    s->h_media[medium].g = g;
    s->h_dmedia[medium] = b;
    return MH_OK;
}

// The scene's phase data on the device from its (edited) host copies, laid out
// by scene::assemble_phase_data: the tables and blend records in one buffer, the
// media records with their offsets into it, and, when `regrid`, the grid buffer
// rebuilt as the media's own grids followed by the blends' weight grids.
// Everything is built aside and becomes the scene's only after the last HIP call
// has succeeded: a failure leaves the old buffers and the records that point
// into them in place.
static int commit_phase_data(mh_scene *s, const char *fn, std::vector<DMedium> &media,
                             std::vector<std::vector<PhaseRec>> &tabs, std::vector<mh_scene::BlendHost> &blends,
                             bool regrid) {
    MH_HIP(hipSetDevice(s->device));
    MH_HIP(hipStreamSynchronize(s->stream));  // earlier calls may still read the old tables
    scene::PhaseData P;
    if (scene::Error e = scene::assemble_phase_data(fn, media, tabs, blends, regrid, s->grid_floats, P)) return fail(e);
    DevBuf tab_buf, grid_buf;
    hipError_t e = upload(tab_buf, P.all.data(), P.all.size(), s->stream);
    if (e == hipSuccess && regrid) {
        e = grid_buf.alloc(std::max<uint64_t>(P.grid_total, 4) * sizeof(float));
        if (e == hipSuccess && s->grid_floats)
            e = hipMemcpyAsync(grid_buf.ptr, s->grid.ptr, s->grid_floats * sizeof(float), hipMemcpyDeviceToDevice, s->stream);
        for (uint32_t m = 0; m < s->n_media && e == hipSuccess; ++m)
            if (blends[m].set && blends[m].rec.has_grid)
                e = hipMemcpyAsync(grid_buf.as<float>() + blends[m].rec.grid_offset, blends[m].grid.data(),
                                   blends[m].grid.size() * sizeof(float), hipMemcpyHostToDevice, s->stream);
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(s->media.ptr, media.data(), sizeof(DMedium) * s->n_media, hipMemcpyHostToDevice, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    if (e != hipSuccess) return set_error(MH_ERR_HIP, std::string(fn) + hipGetErrorString(e));  // frees tab_buf, grid_buf
    s->phase_tab = std::move(tab_buf);
    if (regrid) {
        s->grid = std::move(grid_buf);
        s->S.grid = s->grid.as<float>();
    }
    s->h_dmedia = std::move(media);
    s->h_phase_tabs = std::move(tabs);
    s->h_blends = std::move(blends);
    s->S.phase_tab = s->phase_tab.as<PhaseRec>();
    s->S.phase_tab_bytes = (uint32_t)(P.all.size() * sizeof(PhaseRec));
    return MH_OK;
}

int mh_scene_set_phase_table(mh_scene *s, uint32_t medium, uint32_t n, const float *cost, const float *values) {
    const char *fn = "mh_scene_set_phase_table: ";
    auto bad = [&](const char *why) { return set_error(MH_ERR_INVALID_ARGUMENT, std::string(fn) + why); };
    if (!s || !cost || !values) return bad("NULL argument");
    if (medium >= s->n_media) return bad("medium index out of bounds");
    if (s->h_dmedia[medium].phase != MH_PHASE_TABULATED) return bad("the medium's phase function is not MH_PHASE_TABULATED");
    std::vector<PhaseRec> tab;
    uint32_t valid = 0;
    if (scene::Error e = scene::phase_table(fn, n, cost, values, tab, valid)) return fail(e);
    std::vector<DMedium> media = s->h_dmedia;
    std::vector<std::vector<PhaseRec>> tabs = s->h_phase_tabs;
    std::vector<mh_scene::BlendHost> blends = s->h_blends;
    tabs[medium] = std::move(tab);
    media[medium].tab_valid = valid;
    return commit_phase_data(s, fn, media, tabs, blends, false);
}

int mh_scene_set_phase_blend_table(mh_scene *s, uint32_t medium, uint32_t child, uint32_t n, const float *cost,
                                   const float *values) {
    const char *fn = "mh_scene_set_phase_blend_table: ";
    auto bad = [&](const char *why) { return set_error(MH_ERR_INVALID_ARGUMENT, std::string(fn) + why); };
    if (!s || !cost || !values) return bad("NULL argument");
    if (medium >= s->n_media) return bad("medium index out of bounds");
    if (child > 1) return bad("child index out of bounds (a blend has two children)");
    if (s->h_dmedia[medium].phase != MH_PHASE_BLEND) return bad("the medium's phase function is not MH_PHASE_BLEND");
    if (!s->h_blends[medium].set) return bad("the medium has no blend yet (call mh_scene_set_phase_blend first)");
    if (s->h_blends[medium].rec.phase[child] != MH_PHASE_TABULATED) return bad("the child is not MH_PHASE_TABULATED");
    std::vector<PhaseRec> tab;
    uint32_t valid = 0;
    if (scene::Error e = scene::phase_table(fn, n, cost, values, tab, valid)) return fail(e);
    std::vector<DMedium> media = s->h_dmedia;
    std::vector<std::vector<PhaseRec>> tabs = s->h_phase_tabs;
    std::vector<mh_scene::BlendHost> blends = s->h_blends;
    blends[medium].tab[child] = std::move(tab);
    blends[medium].rec.tab_valid[child] = valid;
    return commit_phase_data(s, fn, media, tabs, blends, false);
}

int mh_scene_set_phase_blend(mh_scene *s, uint32_t medium, const mh_phase_blend *b) {
    const char *fn = "mh_scene_set_phase_blend: ";
    if (!s) return set_error(MH_ERR_INVALID_ARGUMENT, std::string(fn) + "NULL argument");
    if (scene::Error e = scene::check_blend(fn, s->h_dmedia, medium, b)) return fail(e);
    std::vector<DMedium> media = s->h_dmedia;
    std::vector<std::vector<PhaseRec>> tabs = s->h_phase_tabs;
    std::vector<mh_scene::BlendHost> blends = s->h_blends;
    scene::set_blend(blends[medium], *b);
    return commit_phase_data(s, fn, media, tabs, blends, true);
}

int mh_scene_update_phase_blend_weight(mh_scene *s, uint32_t medium, const float *data, uint64_t n) {
    const char *fn = "mh_scene_update_phase_blend_weight: ";
    auto bad = [&](const char *why) { return set_error(MH_ERR_INVALID_ARGUMENT, std::string(fn) + why); };
    if (!s || !data) return bad("NULL argument");
    if (medium >= s->n_media) return bad("medium index out of bounds");
    if (s->h_dmedia[medium].phase != MH_PHASE_BLEND || !s->h_blends[medium].set)
        return bad("the medium has no blend (mh_scene_set_phase_blend)");
    mh_scene::BlendHost &h = s->h_blends[medium];
    const uint64_t want = h.rec.has_grid ? (uint64_t)h.rec.res[0] * h.rec.res[1] * h.rec.res[2] : 1ull;
    if (n != want) return bad("size mismatch (a weight grid's x * y * z values, or 1 for a constant weight)");
    if (!scene::all_finite(data, n)) return bad("the weight must be finite");
    MH_HIP(hipSetDevice(s->device));
    MH_HIP(hipStreamSynchronize(s->stream));  // earlier calls may still read the old weight
    if (h.rec.has_grid) {
        std::vector<float> bricked(h.grid.size());
        grid_to_bricks(data, h.rec.res, bricked.data());
        MH_HIP(hipMemcpyAsync(s->grid.as<float>() + h.rec.grid_offset, bricked.data(), bricked.size() * sizeof(float),
                              hipMemcpyHostToDevice, s->stream));
        MH_HIP(hipStreamSynchronize(s->stream));
        h.grid = std::move(bricked);
    } else {
        DBlend rec = h.rec;
        rec.weight = *data;
        MH_HIP(hipMemcpyAsync(s->phase_tab.as<PhaseRec>() + s->h_dmedia[medium].tab_offset, &rec, sizeof(DBlend),
                              hipMemcpyHostToDevice, s->stream));
        MH_HIP(hipStreamSynchronize(s->stream));
        h.rec = rec;
    }
    return MH_OK;
}

static int check_phase_tables(const mh_scene *s, const char *fn) {
    if (scene::Error e = scene::check_phase_tables(fn, s->h_dmedia, s->h_blends)) return fail(e);
    return MH_OK;
}

// Phase-function queries: a grid-stride kernel around phase_sample / phase_eval.
// at: the position-aware calls (sample: in = u1 u2x u2y, pos = the interaction points)
// grad: mh_phase_eval_grad, the evaluation's derivative with respect to an `hg` medium's g
static int phase_query(mh_scene *s, const char *fn, bool sample, bool at, uint32_t medium, uint64_t n, const float *in,
                       const float *pos, float *out, float *pdf, uint32_t flags, bool grad = false) {
    if (!s) return set_error(MH_ERR_INVALID_ARGUMENT, std::string(fn) + ": NULL scene");
    if (medium >= s->n_media) return set_error(MH_ERR_INVALID_ARGUMENT, std::string(fn) + ": medium index out of bounds");
    if (grad && s->h_dmedia[medium].phase != MH_PHASE_HG)
        return set_error(MH_ERR_UNSUPPORTED, std::string(fn) + ": the medium's phase function is not MH_PHASE_HG (other "
                                                               "phase functions' parameters are not differentiable)");
    if (n && (!in || !out || (sample && !pdf) || (at && !pos)))
        return set_error(MH_ERR_INVALID_ARGUMENT, std::string(fn) + ": NULL argument");
    if (n >= (1ull << 32)) return set_error(MH_ERR_INVALID_ARGUMENT, std::string(fn) + ": more than 2^32 - 1 items");
    if (!at && s->h_dmedia[medium].phase == MH_PHASE_BLEND)
        return set_error(MH_ERR_INVALID_ARGUMENT,
                         std::string(fn) + ": a blend phase function needs sample1 and the interaction point "
                                           "(call mh_phase_sample_at / mh_phase_eval_at)");
    if (int rc = check_phase_tables(s, fn)) return rc;
    if (n == 0) return MH_OK;
    MH_HIP(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    const bool dev = flags & MH_FLAG_DEVICE_POINTERS;
    const uint64_t n_in = sample ? (at ? 3 * n : 2 * n) : 3 * n, n_out = sample ? 3 * n : n;
    const float *d_in = in, *d_pos = at ? pos : nullptr;
    float *d_out = out, *d_pdf = pdf;
    if (!dev) {
        MH_HIP(s->tmp_a.alloc(n_in * 4));
        MH_HIP(hipMemcpyAsync(s->tmp_a.ptr, in, n_in * 4, hipMemcpyHostToDevice, st));
        d_in = s->tmp_a.as<float>();
        if (at) {
            MH_HIP(s->tmp_c.alloc(3 * n * 4));
            MH_HIP(hipMemcpyAsync(s->tmp_c.ptr, pos, 3 * n * 4, hipMemcpyHostToDevice, st));
            d_pos = s->tmp_c.as<float>();
        }
        MH_HIP(s->tmp_b.alloc((n_out + n) * 4));
        d_out = s->tmp_b.as<float>();
        d_pdf = d_out + n_out;
    }
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 255) / 256, (uint64_t)device_cus(s->device) * 8);
    if (grad) MH_HIP(launch_phase_eval_grad(s->S, medium, n, d_in, d_out, grid, st));
    else MH_HIP(launch_phase_query(s->S, sample, medium, n, d_in, d_pos, d_out, d_pdf, grid, st));
    if (!dev) {
        MH_HIP(hipMemcpyAsync(out, d_out, n_out * 4, hipMemcpyDeviceToHost, st));
        if (sample) MH_HIP(hipMemcpyAsync(pdf, d_pdf, n * 4, hipMemcpyDeviceToHost, st));
    }
    if (!(flags & MH_FLAG_NO_SYNC) || !dev) MH_HIP(hipStreamSynchronize(st));
    return MH_OK;
}
int mh_phase_sample(mh_scene *s, uint32_t medium, uint64_t n, const float *u, float *wo, float *pdf, uint32_t flags) {
    return phase_query(s, "mh_phase_sample", true, false, medium, n, u, nullptr, wo, pdf, flags);
}
int mh_phase_eval(mh_scene *s, uint32_t medium, uint64_t n, const float *wo, float *value, uint32_t flags) {
    return phase_query(s, "mh_phase_eval", false, false, medium, n, wo, nullptr, value, nullptr, flags);
}
int mh_phase_eval_grad(mh_scene *s, uint32_t medium, uint64_t n, const float *wo, float *dvalue_dg, uint32_t flags) {
    return phase_query(s, "mh_phase_eval_grad", false, false, medium, n, wo, nullptr, dvalue_dg, nullptr, flags, true);
}
int mh_phase_sample_at(mh_scene *s, uint32_t medium, uint64_t n, const float *u, const float *pos, float *wo, float *pdf,
                       uint32_t flags) {
    return phase_query(s, "mh_phase_sample_at", true, true, medium, n, u, pos, wo, pdf, flags);
}
int mh_phase_eval_at(mh_scene *s, uint32_t medium, uint64_t n, const float *wo, const float *pos, float *value,
                     uint32_t flags) {
    return phase_query(s, "mh_phase_eval_at", false, true, medium, n, wo, pos, value, nullptr, flags);
}

// ---------------------------------------------------------------------------
// Render
// ---------------------------------------------------------------------------
static bool has_alpha(uint32_t fmt) {
    return fmt == MH_PIXEL_RGBA || fmt == MH_PIXEL_YA || fmt == MH_PIXEL_XYZA;
}
// channels of the developed image (hdrfilm.cpp:349-372: color_ch + alpha)
static uint32_t image_channels(uint32_t fmt) {
    const uint32_t c = (fmt == MH_PIXEL_Y || fmt == MH_PIXEL_YA) ? 1u : 3u;
    return c + (has_alpha(fmt) ? 1u : 0u);
}
struct Layout {
    uint32_t W, H, spp, spp_pp, n_passes, s_begin, s_end;
};

// ad: the Python ADIntegrator's single wavefront (prb / prbvolpath primal,
// W image and render_backward): prepare() accepts up to exactly 2^32 samples
// and raises beyond (common.py:571-578); lane indices [0, 2^32) are uint32.
// Otherwise SamplingIntegrator::render's passes of <= 2^32 - 1 samples.
static int make_layout(const mh_scene *s, uint32_t spp, uint32_t b, uint32_t e, Layout &L, bool ad) {
    L.W = s->S.width;
    L.H = s->S.height;
    L.spp = spp;
    uint64_t wf = (uint64_t)L.W * L.H * spp, lim = 0xffffffffull;
    L.spp_pp = spp;
    L.n_passes = 1;
    if (ad && wf > (1ull << 32))
        return set_error(MH_ERR_INVALID_ARGUMENT,
                         "The total number of Monte Carlo samples required by this rendering task (" +
                             std::to_string(wf) + ") exceeds 2^32 = 4294967296. Please use fewer samples "
                             "per pixel or render using multiple passes.");
    if (!ad && wf > lim) {  // integrator.cpp:281-295
        L.spp_pp = spp / (uint32_t)((wf + lim - 1) / lim);
        L.n_passes = spp / L.spp_pp;
        if (L.spp_pp * L.n_passes != spp)
            return set_error(MH_ERR_INVALID_ARGUMENT,
                             "render(): sample_count should be a multiple of samples_per_wavefront!");
    }
    if (b == 0 && e == 0) e = L.spp_pp;
    if (e > L.spp_pp || b >= e)
        return set_error(MH_ERR_INVALID_ARGUMENT, "render(): invalid sample slab [spp_begin, spp_end)");
    L.s_begin = b;
    L.s_end = e;
    return MH_OK;
}

static LaneMap lane_map(const Layout &L, uint32_t pixel_begin) {
    LaneMap m;
    m.W = L.W;
    m.spp_pp = L.spp_pp;
    m.log_spp = log2_exact(L.spp_pp);
    m.pixel_begin = pixel_begin;
    m.S = L.s_end - L.s_begin;
    m.s_begin = L.s_begin;
    m.log_S = log2_exact(m.S);
    return m;
}

// The scene's 32-word counter block (zeroed per call): [0] closest rays,
// [1] shadow rays, [2..22] k_vol_sched phase statistics (MH_EXP_VSCNT
// builds), [kCtrInvalid] invalid samples, [kCtrPvpHead] the prbvolpath
// backward's work head; bytes 256.. hold k_vol_sched's 8 queue heads
constexpr int kCtrInvalid = 28;
constexpr int kCtrPvpHead = 30;
// [kCtrBounds]: rows of the splat kernels that would have read past their
// input planes (skipped; the call then fails; none in a correct build)
constexpr int kCtrBounds = 29;
// [kCtrLookups]: k_vol_sched's density-grid lookups (mh_stats.grid_lookups)
constexpr int kCtrLookups = 27;
// [kCtrAuxItems]: bitmap vertex records read by the texel scatter (mh_stats.aux_items)
constexpr int kCtrAuxItems = 26;

// launch_splat with its bounds contract: hipErrorInvalidValue from the host
// check becomes a named error instead of a bare HIP code
#define MH_SPLAT(...)                                                                                   \
    do {                                                                                                \
        hipError_t _e = launch_splat(__VA_ARGS__);                                                      \
        if (_e == hipErrorInvalidValue)                                                                 \
            return set_error(MH_ERR_INVALID_ARGUMENT, "splat: sample planes / film smaller than the "   \
                                                      "chunk's layout (bounds contract of launch_splat)"); \
        if (_e != hipSuccess) return set_error(MH_ERR_HIP, std::string("launch_splat: ") + hipGetErrorString(_e)); \
    } while (0)

// the device half of the contract: a non-zero bounds counter fails the call
static int check_bounds_counter(mh_scene *s, const char *api);
// prbvolpath backward grid (MH_VOL_WAVES = 4 waves / SIMD: 4 workgroups per CU)
// (the log entries per thread: kPvpNeeCap, kPvpMainCap of mh_plan.hpp)
constexpr uint32_t kPvpBlocksPerCu = 4;

static double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

static int check_bounds_counter(mh_scene *s, const char *api) {
    unsigned long long v = 0;
    MH_HIP(hipMemcpy(&v, s->counters.as<unsigned long long>() + kCtrBounds, sizeof(v), hipMemcpyDeviceToHost));
    if (v)
        return set_error(MH_ERR_HIP, std::string(api) + ": " + std::to_string(v) +
                                         " splat rows would have read past the sample planes (skipped)");
    return MH_OK;
}

// k_vol_sched's per-phase statistics of the last launch (MH_EXP_VSCNT
// diagnostic builds, MH_VW_DEBUG=1): wave trips, lanes and shader cycles
static int print_vs_phases(mh_scene *s) {
    unsigned long long c[32];
    MH_HIP(hipMemcpy(c, s->counters.ptr, sizeof(c), hipMemcpyDeviceToHost));
    const char *nm[8] = {"free", "head", "trace", "scatter", "surf", "walk", "post", "end"};
    for (int g = 0; g < 8; ++g)  // groups of k_vol_sched (kNGroups = 8): trips, lanes, cycles
        fprintf(stderr, "vs phase %-8s wave trips %llu, lanes %llu (%.1f per trip), cycles %.3e (%.0f per trip)\n",
                nm[g], c[2 + g], c[10 + g], c[2 + g] ? (double)c[10 + g] / c[2 + g] : 0.0, (double)c[18 + g],
                c[2 + g] ? (double)c[18 + g] / c[2 + g] : 0.0);
    return MH_OK;
}

// MH_FLAG_REDUCE / MH_FLAG_REDUCE_ROOT: the call's result summed over the
// scene's communicator (mh_comm.cpp), stream-ordered behind the kernels that
// produced it.  A film honours MH_FLAG_REDUCE_ROOT (a reduce to rank 0); W
// images and gradients are needed on every rank and are always all-reduced.
static bool wants_reduce(uint32_t flags) { return flags & (MH_FLAG_REDUCE | MH_FLAG_REDUCE_ROOT); }

static int check_reduce_flags(const mh_scene *s, uint32_t flags, const char *api, bool accumulating_output) {
    if (!wants_reduce(flags)) return MH_OK;
    if (!s->comm)
        return set_error(MH_ERR_INVALID_ARGUMENT,
                         std::string(api) + ": MH_FLAG_REDUCE needs a communicator (mh_scene_set_comm)");
    if (accumulating_output && (flags & MH_FLAG_ACCUMULATE))
        return set_error(MH_ERR_INVALID_ARGUMENT,
                         std::string(api) + ": MH_FLAG_REDUCE cannot be combined with MH_FLAG_ACCUMULATE "
                                            "(the sum would count the accumulated content once per rank)");
    return MH_OK;
}

static int reduce_result(mh_scene *s, uint32_t flags, float *buf, uint64_t count, hipStream_t st, bool film) {
    if (!wants_reduce(flags)) return MH_OK;
    const int root = (film && (flags & MH_FLAG_REDUCE_ROOT) && !(flags & MH_FLAG_REDUCE)) ? 0 : -1;
    return comm_reduce_one(s->comm, s->device, buf, count, st, root);
}

// The waits of a call whose collectives are in flight: with MH_FLAG_REDUCE a
// deadline-bounded poll that also watches the communicator's async error and
// aborts it on a failure (mh_comm.cpp comm_wait), so a rank whose peer failed
// before issuing its collective returns an error instead of hanging in
// hipStreamSynchronize; otherwise a plain stream sync.
static hipError_t wait_stream(mh_scene *s, uint32_t flags, hipStream_t st) {
    if (wants_reduce(flags) && s->comm) {
        if (comm_wait(s->comm, st, "collective call") == MH_OK) return hipSuccess;
        g_keep_error = true;  // comm_wait's message stands
        return hipErrorLaunchTimeOut;
    }
    return hipStreamSynchronize(st);
}
#define MH_WAIT(s, flags, st)                                                                         \
    do {                                                                                              \
        if (wants_reduce(flags) && (s)->comm) {                                                       \
            if (int _rc = comm_wait((s)->comm, st, __func__)) return _rc;                             \
        } else {                                                                                      \
            MH_HIP(hipStreamSynchronize(st));                                                         \
        }                                                                                             \
    } while (0)

// MH_FLAG_DEVICE_POINTERS | MH_FLAG_NO_SYNC without stats: nothing is read
// back to the host, so the call returns with its work enqueued on the stream
static bool async_call(uint32_t flags, const mh_stats *stats) {
    return (flags & MH_FLAG_DEVICE_POINTERS) && (flags & MH_FLAG_NO_SYNC) && !stats;
}

// Two-stream chunk pipeline of the wavefront (mh_render and
// mh_render_backward): chunk c runs on the scene's stream (c even) or on
// stream2 (c odd), each with its own workspace (and, for the stream engine of
// large meshes, its own stack overflow columns), and the launches take the
// shared-device grid (wf_blocks), so one chunk's late bounces -- a few paths
// each, the chip mostly idle -- and its splat / texel scatter overlap the
// other chunk's launches.  Only where the chunks share nothing but atomically
// updated outputs: the non-deterministic splat / gradient paths; not with MH_FLAG_SHARED_DEVICE
// (the caller already runs another call beside this one).  A single-chunk
// call of at least kTwoStreamMinSamples samples is split into two chunks.
// MH_WF_STREAMS=1 keeps one stream (measurements, the bench's roofline pass).
// Whether a call uses it is the planner's decision (mh_plan.hpp split_chunks).

// stream2 (created on first use, on the scene's device) waits for the work
// enqueued on st so far
static hipError_t fork_stream(mh_scene *s, hipStream_t st) {
    hipError_t e = hipSuccess;
    if (!s->stream2) e = hipStreamCreateWithFlags(&s->stream2, hipStreamNonBlocking);
    if (e == hipSuccess && !s->ev_fork) e = hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming);
    if (e == hipSuccess && !s->ev_join) e = hipEventCreateWithFlags(&s->ev_join, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(s->ev_fork, st);
    if (e == hipSuccess) e = hipStreamWaitEvent(s->stream2, s->ev_fork, 0);
    return e;
}
// st waits for everything enqueued on stream2
static hipError_t join_stream(mh_scene *s, hipStream_t st) {
    hipError_t e = hipEventRecord(s->ev_join, s->stream2);
    if (e == hipSuccess) e = hipStreamWaitEvent(st, s->ev_join, 0);
    return e;
}

// the splat's fast path: >= 4 spp and the default-sized Gaussian filter
static bool fast_splat(const Layout &L, const DScene &S) {
    return L.spp_pp >= 4 && S.rfilter == MH_RFILTER_GAUSSIAN && S.rfilter_radius > 1.5f && S.rfilter_radius <= 2.5f;
}

// Film storage of mh_render / mh_render_forward: RGBW, or R G B A W for alpha
// films; the kernels splat into an RGBW film (film4, + an alpha plane film_a)
// that an alpha film receives at the end (launch_film_rgbaw).  Zeroed, or
// holding the caller's film with MH_FLAG_ACCUMULATE.
struct FilmStage {
    bool alpha = false;
    size_t bytes = 0;
    float *film = nullptr, *film4 = nullptr, *film_a = nullptr;
};
static int stage_film(mh_scene *s, uint64_t n_px, float *film_rgbw, uint32_t flags, hipStream_t st, FilmStage &F) {
    F.alpha = has_alpha(s->pixel_format);
    F.bytes = n_px * (F.alpha ? 20 : 16);
    F.film = film_rgbw;
    if (!(flags & MH_FLAG_DEVICE_POINTERS)) {
        MH_HIP(s->film_tmp.alloc(F.bytes));
        F.film = s->film_tmp.as<float>();
    }
    if (!(flags & MH_FLAG_ACCUMULATE)) MH_HIP(hipMemsetAsync(F.film, 0, F.bytes, st));
    else if (!(flags & MH_FLAG_DEVICE_POINTERS))
        MH_HIP(hipMemcpyAsync(F.film, film_rgbw, F.bytes, hipMemcpyHostToDevice, st));
    F.film4 = F.film;
    if (F.alpha) {
        MH_HIP(s->film4.alloc(n_px * 16));
        MH_HIP(s->alpha_px.alloc(n_px * 4));
        F.film4 = s->film4.as<float>();
        F.film_a = s->alpha_px.as<float>();
        MH_HIP(hipMemsetAsync(F.film4, 0, n_px * 16, st));
        MH_HIP(hipMemsetAsync(F.film_a, 0, n_px * 4, st));
    }
    return MH_OK;
}

// what the planners (mh_plan.hpp) need to know of a call and its scene
static plan::Facts call_facts(const mh_scene *s, const mh_integrator &in, uint32_t flags, uint64_t n_px, uint32_t spp) {
    plan::Facts f;
    f.type = in.type; f.max_depth = in.max_depth; f.flags = flags;
    f.n_px = n_px; f.spp = spp;
    f.wf_fused = wf_fused(s->S); f.vs_ok = vs_supported(s->S, in); f.vw_ok = vw_supported(s->S, in);
    f.wf_max = wf_max_chunk(); f.vw_max = vw_max_chunk();
    return f;
}

// the argument checks mh_render, mh_render_backward and mh_render_forward share
// (after their own NULL and integrator checks)
static int check_call_args(const mh_scene *s, const mh_integrator *in, uint32_t spp, uint32_t flags, const char *api,
                           bool accumulating_output) {
    if (in->rr_depth == 0)
        return set_error(MH_ERR_INVALID_ARGUMENT, "\"rr_depth\" must be set to a value greater than zero!");
    if (spp == 0) return set_error(MH_ERR_INVALID_ARGUMENT, std::string(api) + ": spp must be > 0");
    if (int rc = check_reduce_flags(s, flags, api, accumulating_output)) return rc;
    return check_phase_tables(s, api);
}

// the scene's pool of timing events, grown to n
static hipError_t grow_evpool(mh_scene *s, size_t n) {
    while (s->evpool.size() < n) {
        hipEvent_t e;
        if (hipError_t err = hipEventCreate(&e)) return err;
        s->evpool.push_back(e);
    }
    return hipSuccess;
}

// ctr[0] += closest rays, ctr[1] += shadow rays of n_blocks blocks of wavefront
// queue counters (one per chunk and pass, ctr_words = wf_counter_words(n_bounces) each)
static void fold_wf_counters(const std::vector<uint32_t> &wctr, size_t ctr_words, size_t n_blocks, uint32_t n_bounces,
                             unsigned long long ctr[2]) {
    const size_t per_bounce = ctr_words / (n_bounces + 1), nseg = per_bounce / 32;
    for (size_t blk = 0; blk < n_blocks; ++blk)
        for (uint32_t b = 0; b < n_bounces; ++b)
            for (size_t sg = 0; sg < nseg; ++sg) {
                const size_t o = ctr_words * blk + per_bounce * b + 32 * sg;
                ctr[0] += wctr[o + 0];
                ctr[1] += wctr[o + 1];
            }
}

static int render_impl(mh_scene *s, const mh_integrator *in, uint32_t seed, uint32_t spp, uint32_t spp_begin,
              uint32_t spp_end, float *film_rgbw, uint32_t flags, mh_stats *stats) {
    ScopedPhase phase_("Render");
    if (!s || !in || !film_rgbw) return set_error(MH_ERR_INVALID_ARGUMENT, "mh_render: NULL argument");
    if (in->type > MH_INTEGRATOR_PRBVOLPATH)
        return set_error(MH_ERR_INVALID_ARGUMENT, "mh_render: unknown integrator");
    if (int rc = check_call_args(s, in, spp, flags, "mh_render", true)) return rc;
    double t_start = now_ms();
    if (stats) *stats = mh_stats{};
    Layout L;
    const bool ad = in->type == MH_INTEGRATOR_PRB || in->type == MH_INTEGRATOR_PRBVOLPATH;
    int rc = make_layout(s, spp, spp_begin, spp_end, L, ad);
    if (rc) return rc;
    MH_HIP(hipSetDevice(s->device));
    g_call_issued = true;  // past argument validation: a failure from here aborts the communicator
    // test hook of the communicator's failure semantics (tests/test_gpu_comm.py,
    // documented in INTEGRATION.md): a reducing call (MH_FLAG_REDUCE) fails
    // after it was issued.  Calls without a collective never read it.
    if ((flags & MH_FLAG_REDUCE) && env::test_fail_after_issue())
        return set_error(MH_ERR_HIP, "MH_TEST_FAIL_AFTER_ISSUE: injected failure");
    hipStream_t st = s->stream;
    const uint64_t n_px = (uint64_t)L.W * L.H;
    FilmStage F;
    if (int rc = stage_film(s, n_px, film_rgbw, flags, st, F)) return rc;
    const bool alpha = F.alpha;
    const size_t film_bytes = F.bytes;
    float *const film = F.film, *const film4 = F.film4, *const film_a = F.film_a;
    MH_HIP(hipMemsetAsync(s->counters.ptr, 0, 256, st));
    const uint32_t S_ = L.s_end - L.s_begin;
    const uint64_t per_pixel = (uint64_t)S_ * L.n_passes;
    // execution mode, chunks and streams (mh_plan.hpp)
    plan::Facts facts = call_facts(s, *in, flags, n_px, S_);
    facts.n_passes = L.n_passes;
    facts.vol_sched = vol_sched_mode();
    const plan::RenderPlan plan = plan::plan_render(facts, env::plan_env(env::Call::Render));
    if (plan.err)
        return set_error(plan.err, "mh_render: the wavefront mode supports the 'path' integrator "
                                   "with 1 <= max_depth <= 64 (several passes: packet-engine scenes) and "
                                   "'volpath' with max_depth <= 1024 (one pass)");
    const bool wavefront = plan.wavefront, volwave = plan.volwave, sched = plan.sched;
    const bool vw_debug = env::vw_debug();
    // (two streams: stream2's launches get their own stack overflow columns, S2 below)
    const uint32_t chunk_px = plan.chunks.chunk_px;
    const bool two = plan.chunks.two;
    const uint64_t plane = (uint64_t)chunk_px * per_pixel;
    MH_HIP(s->work.alloc(plane * (alpha ? 6 : 5) * sizeof(float)));
    if (two) MH_HIP(s->work2.alloc(plane * (alpha ? 6 : 5) * sizeof(float)));
    const bool fast = fast_splat(L, s->S);
    const int coalesce = L.spp_pp >= 4;
    const uint32_t seed_value = s->S.sampler_seed + seed;
    const bool determ = plan.determ;
    unsigned long long *invalid = s->counters.as<unsigned long long>() + kCtrInvalid;
    unsigned long long *bounds = s->counters.as<unsigned long long>() + kCtrBounds;
    float kernel_ms = 0.f, trace_ms = 0.f;
    const size_t n_chunks = (size_t)plan.chunks.n_chunks;
    const uint32_t n_bounces = wavefront ? in->max_depth : 0;
    const size_t ev_per_chunk = 3 + 2 * n_bounces;  // integrator span, bounce spans, splat end
    MH_HIP(grow_evpool(s, ev_per_chunk * n_chunks));
    const size_t ctr_words = wavefront ? wf_counter_words(n_bounces) : 0;  // per pass
    const size_t ctr_per_chunk = ctr_words * L.n_passes;
    const int cus = device_cus(s->device);
    if (wavefront) {
        MH_HIP(s->wf_ws.alloc(wf_workspace_bytes(plane)));
        MH_HIP(s->wf_ctr.alloc(std::max<size_t>(16, ctr_per_chunk * n_chunks * 4)));
        if (L.n_passes > 1) MH_HIP(s->wf_carry.alloc((size_t)chunk_px * S_ * 8));
        if (two) {
            MH_HIP(s->wf_ws2.alloc(wf_workspace_bytes(plane)));
            if (L.n_passes > 1) MH_HIP(s->wf_carry2.alloc((size_t)chunk_px * S_ * 8));
        }
    }
    DScene S2 = s->S;  // stream2's scene view: its own stack overflow columns
    if (two && s->S.stack_ovf) {
        MH_HIP(s->stack_ovf2.alloc(s->stack_ovf.bytes));
        S2.stack_ovf = s->stack_ovf2.as<uint32_t>();
    }
    if (two) MH_HIP(fork_stream(s, st));
    if (volwave && !sched) {
        MH_HIP(s->wf_ws.alloc(vw_workspace_bytes(plane)));
        MH_HIP(s->wf_ctr.alloc((size_t)vw_counter_words(vw_rounds(*in)) * 4));
    }
    size_t chunk = 0;
    for (uint64_t p0 = 0; p0 < n_px; p0 += chunk_px, ++chunk) {
        uint32_t npx = (uint32_t)std::min<uint64_t>(chunk_px, n_px - p0);
        LaneMap lm = lane_map(L, (uint32_t)p0);
        uint64_t n = (uint64_t)npx * S_;
        hipEvent_t *ev = &s->evpool[ev_per_chunk * chunk];
        const bool odd = two && (chunk & 1);
        const hipStream_t cs = odd ? s->stream2 : st;
        DevBuf &work = odd ? s->work2 : s->work;
        MH_HIP(hipEventRecord(ev[0], cs));
        {
        ScopedPhase sample_("SamplingIntegratorSample");
        if (wavefront) {
            MH_HIP(launch_wavefront(odd ? S2 : s->S, *in, lm, seed_value, n, plane, work.as<float>(),
                                    (odd ? s->wf_ws2 : s->wf_ws).ptr, plane,
                                    s->wf_ctr.as<uint32_t>() + ctr_per_chunk * chunk,
                                    n_bounces, wf_blocks(cus, two || (flags & MH_FLAG_SHARED_DEVICE) != 0), ev + 2, cs,
                                    L.n_passes,
                                    L.n_passes > 1 ? (odd ? s->wf_carry2 : s->wf_carry).as<uint64_t>() : nullptr,
                                    alpha));
        } else if (sched) {
            MH_HIP(launch_vol_sched(s->S, *in, lm, seed_value, n, plane, s->work.as<float>(), vs_blocks(cus),
                                    s->counters.as<unsigned long long>(), st, alpha));
        } else if (volwave) {
            MH_HIP(launch_volwave(s->S, *in, lm, seed_value, n, plane, s->work.as<float>(), s->wf_ws.ptr, plane,
                                  s->wf_ctr.as<uint32_t>(), vw_blocks(cus), s->counters.as<unsigned long long>(),
                                  st, alpha));
        } else {
            MH_HIP(launch_render(s->S, *in, lm, seed_value, L.n_passes, n, plane, s->work.as<float>(),
                                 s->counters.as<unsigned long long>(), st, alpha));
        }
        }
        MH_HIP(hipEventRecord(ev[1], cs));
        ScopedPhase put_("ImageBlockPut");
        MH_SPLAT(s->S, lm, kSplatFilm, fast, npx, L.n_passes, n, plane, work.as<float>(), film4,
                 seed_value, coalesce, cs, invalid, determ, work.bytes / 4, n_px * 4, bounds);
        if (alpha)
            MH_SPLAT(s->S, lm, kSplatAlpha, fast, npx, L.n_passes, n, plane, work.as<float>(), film_a,
                     seed_value, coalesce, cs, nullptr, determ, work.bytes / 4, n_px, bounds);
        MH_HIP(hipEventRecord(ev[ev_per_chunk - 1], cs));
    }
    if (two) MH_HIP(join_stream(s, st));
    if (alpha) MH_HIP(launch_film_rgbaw(n_px, film4, film_a, film, st));
    if (int rc = reduce_result(s, flags, film, film_bytes / 4, st, true)) return rc;
    if (!(flags & MH_FLAG_DEVICE_POINTERS))
        MH_HIP(hipMemcpyAsync(film_rgbw, film, film_bytes, hipMemcpyDeviceToHost, st));
    // asynchronous call (device film, no stats): return once the work is
    // enqueued on the scene's stream, as a stream-ordered library op does
    if (async_call(flags, stats)) return MH_OK;
    if (!stats && !vw_debug) {  // nothing to read back: the call's own sync + the bounds word
        MH_WAIT(s, flags, st);
        return check_bounds_counter(s, "mh_render");
    }
    unsigned long long ctr[2] = {0, 0}, n_invalid = 0, n_lookups = 0;
    std::vector<uint32_t> wctr;
    if (wavefront) {
        wctr.resize(ctr_per_chunk * n_chunks);
        MH_HIP(hipMemcpyAsync(wctr.data(), s->wf_ctr.ptr, wctr.size() * 4, hipMemcpyDeviceToHost, st));
    } else {
        MH_HIP(hipMemcpyAsync(ctr, s->counters.ptr, sizeof(ctr), hipMemcpyDeviceToHost, st));
    }
    unsigned long long iv[2] = {0, 0};  // [kCtrInvalid], [kCtrBounds]
    static_assert(kCtrBounds == kCtrInvalid + 1, "one read-back of both words");
    MH_HIP(hipMemcpyAsync(iv, invalid, sizeof(iv), hipMemcpyDeviceToHost, st));
    if (sched)
        MH_HIP(hipMemcpyAsync(&n_lookups, s->counters.as<unsigned long long>() + kCtrLookups, 8,
                              hipMemcpyDeviceToHost, st));
    MH_WAIT(s, flags, st);  // the stats counters are read back
    n_invalid = iv[0];
    if (iv[1])
        return set_error(MH_ERR_HIP, "mh_render: " + std::to_string(iv[1]) +
                                         " splat rows would have read past the sample planes (skipped)");
    float splat_ms = 0.f;
    for (size_t c = 0; c < n_chunks; ++c) {
        hipEvent_t *ev = &s->evpool[ev_per_chunk * c];
        float ms = 0.f;
        MH_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        kernel_ms += ms;
        MH_HIP(hipEventElapsedTime(&ms, ev[1], ev[ev_per_chunk - 1]));
        splat_ms += ms;
        // the fused bounce kernels are timed as one span (launch_wavefront_pass)
        const uint32_t pairs = wavefront ? (facts.wf_fused || L.n_passes > 1 ? 1u : n_bounces) : 0u;
        for (uint32_t b = 0; b < pairs; ++b) {
            MH_HIP(hipEventElapsedTime(&ms, ev[2 + 2 * b], ev[3 + 2 * b]));
            trace_ms += ms;
        }
    }
    if (wavefront) fold_wf_counters(wctr, ctr_words, n_chunks * L.n_passes, n_bounces, ctr);
    if (sched && vw_debug)  // MH_EXP_VSCNT builds: wave trips per phase
        if (int rc2 = print_vs_phases(s)) return rc2;
    if (volwave && !sched && vw_debug) {  // per-round queue sizes (+ MH_EXP_VWCNT builds: trips / steps)
        const uint32_t R = vw_rounds(*in), W = vw_counter_words(R) / (R + 1);
        std::vector<uint32_t> c((size_t)W * (R + 1));
        MH_HIP(hipMemcpy(c.data(), s->wf_ctr.ptr, c.size() * 4, hipMemcpyDeviceToHost));
        for (uint32_t r = 1; r <= R; ++r) {
            unsigned long long q = 0, trips = 0, steps = 0, it_m = 0, it_w = 0;
            for (uint32_t g = 0; g < W / 32; ++g) {
                const uint32_t *w = &c[(size_t)W * r + 32 * g];
                q += w[0];
                trips += w[2] | ((unsigned long long)w[3] << 32);
                steps += w[4] | ((unsigned long long)w[5] << 32);
                it_m += w[6];
                it_w += w[7];
            }
            if (q || trips) fprintf(stderr, "vw round %u: walks %llu, main trips %llu (wave iters %llu), walk steps %llu (wave iters %llu)\n",
                                    r - 1, q, trips, it_m, steps, it_w);
        }
    }
    if (stats) {
        stats->samples = n_px * per_pixel;
        stats->rays_closest = ctr[0];
        stats->rays_shadow = ctr[1];
        stats->bounces = ctr[0];
        stats->ms_total = now_ms() - t_start;
        stats->ms_kernel = kernel_ms;
        // volpath on the phase scheduler: its k_vol_sched launches (one per chunk)
        stats->ms_trace = sched ? kernel_ms : trace_ms;
        stats->n_trace_launches = wavefront ? (uint64_t)n_chunks * n_bounces * L.n_passes : sched ? n_chunks : 0;
        stats->mode = plan.mode;
        stats->invalid_samples = (uint32_t)std::min<unsigned long long>(n_invalid, 0xffffffffull);
        stats->grid_lookups = n_lookups;
        stats->aux_items = n_px * per_pixel;
        stats->ms_aux = splat_ms;
        stats->n_aux_launches = n_chunks;
    }
    return MH_OK;
}

int mh_render_samples(mh_scene *s, const mh_integrator *in, uint32_t seed, uint32_t spp,
                      uint32_t spp_begin, uint32_t spp_end, float *out, uint32_t flags) {
    ScopedPhase phase_("Render");
    if (!s || !in || !out) return set_error(MH_ERR_INVALID_ARGUMENT, "mh_render_samples: NULL argument");
    if (in->type > MH_INTEGRATOR_PRBVOLPATH)
        return set_error(MH_ERR_UNSUPPORTED, "mh_render_samples: unsupported integrator");
    if (spp == 0 || in->rr_depth == 0) return set_error(MH_ERR_INVALID_ARGUMENT, "mh_render_samples: bad arguments");
    if (int rc = check_phase_tables(s, "mh_render_samples")) return rc;
    Layout L;
    const bool ad = in->type == MH_INTEGRATOR_PRB || in->type == MH_INTEGRATOR_PRBVOLPATH;
    int rc = make_layout(s, spp, spp_begin, spp_end, L, ad);
    if (rc) return rc;
    if (L.n_passes != 1) return set_error(MH_ERR_UNSUPPORTED, "mh_render_samples: single pass only");
    MH_HIP(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    const uint64_t n = (uint64_t)L.W * L.H * (L.s_end - L.s_begin);
    const bool alpha = has_alpha(s->pixel_format);
    const size_t out_bytes = n * (alpha ? 24 : 20);
    float *dst = out;
    if (!(flags & MH_FLAG_DEVICE_POINTERS)) {
        MH_HIP(s->tmp_a.alloc(out_bytes));
        dst = s->tmp_a.as<float>();
    }
    MH_HIP(hipMemsetAsync(s->counters.ptr, 0, 256, st));
    LaneMap lm = lane_map(L, 0);
    if ((flags & MH_FLAG_WAVEFRONT) && vs_supported(s->S, *in) && vol_sched_mode()) {
        MH_HIP(launch_vol_sched(s->S, *in, lm, s->S.sampler_seed + seed, n, n, dst, vs_blocks(device_cus(s->device)),
                                s->counters.as<unsigned long long>(), st, alpha));
    } else if ((flags & MH_FLAG_WAVEFRONT) && vw_supported(s->S, *in)) {
        MH_HIP(s->wf_ws.alloc(vw_workspace_bytes(n)));
        MH_HIP(s->wf_ctr.alloc((size_t)vw_counter_words(vw_rounds(*in)) * 4));
        MH_HIP(launch_volwave(s->S, *in, lm, s->S.sampler_seed + seed, n, n, dst, s->wf_ws.ptr, n,
                              s->wf_ctr.as<uint32_t>(), vw_blocks(device_cus(s->device)),
                              s->counters.as<unsigned long long>(), st, alpha));
    } else if (flags & MH_FLAG_WAVEFRONT) {
        if (in->type != MH_INTEGRATOR_PATH || in->max_depth == 0 || in->max_depth > 64)
            return set_error(MH_ERR_UNSUPPORTED, "mh_render_samples: wavefront mode needs 'path' (1 <= max_depth <= 64) "
                                                 "or 'volpath' (max_depth <= 1024)");
        MH_HIP(s->wf_ws.alloc(wf_workspace_bytes(n)));
        MH_HIP(s->wf_ctr.alloc(std::max<size_t>(16, 4 * (size_t)wf_counter_words(in->max_depth))));
        MH_HIP(launch_wavefront(s->S, *in, lm, s->S.sampler_seed + seed, n, n, dst, s->wf_ws.ptr, n,
                                s->wf_ctr.as<uint32_t>(), in->max_depth, wf_blocks(device_cus(s->device)), nullptr,
                                st, 1, nullptr, alpha));
    } else {
        MH_HIP(launch_render(s->S, *in, lm, s->S.sampler_seed + seed, 1, n, n, dst,
                             s->counters.as<unsigned long long>(), st, alpha));
    }
    if (!(flags & MH_FLAG_DEVICE_POINTERS))
        MH_HIP(hipMemcpyAsync(out, dst, out_bytes, hipMemcpyDeviceToHost, st));
    MH_HIP(hipStreamSynchronize(st));
    return MH_OK;
}

int mh_develop(mh_scene *s, const float *film_rgbw, float *image_rgb, uint32_t flags) {
    if (!s || !film_rgbw || !image_rgb) return set_error(MH_ERR_INVALID_ARGUMENT, "mh_develop: NULL argument");
    MH_HIP(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    const uint64_t n_px = (uint64_t)s->S.width * s->S.height;
    const uint32_t fmt = s->pixel_format, ch = image_channels(fmt);
    const size_t film_bytes = n_px * (has_alpha(fmt) ? 20 : 16);
    if (flags & MH_FLAG_DEVICE_POINTERS) {
        MH_HIP(launch_develop(n_px, film_rgbw, image_rgb, fmt, st));
        if (!(flags & MH_FLAG_NO_SYNC)) MH_HIP(hipStreamSynchronize(st));
        return MH_OK;
    }
    MH_HIP(s->tmp_a.alloc(film_bytes));
    MH_HIP(s->tmp_b.alloc(n_px * 4 * ch));
    MH_HIP(hipMemcpyAsync(s->tmp_a.ptr, film_rgbw, film_bytes, hipMemcpyHostToDevice, st));
    MH_HIP(launch_develop(n_px, s->tmp_a.as<float>(), s->tmp_b.as<float>(), fmt, st));
    MH_HIP(hipMemcpyAsync(image_rgb, s->tmp_b.ptr, n_px * 4 * ch, hipMemcpyDeviceToHost, st));
    MH_HIP(hipStreamSynchronize(st));
    return MH_OK;
}

// ---------------------------------------------------------------------------
// PRB backward
// ---------------------------------------------------------------------------
static int prb_weights_impl(mh_scene *s, uint32_t seed, uint32_t spp, uint32_t spp_begin, uint32_t spp_end,
                   float *weights, uint32_t flags) {
    ScopedPhase phase_("ImageBlockPut");
    if (!s || !weights) return set_error(MH_ERR_INVALID_ARGUMENT, "mh_prb_weights: NULL argument");
    if (spp == 0) return set_error(MH_ERR_INVALID_ARGUMENT, "mh_prb_weights: spp must be > 0");
    if (int rc = check_reduce_flags(s, flags, "mh_prb_weights", true)) return rc;
    Layout L;
    int rc = make_layout(s, spp, spp_begin, spp_end, L, true);
    if (rc) return rc;
    MH_HIP(hipSetDevice(s->device));
    g_call_issued = true;  // past argument validation: a failure from here aborts the communicator
    hipStream_t st = s->stream;
    const uint64_t n_px = (uint64_t)L.W * L.H;
    float *w = weights;
    if (!(flags & MH_FLAG_DEVICE_POINTERS)) {
        MH_HIP(s->weights_tmp.alloc(n_px * 4));
        w = s->weights_tmp.as<float>();
    }
    if (!(flags & MH_FLAG_ACCUMULATE)) MH_HIP(hipMemsetAsync(w, 0, n_px * 4, st));
    LaneMap lm = lane_map(L, 0);
    const uint32_t S_ = L.s_end - L.s_begin;
    MH_SPLAT(s->S, lm, kSplatWeights, fast_splat(L, s->S), (uint32_t)n_px, 1, n_px * S_, 0, nullptr, w,
             s->S.sampler_seed + seed, L.spp_pp >= 4, st, nullptr, plan::deterministic(flags, env::deterministic()),
             0, n_px, nullptr);
    if (int rc = reduce_result(s, flags, w, n_px, st, false)) return rc;
    if (!(flags & MH_FLAG_DEVICE_POINTERS))
        MH_HIP(hipMemcpyAsync(weights, w, n_px * 4, hipMemcpyDeviceToHost, st));
    if (!async_call(flags, nullptr)) MH_WAIT(s, flags, st);
    return MH_OK;
}

// ---------------------------------------------------------------------------
// Differentiated parameters -> slots, their buffers and the meta block: the
// assignment and every layout are mh_slots.hpp's (host only); here they meet
// the scene and the device
// ---------------------------------------------------------------------------
using slots::Slots;

static int build_slots(const mh_scene *s, uint32_t n_params, const uint32_t *param_tex, bool vol, const char *api,
                       const char *method, Slots &P) {
    slots::SceneFacts sc;
    for (uint32_t t = 0; t < s->n_textures; ++t) {
        const DTexture &tx = s->h_textures[t];
        sc.textures.push_back({tx.type, (size_t)tx.width * tx.height * tx.channels});
    }
    for (uint32_t m = 0; m < s->n_media; ++m) {
        const mh_medium &md = s->h_media[m];
        sc.media.push_back({md.type, {md.grid_res[0], md.grid_res[1], md.grid_res[2]}, s->h_dmedia[m].phase == MH_PHASE_HG});
    }
    sc.n_emitters = s->h_emitters.size();
    const slots::Error err = slots::build_slots(sc, n_params, param_tex, vol, api, method, P);
    return err ? set_error(err.code, err.msg) : MH_OK;
}

// per-slot device buffers (s->tmp_c, zeroed: blk = slots::slot_block(P.counts)) and the meta block (s->grad_meta)
// corners: the grid sigma_t slots scatter into per-cell corner blocks
// (s->grid_corner, zeroed; launch_corner_gather after the backward) unless
// MH_GRID_CORNER=0, the block would exceed its limits (slots::corner_layout) or cannot be allocated
// fx: MH_FLAG_DETERMINISTIC -- int64 corner blocks (twice the bytes), which
// are then required (no direct-atomic fallback)
static hipError_t upload_slots(mh_scene *s, Slots &P, const slots::SlotBlock &blk, hipStream_t st,
                               std::vector<float *> &bufs, GradArgs &ga, bool corners = false, bool fx = false) {
    hipError_t e = s->tmp_c.alloc(blk.alloc_floats() * 4);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(s->tmp_c.ptr, 0, blk.alloc_floats() * 4, st);
    if (e != hipSuccess) return e;
    bufs.assign(kMaxParams, nullptr);
    for (int k = 0; k < kMaxParams; ++k) bufs[k] = P.counts[k] ? s->tmp_c.as<float>() + blk.off[k] : nullptr;
    P.corner.assign(kMaxParams, nullptr);
    P.fx = false;
    if (corners && (fx || !env::grid_corner_off())) {
        const slots::CornerLayout C = slots::corner_layout(P.grid_res, fx);
        if (C.fits && s->grid_corner.alloc(C.bytes()) == hipSuccess) {
            e = hipMemsetAsync(s->grid_corner.ptr, 0, C.bytes(), st);
            if (e != hipSuccess) return e;
            for (int k = 0; k < kMaxParams; ++k)
                if (C.use[k])
                    P.corner[k] = reinterpret_cast<float *>(s->grid_corner.as<uint8_t>() + C.off[k] * C.value_bytes);
            P.fx = fx;
        } else {
            (void)hipGetLastError();
        }
    }
    const slots::MetaLayout o = slots::meta_layout(s->n_textures, s->n_media, s->h_emitters.size());
    if (!o.contracts_hold(s->n_media, P.n_emitter_params)) return hipErrorInvalidValue;
    P.meta = slots::meta_image(o, P, bufs.data());
    // uploaded only when it changes (a new parameter set or reallocated slot
    // buffers), then with a stream sync; repeated calls with the same
    // parameters stay asynchronous
    if (!(s->grad_meta.ptr && s->meta_host == P.meta)) {
        e = s->grad_meta.alloc(o.size);
        if (e != hipSuccess) return e;
        e = hipMemcpyAsync(s->grad_meta.ptr, P.meta.data(), o.size, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
        e = hipStreamSynchronize(st);
        if (e != hipSuccess) return e;
        s->meta_host = P.meta;
    }
    const uint8_t *mb = s->grad_meta.as<uint8_t>();
    ga.slot_of_tex = reinterpret_cast<const int32_t *>(mb + o.slot);
    ga.is_rgb = reinterpret_cast<const uint32_t *>(mb + o.is_rgb);
    ga.bufs = reinterpret_cast<float *const *>(mb + o.bufs);
    ga.n_rgb = P.n_rgb;
    ga.sigma_slot = P.n_medium_params ? reinterpret_cast<const int32_t *>(mb + o.sigma) : nullptr;
    ga.albedo_slot = P.n_medium_params ? reinterpret_cast<const int32_t *>(mb + o.albedo) : nullptr;
    ga.emitter_off = o.emitter_off(P.n_emitter_params);
    ga.n_phase_g = P.n_phase_params;
    bool any_corner = false;
    for (float *c : P.corner) any_corner = any_corner || c;
    ga.corner = any_corner ? reinterpret_cast<float *const *>(mb + o.corner) : nullptr;
    ga.hot_med = ga.hot_sigma = ga.hot_albedo = -1;
    ga.hot_buf = ga.hot_corner = nullptr;
    for (size_t m = 0; m < P.sigma_slot.size() && P.n_medium_params; ++m) {
        if (P.sigma_slot[m] < 0 && P.albedo_slot[m] < 0) continue;
        ga.hot_med = (int32_t)m;
        ga.hot_sigma = P.sigma_slot[m];
        ga.hot_albedo = P.albedo_slot[m];
        if (ga.hot_sigma >= 0) {
            ga.hot_buf = bufs[ga.hot_sigma];
            ga.hot_corner = P.corner[ga.hot_sigma];
        }
        break;
    }
    return hipSuccess;
}

// ---------------------------------------------------------------------------
// mh_render_backward: render_backward_impl drives the steps below, which share
// one BwdCall.  Every step enqueues on the scene's stream in the order written.
// ---------------------------------------------------------------------------
struct BwdCall {
    mh_scene *s = nullptr;
    const mh_integrator *in = nullptr;
    uint32_t seed = 0, flags = 0;
    hipStream_t st = nullptr;
    Layout L{};
    uint64_t n_px = 0, n = 0;  // pixels, samples of the slab
    uint32_t S_ = 0;           // the slab's samples per pixel
    bool dev = false, vol = false;  // MH_FLAG_DEVICE_POINTERS, prbvolpath
    Slots P;
    slots::SlotBlock blk;
    std::vector<float *> bufs;  // slot -> its buffer in s->tmp_c
    GradArgs ga;
    plan::BackwardPlan plan;
    const float *g_in = nullptr, *w = nullptr;  // grad_in (then grad_in / W per pixel) and W on the device
    // what the engines leave for the finish and the stats
    size_t wf_ctr_words = 0, wf_chunks = 0;
    uint32_t *pvb_lost = nullptr;  // prbvolpath on the scheduler: overflow entries that found their list full
    slots::FxScales fxs;           // deterministic: 2^S / 2^-S of the fixed point (fx_between)
};

// the call's waits (MH_WAIT, under the driver's name whichever step waits)
static int bwd_wait(const BwdCall &c) {
    if (wants_reduce(c.flags) && c.s->comm) return comm_wait(c.s->comm, c.st, "render_backward_impl");
    MH_HIP(hipStreamSynchronize(c.st));
    return MH_OK;
}

static int bwd_validate(const mh_scene *s, const mh_integrator *in, uint32_t spp, const float *grad_in,
                        uint32_t n_params, const uint32_t *param_tex, float *const *grads, uint32_t flags) {
    if (!s || !in || !grad_in || (n_params && (!param_tex || !grads)))
        return set_error(MH_ERR_INVALID_ARGUMENT, "mh_render_backward: NULL argument");
    if (in->type != MH_INTEGRATOR_PRB && in->type != MH_INTEGRATOR_PRBVOLPATH)
        return set_error(MH_ERR_UNSUPPORTED, "render_backward(): requires the 'prb' or 'prbvolpath' integrator");
    return check_call_args(s, in, spp, flags, "mh_render_backward", false);
}

// the parameter slots, the plan (mh_plan.hpp: engine, determinism, chunks and
// streams), the slots' buffers and the kernels' GradArgs
static int bwd_slots_and_plan(BwdCall &c, uint32_t n_params, const uint32_t *param_tex) {
    mh_scene *s = c.s;
    Slots &P = c.P;
    if (int rc = build_slots(s, n_params, param_tex, c.vol, "mh_render_backward", "render_backward", P)) return rc;
    c.blk = slots::slot_block(P.counts);
    plan::Facts facts = call_facts(s, *c.in, c.flags, c.n_px, c.S_);
    facts.n_rgb = P.n_rgb;
    facts.n_bmp = P.n_bmp;
    facts.bmp_slot_bytes = (uint64_t)P.counts[kMaxRgbParams] * 4;
    facts.n_phase_params = P.n_phase_params;
    // (several bitmaps: all with the same channel count, as the scatter's
    // transposed issue assumes)
    uint32_t ch = 0;
    for (uint32_t t = 0; t < (uint32_t)P.slot_of_tex.size(); ++t)
        if (P.slot_of_tex[t] >= kMaxRgbParams) {
            const uint32_t tc = s->h_textures[t].channels;
            facts.bmp_same_ch = facts.bmp_same_ch && (ch == 0 || ch == tc);
            ch = tc;
        }
    c.plan = plan::plan_backward(facts, env::plan_env(c.vol ? env::Call::BackwardVol : env::Call::Backward));
    // MH_FLAG_DETERMINISTIC on prbvolpath (fx) or on prb's replay kernel
    // (det_replay): int64 fixed point in two passes
    MH_HIP(upload_slots(s, P, c.blk, c.st, c.bufs, c.ga, c.vol, c.plan.fx));
    if (c.plan.fx)
        for (int k = 0; k < kMaxParams; ++k)
            if (P.grid_res[k][0] && !P.corner[k])
                return set_error(MH_ERR_OUT_OF_MEMORY,
                                 "render_backward(): the deterministic grid gradient's corner block could not be allocated");
    // one bitmap parameter of <= 48 KiB: the replay kernel accumulates its
    // texel gradients per workgroup in LDS (k_prb_backward)
    // (MH_PRB_LDS_TEX=0: global atomics, the parity tests' cross-check)
    if (c.plan.lds_tex) {
        c.ga.lds_slot = kMaxRgbParams;
        c.ga.lds_floats = (uint32_t)P.counts[kMaxRgbParams];
    }
    return MH_OK;
}

// grad_in and the weights on the device, grad_in / W once per pixel (the
// adjoint of develop), the call's counters and the deterministic replay's mirror
static int bwd_stage_adjoint(BwdCall &c, const float *grad_in, const float *weights) {
    mh_scene *s = c.s;
    const hipStream_t st = c.st;
    const Layout &L = c.L;
    const uint64_t n_px = c.n_px;
    const uint32_t flags = c.flags;
    const float *g_in = grad_in;
    if (!c.dev) {
        MH_HIP(s->tmp_d.alloc(n_px * 12));
        MH_HIP(hipMemcpyAsync(s->tmp_d.ptr, grad_in, n_px * 12, hipMemcpyHostToDevice, st));
        g_in = s->tmp_d.as<float>();
    }
    c.w = weights;
    if (!weights) {
        MH_HIP(s->weights_tmp.alloc(n_px * 4));
        MH_HIP(hipMemsetAsync(s->weights_tmp.ptr, 0, n_px * 4, st));
        // W of every sample of every pixel (common.py:936-947); with
        // MH_FLAG_REDUCE the slab's own samples + an all-reduce, unless each
        // rank is to compute the whole image itself (MH_FLAG_LOCAL_WEIGHTS)
        const bool slab_w = wants_reduce(flags) && !(flags & MH_FLAG_LOCAL_WEIGHTS);
        Layout Lall = L;
        if (!slab_w) {
            Lall.s_begin = 0;
            Lall.s_end = L.spp_pp;
        }
        LaneMap lmw = lane_map(Lall, 0);
        MH_SPLAT(s->S, lmw, kSplatWeights, fast_splat(L, s->S), (uint32_t)n_px, 1,
                 n_px * (Lall.s_end - Lall.s_begin), 0, nullptr, s->weights_tmp.as<float>(),
                 s->S.sampler_seed + c.seed, L.spp_pp >= 4, st, nullptr, c.plan.determ, 0, n_px, nullptr);
        if (slab_w)
            if (int rc = reduce_result(s, flags, s->weights_tmp.as<float>(), n_px, st, false)) return rc;
        c.w = s->weights_tmp.as<float>();
    } else if (!c.dev) {
        MH_HIP(s->tmp_e.alloc(n_px * 4));
        MH_HIP(hipMemcpyAsync(s->tmp_e.ptr, weights, n_px * 4, hipMemcpyHostToDevice, st));
        c.w = s->tmp_e.as<float>();
    }

    MH_HIP(hipMemsetAsync(s->counters.ptr, 0, 256, st));
    MH_HIP(s->gw.alloc(n_px * 16));  // float4 per pixel (k_grad_over_w)
    MH_HIP(launch_grad_over_w(n_px, g_in, c.w, s->gw.as<float>(), st));
    c.g_in = s->gw.as<float>();
    // the deterministic replay: small slots through acc_add_fx, bitmap texels
    // through bmp_add_fx into an int64 mirror of the slot block (no LDS accumulator)
    if (c.plan.det_replay) {
        MH_HIP(s->replay_fx.alloc(c.blk.alloc_floats() * 8));
        MH_HIP(hipMemsetAsync(s->replay_fx.ptr, 0, c.blk.alloc_floats() * 8, st));
        c.ga.fx_i64 = s->replay_fx.as<long long>();
        c.ga.fx_f32 = s->tmp_c.as<float>();
        c.ga.lds_slot = -1;
    }
    return MH_OK;
}

// ---- MH_FLAG_DETERMINISTIC off the wavefront: int64 fixed point in two passes ----
// Pass 1 finds the largest |item| of the grid scatter and of every slot
// (nothing is accumulated that survives), pass 2 adds round(item * 2^S) as
// int64 with slots::fx_exp's S: the sums are exact, so their order is free.

// between the passes: the scales from pass 1's maxima; pass 1's rgb-slot adds
// and counters go
static hipError_t fx_between(BwdCall &c, GradArgs &gp) {
    mh_scene *s = c.s;
    const hipStream_t st = c.st;
    uint32_t mb[1 + kMaxParams] = {};  // words 1 + k: slot k (small slots; bitmaps on the replay)
    hipError_t e = hipMemcpyAsync(mb, s->fx_word.as<uint8_t>() + kFxMaxOff, sizeof(mb), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = wait_stream(s, c.flags, st);
    if (e != hipSuccess) return e;
    c.fxs = slots::fx_scales(mb);
    gp.fx_scale = c.fxs.scale;
    e = hipMemcpyAsync(s->fx_word.as<uint8_t>() + kFxScaleOff, c.fxs.slot_scale, sizeof(c.fxs.slot_scale),
                       hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(s->fx_word.as<uint8_t>() + kFxSumOff, 0, 8 * 3 * kMaxRgbParams, st);
    if (e == hipSuccess) e = hipMemsetAsync(s->tmp_c.ptr, 0, c.blk.alloc_floats() * 4, st);
    if (e == hipSuccess) e = hipMemsetAsync(s->counters.ptr, 0, 256, st);
    return e;
}
// launch(gp) -> status enqueues one pass with the pass's GradArgs
static int fx_two_pass(BwdCall &c, const std::function<int(const GradArgs &)> &launch) {
    mh_scene *s = c.s;
    MH_HIP(s->fx_word.alloc(kFxWordBytes));
    MH_HIP(hipMemsetAsync(s->fx_word.ptr, 0, kFxScaleOff - kFxMaxOff, c.st));
    GradArgs gp = c.ga;
    gp.fx_max = s->fx_word.as<uint32_t>();
    for (uint32_t pass = 1; pass <= 2; ++pass) {
        gp.fx_mode = pass;
        if (pass == 2) MH_HIP(fx_between(c, gp));
        if (int rc = launch(gp)) return rc;
    }
    return MH_OK;
}
// after pass 2: the small slots' exact sums into their buffers (which
// pass 2 left at zero: acc_add_fx bypasses the register accumulators)
static hipError_t fx_small_fold(BwdCall &c) {
    mh_scene *s = c.s;
    const hipStream_t st = c.st;
    long long w[3 * kMaxRgbParams];
    hipError_t e = hipMemcpyAsync(w, s->fx_word.as<uint8_t>() + kFxSumOff, sizeof(w), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = wait_stream(s, c.flags, st);
    for (uint32_t k = 0; e == hipSuccess && k < c.P.n_rgb; ++k) {
        float v[3];
        for (int ch = 0; ch < 3; ++ch) v[ch] = (float)((double)w[3 * k + ch] * c.fxs.slot_inv[k]);
        e = hipMemcpyAsync(c.bufs[k], v, std::min<size_t>(3, slots::padded(c.P.counts[k])) * 4, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = wait_stream(s, c.flags, st);
    }
    return e;
}

// ---- the engines ----------------------------------------------------------------
// prb on the fused wavefront: rgb slots as per-block partials, bitmap slots
// through vertex records and a texel scatter per chunk
static int bwd_wavefront(BwdCall &c) {
    mh_scene *s = c.s;
    const mh_integrator *in = c.in;
    const hipStream_t st = c.st;
    const Layout &L = c.L;
    const plan::BackwardPlan &plan = c.plan;
    const GradArgs &ga = c.ga;
    const uint64_t n_px = c.n_px;
    const uint32_t S_ = c.S_, n_rgb = c.P.n_rgb;
    const bool bmp_wf = plan.bmp_wf;
    const int cus = device_cus(s->device);
    const uint32_t n_depth = plan.n_depth, chunk_px = plan.chunks.chunk_px;
    const bool two = plan.chunks.two;  // two-stream chunk pipeline (fork_stream)
    // MH_FLAG_SHARED_DEVICE (another call runs beside this one) or the two
    // chunk streams: the launches take a share of the CUs' slots (wf_blocks)
    const uint32_t grid = wf_grid(wf_blocks(cus, two || (c.flags & MH_FLAG_SHARED_DEVICE) != 0));
    const uint64_t cap = (uint64_t)chunk_px * S_;
    const size_t n_chunks = (size_t)plan.chunks.n_chunks;
    const uint32_t n_bounces = in->max_depth;
    const size_t ctr_per_chunk = wf_counter_words(n_bounces);
    MH_HIP(s->wf_ws.alloc(wf_workspace_bytes(cap)));
    MH_HIP(s->wf_ws_prb.alloc(wf_prb_workspace_bytes(cap)));
    if (two) {
        MH_HIP(s->wf_ws2.alloc(wf_workspace_bytes(cap)));
        MH_HIP(s->wf_ws_prb2.alloc(wf_prb_workspace_bytes(cap)));
    }
    WfBitmapArgs bmp;
    if (bmp_wf) {
        MH_HIP(s->wf_ws_bmp.alloc(wf_bmp_workspace_bytes(cap, n_depth)));
        if (two) MH_HIP(s->wf_ws_bmp2.alloc(wf_bmp_workspace_bytes(cap, n_depth)));
        int max_wg = 64 << 10, per_cu_lds = 160 << 10;
        (void)hipDeviceGetAttribute(&max_wg, hipDeviceAttributeMaxSharedMemoryPerBlock, s->device);
        (void)hipDeviceGetAttribute(&per_cu_lds, hipDeviceAttributeMaxSharedMemoryPerMultiprocessor, s->device);
        bmp.ws = s->wf_ws_bmp.ptr;
        bmp.n_depth = n_depth;
        bmp.slot = kMaxRgbParams;
        // every bitmap slot kMaxRgbParams + b: its texture and its offset in
        // the bitmap slots' contiguous block of s->tmp_c (slots::slot_block)
        for (int b = 0; b < kMaxBitmapParams; ++b) bmp.off[b] = c.blk.bmp_off[b];
        for (uint32_t t = 0; t < (uint32_t)c.P.slot_of_tex.size(); ++t)
            if (c.P.slot_of_tex[t] >= kMaxRgbParams) bmp.tex[c.P.slot_of_tex[t] - kMaxRgbParams] = t;
        bmp.grad = c.bufs[kMaxRgbParams];
        bmp.n_floats = c.blk.bmp_floats;
        bmp.lds_max = plan.bmp_lds ? (uint32_t)std::min(max_wg, 64 << 10) : 0u;
        if (plan.determ) {  // fixed-point texel sums (k_wf_bitmap_scatter<false, Fx>)
            MH_HIP(s->bmp_fx.alloc((size_t)bmp.n_floats * 8 + 256));
            bmp.fx_word = s->bmp_fx.as<uint32_t>();
            bmp.fx_acc = reinterpret_cast<unsigned long long *>(s->bmp_fx.as<uint8_t>() + 256);
        }
        bmp.n_rec = s->counters.as<unsigned long long>() + kCtrAuxItems;
        bmp.wg_lds = (uint32_t)max_wg;
        bmp.cu_lds = (uint32_t)per_cu_lds;
        bmp.cus = (uint32_t)cus;
    }
    // MH_FLAG_DETERMINISTIC: rgb slots summed per path and reduced in a
    // fixed order (WfDet); bitmap texels in int64 fixed point (bmp.fx_acc)
    const bool det_grad = plan.det_grad;
    if (det_grad) MH_HIP(s->wf_ws_det.alloc(wf_det_workspace_bytes(cap)));
    MH_HIP(s->wf_ctr.alloc(ctr_per_chunk * n_chunks * 4));
    const size_t partial_bytes = (size_t)grid * kMaxRgbParams * 3 * 4;
    MH_HIP(s->wf_partial.alloc(partial_bytes));
    MH_HIP(hipMemsetAsync(s->wf_partial.ptr, 0, partial_bytes, st));
    if (two) {
        MH_HIP(s->wf_partial2.alloc(partial_bytes));
        MH_HIP(hipMemsetAsync(s->wf_partial2.ptr, 0, partial_bytes, st));
    }
    MH_HIP(grow_evpool(s, 3 * n_chunks));
    DScene S2 = s->S;  // stream2's scene view: its own stack overflow columns (stream-engine scenes)
    if (two && s->S.stack_ovf) {
        MH_HIP(s->stack_ovf2.alloc(s->stack_ovf.bytes));
        S2.stack_ovf = s->stack_ovf2.as<uint32_t>();
    }
    if (two) MH_HIP(fork_stream(s, st));
    size_t chunk = 0;
    for (uint64_t p0 = 0; p0 < n_px; p0 += chunk_px, ++chunk) {
        const uint32_t npx = (uint32_t)std::min<uint64_t>(chunk_px, n_px - p0);
        // the chunk's stream and buffers (two: odd chunks on stream2)
        const bool odd = two && (chunk & 1);
        WfBitmapArgs bc = bmp;
        if (odd) bc.ws = s->wf_ws_bmp2.ptr;
        MH_HIP(launch_wavefront_prb(odd ? S2 : s->S, *in, lane_map(L, (uint32_t)p0), s->S.sampler_seed + c.seed,
                                    (uint64_t)npx * S_, L.spp_pp >= 4, c.g_in, c.w, ga.slot_of_tex, n_rgb,
                                    (odd ? s->wf_ws2 : s->wf_ws).ptr, (odd ? s->wf_ws_prb2 : s->wf_ws_prb).ptr, cap,
                                    s->wf_ctr.as<uint32_t>() + ctr_per_chunk * chunk, n_bounces, grid,
                                    (odd ? s->wf_partial2 : s->wf_partial).as<float>(), odd ? s->stream2 : st,
                                    &s->evpool[3 * chunk], bmp_wf ? &bc : nullptr,
                                    det_grad ? s->wf_ws_det.ptr : nullptr, ga.emitter_off));
    }
    if (two) MH_HIP(join_stream(s, st));
    MH_HIP(launch_wf_grad_reduce(s->wf_partial.as<float>(), grid, n_rgb, ga.bufs, st));
    if (two) MH_HIP(launch_wf_grad_reduce(s->wf_partial2.as<float>(), grid, n_rgb, ga.bufs, st));
    c.wf_ctr_words = ctr_per_chunk;
    c.wf_chunks = n_chunks;
    return MH_OK;
}

// prbvolpath: persistent grid, one NEE-walk log per thread (NeeLog;
// MH_PVP_NEE_LOG=0: the NEE walks are replayed, bwd_replay);
// single pass (MainLog, main_cap entries per thread) unless
// MH_PVP_SINGLE=0, on the phase scheduler (k_vol_sched<PvBwdMachine>)
// unless MH_PVP_SCHED=0 (the per-sample kernel k_prbvol_backward)
static int bwd_pvp_log(BwdCall &c) {
    mh_scene *s = c.s;
    const mh_integrator *in = c.in;
    const hipStream_t st = c.st;
    const Layout &L = c.L;
    const uint64_t n = c.n;
    const int cus = device_cus(s->device);
    uint32_t main_cap = c.plan.main_cap;
    const uint32_t cap = c.plan.nee_cap;
    bool sched = c.plan.sched;
    // the persistent grid (and with it both per-thread logs): the
    // scheduler's, or k_prbvol_backward's shrunk to the work (a wave takes
    // 64 samples per batch, so more threads than samples would only hold log space)
    const uint32_t blocks = sched ? vs_blocks(cus)
                                  : (uint32_t)std::max<uint64_t>(
                                        1, std::min<uint64_t>((uint64_t)cus * kPvpBlocksPerCu, (n + 255) / 256));
    // a log that cannot be allocated degrades the kernel instead of failing
    // the call: no MainLog -> primal + adjoint replay per sample; no NeeLog
    // either -> one thread per sample with the NEE walks replayed
    bool nee_ok = s->pvp_log.alloc((size_t)blocks * 256 * cap * 16) == hipSuccess;
    if (!nee_ok) { (void)hipGetLastError(); s->pvp_log.release(); }
    if (main_cap && (!nee_ok || s->pvp_main.alloc((size_t)blocks * 256 * main_cap * 64) != hipSuccess)) {
        (void)hipGetLastError();
        s->pvp_main.release();
        main_cap = 0;
    }
    // overflow lists of the scheduler (2 + kPvbWalkRec float4 per entry)
    const uint32_t ovf_cap = (uint32_t)std::min<uint64_t>(n, 1ull << 26);
    sched = sched && main_cap && nee_ok &&
            s->pvp_ovf.alloc((size_t)ovf_cap * (2 + kPvbWalkRec) * 16 + 256) == hipSuccess;
    auto launch = [&](const GradArgs &gp) -> int {
        if (sched) {
            VsBwdArgs bw;
            bw.grad_in = c.g_in;
            bw.coalesce = L.spp_pp >= 4;
            bw.ga = gp;
            bw.main_log = s->pvp_main.as<float4>();
            bw.nee_log = s->pvp_log.as<float4>();
            bw.main_cap = main_cap;
            bw.nee_cap = cap;
            bw.ovf_paths = s->pvp_ovf.as<float4>();
            bw.ovf_walks = bw.ovf_paths + (size_t)2 * ovf_cap;
            bw.ovf_count = reinterpret_cast<uint32_t *>(bw.ovf_walks + (size_t)kPvbWalkRec * ovf_cap);
            bw.ovf_cap = ovf_cap;
            MH_HIP(hipMemsetAsync(bw.ovf_count, 0, 16, st));
            c.pvb_lost = bw.ovf_count + 2;
            const LaneMap lm0 = lane_map(L, 0);
            MH_HIP(launch_vol_sched_bwd(s->S, *in, lm0, s->S.sampler_seed + c.seed, n, bw, blocks,
                                        s->counters.as<unsigned long long>(), st));
            MH_HIP(launch_vol_sched_bwd_replays(s->S, *in, lm0, s->S.sampler_seed + c.seed, n, bw,
                                                s->counters.as<unsigned long long>(), st));
            if (env::vw_debug()) {
                if (int rc = bwd_wait(c)) return rc;
                if (int rc2 = print_vs_phases(s)) return rc2;
                uint32_t oc[3];
                MH_HIP(hipMemcpy(oc, bw.ovf_count, sizeof(oc), hipMemcpyDeviceToHost));
                fprintf(stderr, "pvb overflow replays: %u paths, %u walks, %u lost\n", oc[0], oc[1], oc[2]);
            }
        } else {
            MH_HIP(launch_prb_backward(s->S, *in, lane_map(L, 0), s->S.sampler_seed + c.seed, n, L.spp_pp >= 4,
                                       c.g_in, c.w, gp, c.plan.fused, s->counters.as<unsigned long long>(), st,
                                       nee_ok ? s->pvp_log.as<float4>() : nullptr, cap, blocks,
                                       s->counters.as<unsigned long long>() + kCtrPvpHead,
                                       main_cap ? s->pvp_main.as<float4>() : nullptr, main_cap));
        }
        return MH_OK;
    };
    return c.plan.fx ? fx_two_pass(c, launch) : launch(c.ga);
}

// the per-lane replay kernel (k_prb_backward; prbvolpath with MH_PVP_NEE_LOG=0:
// its NEE walks replayed), deterministic (fxr) in two fixed-point passes
static int bwd_replay(BwdCall &c) {
    mh_scene *s = c.s;
    const Layout &L = c.L;
    auto launch = [&](const GradArgs &gp) -> int {
        MH_HIP(launch_prb_backward(s->S, *c.in, lane_map(L, 0), s->S.sampler_seed + c.seed, c.n, L.spp_pp >= 4,
                                   c.g_in, c.w, gp, c.plan.fused, s->counters.as<unsigned long long>(), c.st));
        return MH_OK;
    };
    return c.plan.fxr ? fx_two_pass(c, launch) : launch(c.ga);
}

// ---- after the engine -----------------------------------------------------------
// the fixed-point sums and the corner blocks into the slot buffers, the
// reduction over the communicator, and the slot buffers into the caller's
static int bwd_finish(BwdCall &c, uint32_t n_params, float *const *grads) {
    mh_scene *s = c.s;
    const hipStream_t st = c.st;
    const Slots &P = c.P;
    const std::vector<float *> &bufs = c.bufs;
    if (c.plan.fxr) MH_HIP(fx_small_fold(c));
    if (c.plan.det_replay)
        for (int k = kMaxRgbParams; k < kMaxParams; ++k)
            if (P.counts[k])
                MH_HIP(launch_fx_to_float(s->replay_fx.as<long long>() + (bufs[k] - s->tmp_c.as<float>()), bufs[k],
                                          P.counts[k], c.fxs.slot_inv[k], st));
    for (int k = 0; k < kMaxParams; ++k) {
        if (!P.corner[k]) continue;
        if (P.fx)
            MH_HIP(launch_corner_gather_fx(reinterpret_cast<const long long *>(P.corner[k]), bufs[k], P.grid_res[k],
                                           c.fxs.inv, st));
        else
            MH_HIP(launch_corner_gather(P.corner[k], bufs[k], P.grid_res[k], st));
    }
    MH_HIP(hipEventRecord(s->ev1, st));
    // the slot buffers are one block of s->tmp_c (upload_slots)
    if (int rc = reduce_result(s, c.flags, s->tmp_c.as<float>(), c.blk.total, st, false)) return rc;
    // accumulate into the caller's gradient buffers
    std::vector<float> host_tmp;
    for (uint32_t k = 0; k < n_params; ++k) {
        const uint32_t slot = P.slot_of_param[k];
        const size_t cnt = P.counts[slot];
        if (c.dev) {
            MH_HIP(launch_accumulate(grads[k], bufs[slot], cnt, st));
        } else {
            host_tmp.resize(cnt);
            MH_HIP(hipMemcpyAsync(host_tmp.data(), bufs[slot], cnt * 4, hipMemcpyDeviceToHost, st));
            if (int rc = bwd_wait(c)) return rc;
            for (size_t i = 0; i < cnt; ++i) grads[k][i] += host_tmp[i];
        }
    }
    return MH_OK;
}

// (after a stream sync) an overflow replay that did not run fails the call
static int bwd_check_lost(const BwdCall &c) {
    uint32_t lost = 0;
    if (c.pvb_lost) MH_HIP(hipMemcpy(&lost, c.pvb_lost, 4, hipMemcpyDeviceToHost));
    if (lost)
        return set_error(MH_ERR_OUT_OF_MEMORY, "render_backward(): " + std::to_string(lost) +
                                                   " prbvolpath overflow replays did not fit their list "
                                                   "(MH_PVP_SCHED=0 runs the per-sample kernel)");
    return MH_OK;
}

// the call's sync, the lost-replay check and, if asked for, the ray counters and timings
static int bwd_stats(BwdCall &c, mh_stats *stats, double t_start) {
    mh_scene *s = c.s;
    const mh_integrator *in = c.in;
    const hipStream_t st = c.st;
    const bool wavefront = c.plan.wavefront;
    const size_t wf_chunks = c.wf_chunks;
    if (!stats) {
        if (int rc = bwd_wait(c)) return rc;
        return bwd_check_lost(c);
    }
    unsigned long long ctr[2] = {0, 0}, n_rec = 0;
    std::vector<uint32_t> wctr(c.wf_ctr_words * wf_chunks);
    if (wavefront) {
        MH_HIP(hipMemcpyAsync(wctr.data(), s->wf_ctr.ptr, wctr.size() * 4, hipMemcpyDeviceToHost, st));
        MH_HIP(hipMemcpyAsync(&n_rec, s->counters.as<unsigned long long>() + kCtrAuxItems, 8, hipMemcpyDeviceToHost, st));
    } else
        MH_HIP(hipMemcpyAsync(ctr, s->counters.ptr, sizeof(ctr), hipMemcpyDeviceToHost, st));
    if (int rc = bwd_wait(c)) return rc;
    if (int rc_lost = bwd_check_lost(c)) return rc_lost;
    if (wavefront) fold_wf_counters(wctr, c.wf_ctr_words, wf_chunks, in->max_depth, ctr);
    float ms = 0.f, trace_ms = 0.f, scat_ms = 0.f;
    MH_HIP(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    for (size_t ck = 0; wavefront && ck < wf_chunks; ++ck) {
        float t = 0.f;
        MH_HIP(hipEventElapsedTime(&t, s->evpool[3 * ck], s->evpool[3 * ck + 1]));
        trace_ms += t;
        MH_HIP(hipEventElapsedTime(&t, s->evpool[3 * ck + 1], s->evpool[3 * ck + 2]));
        scat_ms += t;
    }
    if (c.plan.bmp_wf) {  // the texel scatter: one launch per chunk
        stats->aux_items = n_rec;
        stats->ms_aux = scat_ms;
        stats->n_aux_launches = wf_chunks;
    }
    // the bounce-kernel span (fused: k_wf_bounce_prb launches only)
    stats->ms_trace = trace_ms;
    stats->n_trace_launches = wavefront ? (uint64_t)wf_chunks * in->max_depth : 0;
    stats->mode = wavefront ? 1u : 0u;
    stats->samples = c.n;
    stats->rays_closest = ctr[0];
    stats->rays_shadow = ctr[1];
    stats->bounces = ctr[0];
    stats->ms_total = now_ms() - t_start;
    stats->ms_kernel = ms;
    return MH_OK;
}

static int render_backward_impl(mh_scene *s, const mh_integrator *in, uint32_t seed, uint32_t spp,
                       uint32_t spp_begin, uint32_t spp_end, const float *grad_in,
                       const float *weights, uint32_t n_params, const uint32_t *param_tex,
                       float *const *grads, uint32_t flags, mh_stats *stats) {
    ScopedPhase phase_("RenderBackward");
    if (int rc = bwd_validate(s, in, spp, grad_in, n_params, param_tex, grads, flags)) return rc;
    const double t_start = now_ms();
    if (stats) *stats = mh_stats{};
    BwdCall c;
    if (int rc = make_layout(s, spp, spp_begin, spp_end, c.L, true)) return rc;
    MH_HIP(hipSetDevice(s->device));
    g_call_issued = true;  // past argument validation: a failure from here aborts the communicator
    c.s = s;
    c.in = in;
    c.seed = seed;
    c.flags = flags;
    c.st = s->stream;
    c.n_px = (uint64_t)c.L.W * c.L.H;
    c.S_ = c.L.s_end - c.L.s_begin;
    c.n = c.n_px * c.S_;
    c.dev = flags & MH_FLAG_DEVICE_POINTERS;
    c.vol = in->type == MH_INTEGRATOR_PRBVOLPATH;
    if (int rc = bwd_slots_and_plan(c, n_params, param_tex)) return rc;
    if (int rc = bwd_stage_adjoint(c, grad_in, weights)) return rc;
    MH_HIP(hipEventRecord(s->ev0, c.st));
    // wavefront; prbvolpath with its logs; else the replay kernel
    if (int rc = c.plan.wavefront ? bwd_wavefront(c) : c.plan.pvp_log ? bwd_pvp_log(c) : bwd_replay(c)) return rc;
    if (int rc = bwd_finish(c, n_params, grads)) return rc;
    if (async_call(flags, stats)) return MH_OK;  // gradients stay stream-ordered on the device
    return bwd_stats(c, stats, t_start);
}

// ---------------------------------------------------------------------------
// Forward-mode derivative: RBIntegrator.render_forward (common.py:696-826)
// ---------------------------------------------------------------------------
static int render_forward_impl(mh_scene *s, const mh_integrator *in, uint32_t seed, uint32_t spp, uint32_t spp_begin,
                      uint32_t spp_end, uint32_t n_params, const uint32_t *param_tex, const float *const *tangents,
                      float *film_rgbw, uint32_t flags, mh_stats *stats) {
    ScopedPhase phase_("RenderForward");
    if (!s || !in || !film_rgbw || (n_params && (!param_tex || !tangents)))
        return set_error(MH_ERR_INVALID_ARGUMENT, "mh_render_forward: NULL argument");
    if (in->type != MH_INTEGRATOR_PRB && in->type != MH_INTEGRATOR_PRBVOLPATH)
        return set_error(MH_ERR_UNSUPPORTED, "render_forward(): requires the 'prb' or 'prbvolpath' integrator");
    if (int rc = check_call_args(s, in, spp, flags, "mh_render_forward", true)) return rc;
    const double t_start = now_ms();
    if (stats) *stats = mh_stats{};
    Layout L;
    int rc = make_layout(s, spp, spp_begin, spp_end, L, true);  // prepare(): one wavefront of <= 2^32
    if (rc) return rc;
    MH_HIP(hipSetDevice(s->device));
    g_call_issued = true;  // past argument validation: a failure from here aborts the communicator
    hipStream_t st = s->stream;
    const bool dev = flags & MH_FLAG_DEVICE_POINTERS;
    Slots P;
    rc = build_slots(s, n_params, param_tex, in->type == MH_INTEGRATOR_PRBVOLPATH, "mh_render_forward",
                     "render_forward", P);
    if (rc) return rc;
    std::vector<float *> bufs;
    GradArgs ga;
    MH_HIP(upload_slots(s, P, slots::slot_block(P.counts), st, bufs, ga));  // zeroed slot buffers, here the tangents
    for (uint32_t k = 0; k < n_params; ++k) {
        const uint32_t slot = P.slot_of_param[k];
        if (!tangents[k]) return set_error(MH_ERR_INVALID_ARGUMENT, "mh_render_forward: NULL tangent");
        MH_HIP(hipMemcpyAsync(bufs[slot], tangents[k], P.counts[slot] * 4,
                              dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    }
    // the film: as mh_render
    const uint64_t n_px = (uint64_t)L.W * L.H;
    FilmStage F;
    if (int rc2 = stage_film(s, n_px, film_rgbw, flags, st, F)) return rc2;
    const bool alpha = F.alpha;
    const size_t film_bytes = F.bytes;
    float *const film = F.film, *const film4 = F.film4, *const film_a = F.film_a;
    MH_HIP(hipMemsetAsync(s->counters.ptr, 0, 256, st));
    const uint32_t S_ = L.s_end - L.s_begin;
    // prb on packet-engine scenes: the fused forward-mode wavefront
    // (k_wf_bounce_fwd); prbvolpath, larger scenes or MH_FLAG_MEGAKERNEL /
    // MH_MODE=mega: the per-sample kernel (k_render_forward)
    const plan::ForwardPlan plan =
        plan::plan_forward(call_facts(s, *in, flags, n_px, S_), env::plan_env(env::Call::Forward));
    const uint32_t chunk_px = plan.chunk_px;
    const uint64_t plane = (uint64_t)chunk_px * S_;
    MH_HIP(s->work.alloc(plane * (alpha ? 6 : 5) * sizeof(float)));
    const bool wavefront = plan.wavefront;
    const int cus = device_cus(s->device);
    if (wavefront) {
        MH_HIP(s->wf_ws.alloc(wf_workspace_bytes(plane)));
        MH_HIP(s->wf_ws_prb.alloc(wf_prb_workspace_bytes(plane)));
        MH_HIP(s->wf_ctr.alloc((size_t)wf_counter_words(in->max_depth) * 4));
    }
    const bool fast = fast_splat(L, s->S);
    const int coalesce = L.spp_pp >= 4;  // block.set_coalesce(... and spp >= 4) (common.py:795-796)
    const uint32_t seed_value = s->S.sampler_seed + seed;
    const bool determ = plan.determ;
    unsigned long long *bounds = s->counters.as<unsigned long long>() + kCtrBounds;
    MH_HIP(hipEventRecord(s->ev0, st));
    for (uint64_t p0 = 0; p0 < n_px; p0 += chunk_px) {
        const uint32_t npx = (uint32_t)std::min<uint64_t>(chunk_px, n_px - p0);
        const LaneMap lm = lane_map(L, (uint32_t)p0);
        const uint64_t n = (uint64_t)npx * S_;
        if (wavefront)
            MH_HIP(launch_wavefront_fwd(s->S, *in, lm, seed_value, n, ga.slot_of_tex, ga.bufs, ga.is_rgb,
                                        s->work.as<float>(), plane, alpha, s->wf_ws.ptr, s->wf_ws_prb.ptr, plane,
                                        s->wf_ctr.as<uint32_t>(), in->max_depth, wf_grid(wf_blocks(cus)), st,
                                        ga.emitter_off));
        else
            MH_HIP(launch_render_forward(s->S, *in, lm, seed_value, n, plane, s->work.as<float>(), ga,
                                         s->counters.as<unsigned long long>(), st, alpha));
        // no sample check here: tangent radiance is legitimately negative
        MH_SPLAT(s->S, lm, kSplatFilm, fast, npx, 1, n, plane, s->work.as<float>(), film4, seed_value,
                 coalesce, st, nullptr, determ, s->work.bytes / 4, n_px * 4, bounds);
        if (alpha)
            MH_SPLAT(s->S, lm, kSplatAlpha, fast, npx, 1, n, plane, s->work.as<float>(), film_a, seed_value,
                     coalesce, st, nullptr, determ, s->work.bytes / 4, n_px, bounds);
    }
    if (alpha) MH_HIP(launch_film_rgbaw(n_px, film4, film_a, film, st));
    MH_HIP(hipEventRecord(s->ev1, st));
    if (int rc2 = reduce_result(s, flags, film, film_bytes / 4, st, true)) return rc2;
    if (!dev) MH_HIP(hipMemcpyAsync(film_rgbw, film, film_bytes, hipMemcpyDeviceToHost, st));
    if (async_call(flags, stats)) return MH_OK;
    if (!stats) {
        MH_WAIT(s, flags, st);
        return check_bounds_counter(s, "mh_render_forward");
    }
    unsigned long long ctr[2] = {0, 0};
    MH_HIP(hipMemcpyAsync(ctr, s->counters.ptr, sizeof(ctr), hipMemcpyDeviceToHost, st));
    MH_WAIT(s, flags, st);
    if (int rc = check_bounds_counter(s, "mh_render_forward")) return rc;
    if (stats) {
        float ms = 0.f;
        MH_HIP(hipEventElapsedTime(&ms, s->ev0, s->ev1));
        stats->samples = n_px * S_;
        stats->rays_closest = ctr[0];
        stats->rays_shadow = ctr[1];
        stats->bounces = ctr[0];
        stats->ms_total = now_ms() - t_start;
        stats->ms_kernel = ms;
        stats->ms_trace = 0.f;
        stats->n_trace_launches = 0;
        stats->mode = plan.mode;  // 2: fused wavefront, 0: per-sample kernel
        stats->invalid_samples = 0;  // not counted: a tangent's radiance may be negative
    }
    return MH_OK;
}

// ---------------------------------------------------------------------------
// Ray-query sub-boundary
// ---------------------------------------------------------------------------
static int trace_impl(mh_scene *s, bool shadow, uint64_t n, const float *rays, float *t, float *u,
                      float *v, uint32_t *prim, uint32_t *shape, uint32_t *inst, uint32_t *occ, uint32_t flags,
                      mh_stats *stats) {
    ScopedPhase phase_("RayIntersect");
    if (!s || (n && !rays)) return set_error(MH_ERR_INVALID_ARGUMENT, "mh_trace: NULL argument");
    if (n == 0) return MH_OK;
    double t_start = now_ms();
    if (stats) *stats = mh_stats{};
    MH_HIP(hipSetDevice(s->device));
    hipStream_t st = s->stream;
    const bool dev = flags & MH_FLAG_DEVICE_POINTERS;
    const float *r = rays;
    float *dt = t, *du = u, *dv = v;
    uint32_t *dp = prim, *ds = shape, *di = inst, *doc = occ;
    if (!dev) {
        MH_HIP(s->tmp_a.alloc(n * 28));
        MH_HIP(hipMemcpyAsync(s->tmp_a.ptr, rays, n * 28, hipMemcpyHostToDevice, st));
        r = s->tmp_a.as<float>();
        MH_HIP(s->tmp_b.alloc(n * 24));
        float *base = s->tmp_b.as<float>();
        dt = base; du = base + n; dv = base + 2 * n;
        dp = reinterpret_cast<uint32_t *>(base + 3 * n);
        ds = reinterpret_cast<uint32_t *>(base + 4 * n);
        di = inst ? reinterpret_cast<uint32_t *>(base + 5 * n) : nullptr;
        doc = reinterpret_cast<uint32_t *>(base);
    }
    // persistent grid: 8 workgroups of 256 lanes per CU
    uint32_t grid = (uint32_t)std::min<uint64_t>((n + 255) / 256, (uint64_t)device_cus(s->device) * 8);
    MH_HIP(hipEventRecord(s->ev0, st));
    MH_HIP(launch_trace(s->S, shadow, n, r, dt, du, dv, dp, ds, di, doc, grid, st));
    MH_HIP(hipEventRecord(s->ev1, st));
    if (!dev) {
        if (shadow) {
            MH_HIP(hipMemcpyAsync(occ, doc, n * 4, hipMemcpyDeviceToHost, st));
        } else {
            MH_HIP(hipMemcpyAsync(t, dt, n * 4, hipMemcpyDeviceToHost, st));
            MH_HIP(hipMemcpyAsync(u, du, n * 4, hipMemcpyDeviceToHost, st));
            MH_HIP(hipMemcpyAsync(v, dv, n * 4, hipMemcpyDeviceToHost, st));
            MH_HIP(hipMemcpyAsync(prim, dp, n * 4, hipMemcpyDeviceToHost, st));
            MH_HIP(hipMemcpyAsync(shape, ds, n * 4, hipMemcpyDeviceToHost, st));
            if (inst) MH_HIP(hipMemcpyAsync(inst, di, n * 4, hipMemcpyDeviceToHost, st));
        }
    }
    if (!(flags & MH_FLAG_NO_SYNC) || !dev) MH_HIP(hipStreamSynchronize(st));
    if (stats) {
        MH_HIP(hipEventSynchronize(s->ev1));
        float ms = 0.f;
        MH_HIP(hipEventElapsedTime(&ms, s->ev0, s->ev1));
        stats->samples = 0;
        stats->rays_closest = shadow ? 0 : n;
        stats->rays_shadow = shadow ? n : 0;
        stats->bounces = 0;
        stats->ms_total = now_ms() - t_start;
        stats->ms_kernel = ms;
    }
    return MH_OK;
}

int mh_trace_closest(mh_scene *s, uint64_t n, const float *rays, float *t, float *u, float *v,
                     uint32_t *prim, uint32_t *shape, uint32_t flags, mh_stats *stats) {
    return mh_trace_preliminary(s, n, rays, t, u, v, prim, shape, nullptr, flags, stats);
}

int mh_trace_preliminary(mh_scene *s, uint64_t n, const float *rays, float *t, float *u, float *v,
                         uint32_t *prim, uint32_t *shape, uint32_t *instance, uint32_t flags, mh_stats *stats) {
    if (n && (!t || !u || !v || !prim || !shape))
        return set_error(MH_ERR_INVALID_ARGUMENT, "mh_trace_closest: NULL output");
    return trace_impl(s, false, n, rays, t, u, v, prim, shape, instance, nullptr, flags, stats);
}

int mh_trace_shadow(mh_scene *s, uint64_t n, const float *rays, uint32_t *occluded, uint32_t flags,
                    mh_stats *stats) {
    if (n && !occluded) return set_error(MH_ERR_INVALID_ARGUMENT, "mh_trace_shadow: NULL output");
    return trace_impl(s, true, n, rays, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, occluded, flags,
                      stats);
}

// ===========================================================================
// Multi-GPU (include/mitsuba_hip.h, "Multi-GPU").  The
// reference's splice point is SamplingIntegrator::render
// (src/render/integrator.cpp:276-390): its sample loop is cut into per-device
// slabs of every pixel, whose union is sample-identical to one render.
// ===========================================================================
// The entry points with in-call collectives: a call that fails with
// MH_FLAG_REDUCE aborts the scene's communicator (comm_abort), since it has
// issued only part of the call's collectives and its peers' streams wait on
// the rest: their waits then end in an error (comm_wait), and later
// collectives on this communicator fail at once instead of pairing with a
// peer's different collective.
static int abort_on_failure(mh_scene *s, uint32_t flags, int rc) {
    const bool issued = g_call_issued;  // argument errors (before any work) leave the communicator usable
    g_call_issued = false;
    g_keep_error = false;
#ifdef MH_DEBUG
    // the debug build's device bounds guards (MH_GUARD) fail the call
    // (not for asynchronous calls, whose work is still queued; a call with
    // collectives in flight waits through comm_wait and its deadline, not a
    // device-wide sync.  The guard words are per device: concurrent scenes on
    // one device read each other's counts -- run guard builds one scene at a time)
    if (rc == MH_OK && issued && s && !(flags & MH_FLAG_NO_SYNC)) {
        (void)hipSetDevice(s->device);
        unsigned long long g[2][kGuardCount] = {};
        const bool waited = (wants_reduce(flags) && s->comm) ? comm_wait(s->comm, s->stream, "MH_DEBUG guard read") == MH_OK
                                                             : hipStreamSynchronize(s->stream) == hipSuccess;
        if (!waited) {
            if (!(wants_reduce(flags) && s->comm)) rc = set_error(MH_ERR_HIP, "MH_DEBUG: the stream could not be synchronized");
            else rc = MH_ERR_HIP;  // comm_wait's message stands
        } else if (guard_read_wf(g[0]) != hipSuccess || guard_read_k(g[1]) != hipSuccess)
            rc = set_error(MH_ERR_HIP, "MH_DEBUG: the device guard counters could not be read");
        static const char *what[kGuardCount] = {"queue item beyond its segment", "path id beyond the chunk",
                                                "appended slot beyond its segment", "sample-plane index beyond the plane",
                                                "generated pixel outside the film", "LDS accumulator index beyond its size", "", ""};
        for (int k = 0; rc == MH_OK && k < kGuardCount; ++k)
            if (g[0][k] + g[1][k])
                rc = set_error(MH_ERR_HIP, std::string("MH_DEBUG device guard: ") + what[k] + " (" +
                                               std::to_string(g[0][k] + g[1][k]) + " lanes)");
    }
#endif
    if (rc != MH_OK && issued && s && s->comm && wants_reduce(flags)) {
        const std::string why = g_error;
        comm_abort(s->comm);
        set_error(rc, why + " (the scene's communicator was aborted)");
    }
    return rc;
}

int mh_render(mh_scene *s, const mh_integrator *in, uint32_t seed, uint32_t spp, uint32_t spp_begin,
              uint32_t spp_end, float *film_rgbw, uint32_t flags, mh_stats *stats) {
    g_call_issued = false;
    return abort_on_failure(s, flags, render_impl(s, in, seed, spp, spp_begin, spp_end, film_rgbw, flags, stats));
}

int mh_prb_weights(mh_scene *s, uint32_t seed, uint32_t spp, uint32_t spp_begin, uint32_t spp_end,
                   float *weights, uint32_t flags) {
    g_call_issued = false;
    return abort_on_failure(s, flags, prb_weights_impl(s, seed, spp, spp_begin, spp_end, weights, flags));
}

int mh_render_backward(mh_scene *s, const mh_integrator *in, uint32_t seed, uint32_t spp,
                       uint32_t spp_begin, uint32_t spp_end, const float *grad_in,
                       const float *weights, uint32_t n_params, const uint32_t *param_tex,
                       float *const *grads, uint32_t flags, mh_stats *stats) {
    g_call_issued = false;
    return abort_on_failure(s, flags, render_backward_impl(s, in, seed, spp, spp_begin, spp_end, grad_in, weights,
                                                           n_params, param_tex, grads, flags, stats));
}

int mh_render_forward(mh_scene *s, const mh_integrator *in, uint32_t seed, uint32_t spp, uint32_t spp_begin,
                      uint32_t spp_end, uint32_t n_params, const uint32_t *param_tex, const float *const *tangents,
                      float *film_rgbw, uint32_t flags, mh_stats *stats) {
    g_call_issued = false;
    return abort_on_failure(s, flags, render_forward_impl(s, in, seed, spp, spp_begin, spp_end, n_params, param_tex,
                                                          tangents, film_rgbw, flags, stats));
}

int mh_scene_set_comm(mh_scene *s, mh_comm *comm) {
    if (!s) return set_error(MH_ERR_INVALID_ARGUMENT, "mh_scene_set_comm: NULL scene");
    if (comm) {
        int dev = -1;
        if (int rc = mh_comm_info(comm, nullptr, nullptr, &dev)) return rc;
        if (dev != s->device)
            return set_error(MH_ERR_INVALID_ARGUMENT, "mh_scene_set_comm: the communicator's device is not the scene's");
    }
    if (s->comm) comm_attach(s->comm, -1);
    s->comm = comm;
    if (comm) comm_attach(comm, +1);
    return MH_OK;
}

int mh_scene_synchronize(mh_scene *s) {
    if (!s) return set_error(MH_ERR_INVALID_ARGUMENT, "mh_scene_synchronize: NULL scene");
    MH_HIP(hipSetDevice(s->device));
    MH_HIP(hipStreamSynchronize(s->stream));
    return check_bounds_counter(s, "mh_scene_synchronize");
}

}  // extern "C"

namespace {

// slab i of n: samples [spp*i/n, spp*(i+1)/n) of every pixel
uint32_t slab_edge(uint32_t spp, uint32_t i, uint32_t n) { return (uint32_t)((uint64_t)spp * i / n); }

// fn(i) for every scene, each on a host thread of its own: the devices (and
// streams) then run concurrently although every call synchronises, and an
// in-call collective finds all of its ranks issued.  The first failure wins.
template <class F>
int for_each_scene(uint32_t n, F fn) {
    std::vector<int> rc(n, MH_OK);
    std::vector<std::string> msg(n);
    std::vector<std::thread> th;
    th.reserve(n);
    for (uint32_t i = 0; i < n; ++i)
        th.emplace_back([&, i] {
            rc[i] = fn(i);
            if (rc[i]) msg[i] = g_error;  // the worker thread's own message
        });
    for (auto &t : th) t.join();
    for (uint32_t i = 0; i < n; ++i)
        if (rc[i]) return set_error(rc[i], "scene " + std::to_string(i) + ": " + msg[i]);
    return MH_OK;
}

// argument checks shared by the sharded entry points; *comm = every scene
// has a communicator whose ranks are the scenes' order (else none may have one)
int check_shards(mh_scene *const *sc, uint32_t n, uint32_t spp, const char *api, bool *comm) {
    const std::string a(api);
    if (!sc || n == 0) return set_error(MH_ERR_INVALID_ARGUMENT, a + ": no scenes");
    if (spp < n) return set_error(MH_ERR_INVALID_ARGUMENT, a + ": spp must be >= the number of scenes (one slab each)");
    uint32_t with = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!sc[i]) return set_error(MH_ERR_INVALID_ARGUMENT, a + ": NULL scene");
        for (uint32_t j = 0; j < i; ++j)
            if (sc[j] == sc[i]) return set_error(MH_ERR_INVALID_ARGUMENT, a + ": a scene appears twice (one per slab)");
        if (sc[i]->S.width != sc[0]->S.width || sc[i]->S.height != sc[0]->S.height ||
            sc[i]->pixel_format != sc[0]->pixel_format)
            return set_error(MH_ERR_INVALID_ARGUMENT, a + ": the scenes' films differ");
        with += sc[i]->comm ? 1u : 0u;
    }
    if (with != 0 && with != n)
        return set_error(MH_ERR_INVALID_ARGUMENT, a + ": either every scene has a communicator or none has");
    for (uint32_t i = 0; i < with; ++i) {
        int nr = 0, r = 0;
        mh_comm_info(sc[i]->comm, &nr, &r, nullptr);
        if (nr != (int)n || r != (int)i)
            return set_error(MH_ERR_INVALID_ARGUMENT, a + ": scene i's communicator must be rank i of n");
    }
    *comm = with == n;
    return MH_OK;
}

// the sum without a communicator: bufs[i] (count floats on scene i's device)
// are copied onto scene 0's device (peer copies; a plain device copy when the
// scenes share it) and added into bufs[0] in scene order; `all` copies the
// sum back to every bufs[i].  Every stream has drained before and after.
int peer_sum(mh_scene *const *sc, uint32_t n, float *const *bufs, uint64_t count, bool all) {
    mh_scene *s0 = sc[0];
    MH_HIP(hipSetDevice(s0->device));
    MH_HIP(s0->shard_tmp.alloc(count * 4));
    for (uint32_t i = 1; i < n; ++i) {
        MH_HIP(hipMemcpyPeerAsync(s0->shard_tmp.ptr, s0->device, bufs[i], sc[i]->device, count * 4, s0->stream));
        MH_HIP(launch_accumulate(bufs[0], s0->shard_tmp.as<float>(), count, s0->stream));
    }
    if (all)
        for (uint32_t i = 1; i < n; ++i)
            MH_HIP(hipMemcpyPeerAsync(bufs[i], sc[i]->device, bufs[0], s0->device, count * 4, s0->stream));
    MH_HIP(hipStreamSynchronize(s0->stream));
    return MH_OK;
}

}  // namespace

extern "C" {

int mh_render_sharded(mh_scene *const *scenes, uint32_t n, const mh_integrator *in, uint32_t seed, uint32_t spp,
                      float *const *films, uint32_t flags, mh_stats *stats) {
    ScopedPhase phase_("Render");
    bool comm = false;
    if (int rc = check_shards(scenes, n, spp, "mh_render_sharded", &comm)) return rc;
    if (!in || !films) return set_error(MH_ERR_INVALID_ARGUMENT, "mh_render_sharded: NULL argument");
    for (uint32_t i = 0; i < n; ++i)
        if (!films[i]) return set_error(MH_ERR_INVALID_ARGUMENT, "mh_render_sharded: NULL film");
    if (flags & MH_FLAG_ACCUMULATE)
        return set_error(MH_ERR_INVALID_ARGUMENT, "mh_render_sharded: MH_FLAG_ACCUMULATE is not supported (the sum "
                                                  "would count the accumulated film once per scene)");
    const uint32_t pass = (flags & (MH_FLAG_DETERMINISTIC | MH_FLAG_MEGAKERNEL | MH_FLAG_WAVEFRONT)) |
                          MH_FLAG_DEVICE_POINTERS;
    const uint32_t red = comm ? ((flags & MH_FLAG_REDUCE) ? MH_FLAG_REDUCE : MH_FLAG_REDUCE_ROOT) : 0u;
    int rc = for_each_scene(n, [&](uint32_t i) {
        return mh_render(scenes[i], in, seed, spp, slab_edge(spp, i, n), slab_edge(spp, i + 1, n), films[i],
                         pass | red, stats ? &stats[i] : nullptr);
    });
    if (rc || comm) return rc;
    const uint64_t count = (uint64_t)scenes[0]->S.width * scenes[0]->S.height * (has_alpha(scenes[0]->pixel_format) ? 5 : 4);
    return peer_sum(scenes, n, films, count, flags & MH_FLAG_REDUCE);
}

int mh_render_backward_sharded(mh_scene *const *scenes, uint32_t n, const mh_integrator *in, uint32_t seed,
                               uint32_t spp, const float *const *grad_in, uint32_t n_params,
                               const uint32_t *param_tex, float *const *grads, uint32_t flags, mh_stats *stats) {
    ScopedPhase phase_("RenderBackward");
    bool comm = false;
    if (int rc = check_shards(scenes, n, spp, "mh_render_backward_sharded", &comm)) return rc;
    if (!in || !grad_in || (n_params && (!param_tex || !grads)))
        return set_error(MH_ERR_INVALID_ARGUMENT, "mh_render_backward_sharded: NULL argument");
    const uint32_t pass = (flags & (MH_FLAG_DETERMINISTIC | MH_FLAG_MEGAKERNEL | MH_FLAG_PRB_REPLAY)) |
                          MH_FLAG_DEVICE_POINTERS;
    if (comm)  // every rank: slab W + all-reduce, its slab's gradient, all-reduce (mh_render_backward in-call)
        return for_each_scene(n, [&](uint32_t i) {
            return mh_render_backward(scenes[i], in, seed, spp, slab_edge(spp, i, n), slab_edge(spp, i + 1, n),
                                      grad_in[i], nullptr, n_params, param_tex, grads + (size_t)i * n_params,
                                      pass | MH_FLAG_REDUCE | (flags & MH_FLAG_LOCAL_WEIGHTS),
                                      stats ? &stats[i] : nullptr);
        });
    // without communicators: the slab W images summed onto every scene ...
    const uint64_t n_px = (uint64_t)scenes[0]->S.width * scenes[0]->S.height;
    std::vector<float *> wb(n), gb(n);
    for (uint32_t i = 0; i < n; ++i) {
        MH_HIP(hipSetDevice(scenes[i]->device));
        MH_HIP(scenes[i]->shard_w.alloc(n_px * 4));
        wb[i] = scenes[i]->shard_w.as<float>();
    }
    int rc = for_each_scene(n, [&](uint32_t i) {
        return mh_prb_weights(scenes[i], seed, spp, slab_edge(spp, i, n), slab_edge(spp, i + 1, n), wb[i],
                              pass & (MH_FLAG_DEVICE_POINTERS | MH_FLAG_DETERMINISTIC));
    });
    if (rc) return rc;
    if ((rc = peer_sum(scenes, n, wb.data(), n_px, true))) return rc;
    // ... each slab's gradient into zeroed per-scene buffers, summed, then
    // accumulated into the caller's buffers as mh_render_backward does
    Slots P;
    if ((rc = build_slots(scenes[0], n_params, param_tex, in->type == MH_INTEGRATOR_PRBVOLPATH,
                          "mh_render_backward_sharded", "render_backward", P)))
        return rc;
    std::vector<uint64_t> off(n_params + 1, 0);
    for (uint32_t k = 0; k < n_params; ++k) off[k + 1] = off[k] + P.counts[P.slot_of_param[k]];
    const uint64_t total = std::max<uint64_t>(off[n_params], 1);
    for (uint32_t i = 0; i < n; ++i) {
        MH_HIP(hipSetDevice(scenes[i]->device));
        MH_HIP(scenes[i]->shard_g.alloc(total * 4));
        gb[i] = scenes[i]->shard_g.as<float>();
        MH_HIP(hipMemsetAsync(gb[i], 0, total * 4, scenes[i]->stream));
        MH_HIP(hipStreamSynchronize(scenes[i]->stream));
    }
    rc = for_each_scene(n, [&](uint32_t i) {
        std::vector<float *> gp(std::max<uint32_t>(n_params, 1));
        for (uint32_t k = 0; k < n_params; ++k) gp[k] = gb[i] + off[k];
        return mh_render_backward(scenes[i], in, seed, spp, slab_edge(spp, i, n), slab_edge(spp, i + 1, n),
                                  grad_in[i], wb[i], n_params, param_tex, gp.data(), pass, stats ? &stats[i] : nullptr);
    });
    if (rc) return rc;
    if ((rc = peer_sum(scenes, n, gb.data(), total, true))) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        MH_HIP(hipSetDevice(scenes[i]->device));
        for (uint32_t k = 0; k < n_params; ++k) {
            if (!grads[(size_t)i * n_params + k])
                return set_error(MH_ERR_INVALID_ARGUMENT, "mh_render_backward_sharded: NULL gradient buffer");
            MH_HIP(launch_accumulate(grads[(size_t)i * n_params + k], gb[i] + off[k], off[k + 1] - off[k],
                                     scenes[i]->stream));
        }
        MH_HIP(hipStreamSynchronize(scenes[i]->stream));
    }
    return MH_OK;
}

}  // extern "C"
