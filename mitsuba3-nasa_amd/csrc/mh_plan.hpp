// mh_plan.hpp — how a call runs, decided from plain values (host only).
//
// mh_render, mh_render_backward and mh_render_forward (mh_api.hip) fill the
// facts of their call, ask the planner once and carry the plan out.  The
// planners call neither HIP nor the environment and hold no state, so every
// rule is checked without a GPU (tools/plan_check.cpp, tests/test_plan_host.py).
#pragma once

#include <stdint.h>

#include <algorithm>

#include "../../include/mitsuba_hip.h"
#include "mh_env.hpp"

namespace mh {
namespace plan {

using env::PlanEnv;

// a single-chunk wavefront call of at least this many samples is split in two,
// so that it can use both streams
constexpr uint64_t kTwoStreamMinSamples = 1ull << 19;
// prbvolpath backward: NEE-log entries per thread (16 B each; longer walks
// replay) and MainLog entries per thread (64 B each: 4 GiB over the 262,144
// threads of a 256-CU grid; a path with more logged vertices replays its adjoint)
constexpr uint32_t kPvpNeeCap = 256, kPvpMainCap = 256;

// MH_FLAG_DETERMINISTIC or MH_DETERMINISTIC=1: fixed-order splat and gradient sums
inline bool deterministic(uint32_t flags, bool env_on) { return (flags & MH_FLAG_DETERMINISTIC) || env_on; }
inline bool megakernel(uint32_t flags, const PlanEnv &e) { return (flags & MH_FLAG_MEGAKERNEL) || e.mode_mega; }
// samples per wavefront chunk: MH_WF_CHUNK, at most wf_max_chunk()
inline uint64_t wf_chunk_samples(const PlanEnv &e, uint64_t wf_max) {
    return std::min<uint64_t>(wf_max, e.wf_chunk ? e.wf_chunk : wf_max);
}
// bitmap vertex records of the backward wavefront: 48 B per path and depth, at
// most 8 GiB of them per chunk (but chunks of at least 2^16 samples)
inline uint64_t bmp_record_cap(uint32_t n_depth) {
    return std::max<uint64_t>(1 << 16, (8ull << 30) / (48ull * n_depth));
}
// The chunks may alternate between the scene's two streams only where they
// share nothing but atomically updated outputs (not deterministic), and not
// with MH_FLAG_SHARED_DEVICE (the caller already runs another call beside this
// one) or MH_WF_STREAMS=1.
inline bool two_streams_ok(uint32_t flags, const PlanEnv &e) {
    return !deterministic(flags, e.deterministic) && !(flags & MH_FLAG_SHARED_DEVICE) && !e.wf_one_stream;
}

// The film cut into chunks of chunk_px pixels (per_pixel samples each, at most
// max_samples per chunk); two: the chunks alternate between two streams.
struct Split {
    uint32_t chunk_px = 0;
    uint64_t n_chunks = 0;
    bool two = false;
};
inline Split split_chunks(uint64_t n_px, uint64_t per_pixel, uint64_t max_samples, bool two_ok) {
    Split c;
    c.chunk_px = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_px, max_samples / per_pixel));
    if (two_ok && c.chunk_px >= n_px && n_px >= 2 && n_px * per_pixel >= kTwoStreamMinSamples)
        c.chunk_px = (uint32_t)((n_px + 1) / 2);
    c.two = two_ok && c.chunk_px < n_px;
    c.n_chunks = (n_px + c.chunk_px - 1) / c.chunk_px;
    return c;
}

// k_vol_sched keeps the tables of the tabulated phase functions in LDS (a
// sample or an evaluation is a dependent chain of about log2(nodes) loads) when
// they fit beside what the launch already holds there -- BVH, traversal
// stacks, shading tables, media records, deferral scratch, the machine's
// static arrays -- within the 64 KiB of a workgroup; else they stay in global
// memory.  The results are the same either way.
constexpr uint64_t kLdsPerWorkgroup = 65536;
inline uint32_t phase_lds_bytes(uint32_t table_bytes, uint64_t other_lds_bytes) {
    return table_bytes && other_lds_bytes <= kLdsPerWorkgroup && table_bytes <= kLdsPerWorkgroup - other_lds_bytes
               ? table_bytes : 0u;
}

// What a call knows about itself and its scene.
struct Facts {
    uint32_t type = 0, max_depth = 0, flags = 0;  // the integrator, the call's flags
    uint64_t n_px = 0;
    uint32_t spp = 1, n_passes = 1;     // samples per pixel of the slab; passes (mh_render)
    bool wf_fused = false;              // wf_fused(S): packet-engine scene on the fused bounce kernel
    bool vs_ok = false, vw_ok = false;  // vs_supported / vw_supported
    bool vol_sched = true;              // vol_sched_mode() (mh_render)
    uint64_t wf_max = 0, vw_max = 0;    // wf_max_chunk(), vw_max_chunk()
    // mh_render_backward: the parameter slots
    uint32_t n_rgb = 0, n_bmp = 0;
    bool bmp_same_ch = true;      // every bitmap parameter has the same channel count
    uint64_t bmp_slot_bytes = 0;  // bytes of the first bitmap slot
    uint32_t n_phase_params = 0;  // '<medium>.phase_function.g' keys (prbvolpath)
};

// ---- mh_render --------------------------------------------------------------
struct RenderPlan {
    int err = MH_OK;         // MH_ERR_UNSUPPORTED: MH_FLAG_WAVEFRONT on a call the wavefront cannot take
    bool wavefront = false;  // `path` on the wavefront kernels
    bool volwave = false;    // volpath on the phase scheduler (sched) or as main / walk rounds
    bool sched = false;
    uint32_t mode = 0;       // as mh_stats reports it: 0 megakernel, 1 / 2 unfused / fused wavefront, 3 volpath
    bool determ = false;
    uint64_t max_samples = 0;
    Split chunks;
};
inline RenderPlan plan_render(const Facts &f, const PlanEnv &e) {
    RenderPlan p;
    // `path` of bounded depth; several passes only on the fused bounce kernel,
    // which carries each lane's PCG32 state from one pass to the next.  volpath: single pass.
    // max_depth 0 launches no bounce kernel, and the fused wavefront's first
    // bounce is what writes a sample's position: the per-lane kernel takes it
    p.wavefront = f.type == MH_INTEGRATOR_PATH && f.max_depth >= 1 && f.max_depth <= 64 &&
                  (f.n_passes == 1 || f.wf_fused);
    p.volwave = (f.vol_sched ? f.vs_ok : f.vw_ok) && f.n_passes == 1;
    if (megakernel(f.flags, e)) p.wavefront = p.volwave = false;
    if ((f.flags & MH_FLAG_WAVEFRONT) && !p.wavefront && !p.volwave) p.err = MH_ERR_UNSUPPORTED;
    p.sched = p.volwave && f.vol_sched;
    p.mode = p.wavefront ? (f.wf_fused ? 2u : 1u) : p.volwave ? 3u : 0u;
    p.determ = deterministic(f.flags, e.deterministic);
    p.max_samples = p.wavefront ? wf_chunk_samples(e, f.wf_max) : p.volwave ? f.vw_max : 1ull << 25;
    // (two streams: the unfused stream-engine kernels of large meshes too)
    p.chunks = split_chunks(f.n_px, (uint64_t)f.spp * f.n_passes, p.max_samples,
                            p.wavefront && two_streams_ok(f.flags, e));
    return p;
}

// ---- mh_render_backward -----------------------------------------------------
struct BackwardPlan {
    bool replay = false;      // forced: MH_FLAG_PRB_REPLAY / MH_PRB_REPLAY=1
    bool mega = false;        // forced: MH_FLAG_MEGAKERNEL / MH_MODE=mega
    bool fused = false;       // every parameter an rgb constant: one fused traversal
    bool bmp_wf = false;      // bitmap parameters: the fused wavefront logs their vertices, a scatter charges the texels
    bool wavefront = false;   // fused or bmp_wf as wavefront kernels; else the per-lane kernel
    bool determ = false;
    bool fx = false;          // prbvolpath, deterministic: int64 fixed point in two passes, also the small slots
    bool det_replay = false;  // the same form on prb's replay kernel (bitmaps the wavefront cannot take, forced replay, megakernel)
    bool fxr = false;         // fx || det_replay
    bool det_grad = false;    // wavefront, deterministic: rgb slots summed per path, reduced in a fixed order
    bool lds_tex = false;     // replay kernel: the one bitmap slot accumulates per workgroup in LDS
    bool bmp_lds = false;     // wavefront texel scatter: LDS accumulation allowed
    uint32_t n_depth = 0;     // wavefront: vertex records per path
    uint64_t max_samples = 0;
    Split chunks;             // wavefront only
    // prbvolpath
    bool pvp_log = false;  // persistent grid with per-thread logs (MH_PVP_NEE_LOG=0: the NEE walks are replayed)
    uint32_t main_cap = 0, nee_cap = 0;  // MainLog (0: none, MH_PVP_SINGLE=0) and NeeLog entries per thread
    bool sched = false;    // the phase scheduler is wanted (MH_PVP_SCHED=0: no); the logs' allocations may still refuse
};
inline BackwardPlan plan_backward(const Facts &f, const PlanEnv &e) {
    BackwardPlan p;
    const bool vol = f.type == MH_INTEGRATOR_PRBVOLPATH;
    p.determ = deterministic(f.flags, e.deterministic);
    p.fx = vol && p.determ;
    p.replay = (f.flags & MH_FLAG_PRB_REPLAY) || e.prb_replay;
    p.mega = megakernel(f.flags, e);
    p.fused = !vol && f.n_bmp == 0 && !p.replay;
    // bitmaps: packet-engine scenes, max_depth <= 32, all with the same channel
    // count (as the scatter's transposed issue assumes); MH_PRB_BMP_WF=0: replay
    p.bmp_wf = !vol && f.n_bmp >= 1 && f.bmp_same_ch && !p.replay && !p.mega && f.wf_fused && f.max_depth >= 1 &&
               f.max_depth <= 32 && !e.prb_bmp_wf_off;
    // max_depth 0: prb still adds the emitter its camera ray sees (prb.py:121-135), whose
    // radiance may be differentiated; the wavefront would launch no bounce kernel at all
    p.wavefront = (p.fused && f.max_depth >= 1 && f.max_depth <= 64 && !p.mega) || p.bmp_wf;
    p.det_replay = p.determ && !vol && !p.wavefront;
    p.fxr = p.fx || p.det_replay;
    // one bitmap parameter of <= 48 KiB (det_replay switches it off again: no LDS accumulator there)
    p.lds_tex = f.n_bmp == 1 && f.bmp_slot_bytes <= (48u << 10) && !e.prb_lds_tex_off;
    p.bmp_lds = !e.prb_lds_tex_off;
    if (p.wavefront) {
        p.max_samples = wf_chunk_samples(e, f.wf_max);
        p.n_depth = std::max<uint32_t>(1, f.max_depth - 1);
        if (p.bmp_wf) p.max_samples = std::min<uint64_t>(p.max_samples, bmp_record_cap(p.n_depth));
        // two streams: float gradients only (per-stream block partials, atomic texel scatter)
        p.chunks = split_chunks(f.n_px, f.spp, p.max_samples, two_streams_ok(f.flags, e));
        p.det_grad = p.determ && f.n_rgb > 0;
    } else if (vol && !e.pvp_nee_log_off) {
        p.pvp_log = true;
        p.main_cap = e.pvp_single_off ? 0u : e.pvp_main_cap ? e.pvp_main_cap : kPvpMainCap;
        p.nee_cap = e.pvp_nee_cap ? e.pvp_nee_cap : kPvpNeeCap;
        // a phase-function parameter: the per-lane kernel with its logs (k_prbvol_backward's PhG
        // instances); the scheduler machines, at 248-256 VGPRs, have no instance with its terms
        p.sched = p.main_cap && f.vs_ok && !e.pvp_sched_off && f.n_phase_params == 0;
    }
    return p;
}

// ---- mh_render_forward ------------------------------------------------------
struct ForwardPlan {
    bool wavefront = false;  // prb on packet-engine scenes: the fused forward-mode wavefront; else the per-sample kernel
    uint32_t mode = 0;       // as mh_stats reports it: 2 / 0
    bool determ = false;
    uint32_t chunk_px = 0;
};
inline ForwardPlan plan_forward(const Facts &f, const PlanEnv &e) {
    ForwardPlan p;
    p.wavefront = f.type == MH_INTEGRATOR_PRB && f.wf_fused && f.max_depth >= 1 && f.max_depth <= 64 &&
                  !megakernel(f.flags, e);
    p.mode = p.wavefront ? 2u : 0u;
    p.determ = deterministic(f.flags, e.deterministic);
    p.chunk_px = split_chunks(f.n_px, f.spp, f.wf_max, false).chunk_px;
    return p;
}

}  // namespace plan
}  // namespace mh
