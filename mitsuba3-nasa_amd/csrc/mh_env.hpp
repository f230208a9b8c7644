// mh_env.hpp — the one place that reads the process environment (host only).
//
// Every MH_* variable of the library is a row of MH_ENV_TABLE; the row names
// its accessor (mh::env::<fn>), and no other file of csrc/ calls getenv.
// Nothing is cached here: an accessor reads the variable when it is called, so
// a variable read per call stays per call (callers that read once keep their
// own static).  INTEGRATION.md §"Environment variables" lists the same rows.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>

namespace mh {
namespace env {

// kinds (the accessor's shape)
//   Present  bool fn()          set to anything, the empty string included
//   Is       bool fn()          equals `val` exactly ("1" on, "0" off, or a
//                               string choice); any other value is the default
//   Int      int fn(int dflt)   atoi, clamped to [lo, hi]; dflt when unset
//   U64      uint64_t fn()      strtoull, at least lo; 0 when unset
//   Real     double fn(double)  atof, at least lo if lo > 0; dflt when unset
enum class Kind { Present, Is, Int, U64, Real };
// for release builds, for diagnostics / experiments, or for the test suite
enum class Use { Release, Diagnostic, TestHook };

struct Var {
    const char *name;
    Kind kind;
    const char *val;   // Is: the value that counts
    double lo, hi;     // the clamp
    const char *dflt;  // behaviour when unset (documentation)
    Use use;
    const char *doc;
};

// X(fn, name, kind, val, lo, hi, default, use,
//   doc)
#define MH_ENV_TABLE(X)                                                                                   \
    X(deterministic, "MH_DETERMINISTIC", Is, "1", 0, 0, "off", Release,                                   \
      "as MH_FLAG_DETERMINISTIC on every call: fixed-order splat and gradient sums")                      \
    X(mode_mega, "MH_MODE", Is, "mega", 0, 0, "per call", Release,                                        \
      "mega: every render / backward / forward call runs its megakernel (as MH_FLAG_MEGAKERNEL)")         \
    X(wf_one_stream, "MH_WF_STREAMS", Is, "1", 0, 0, "two streams", Release,                              \
      "1: the wavefront's chunks stay on the scene's stream (no second stream)")                          \
    X(wf_chunk, "MH_WF_CHUNK", U64, "", 1024, 0, "the wavefront's limit (2^25)", Release,                 \
      "samples per wavefront chunk, at least 1024 and at most the limit")                                 \
    X(vol_mode_rounds, "MH_VOL_MODE", Is, "rounds", 0, 0, "phase scheduler", Release,                     \
      "rounds: volpath as main / walk rounds instead of the phase scheduler")                             \
    X(traversal_lane, "MH_TRAVERSAL", Is, "lane", 0, 0, "packet", Release,                                \
      "lane: per-lane traversal also for scenes the packet engine takes (packet: the default)")           \
    X(prb_replay, "MH_PRB_REPLAY", Is, "1", 0, 0, "off", Release,                                         \
      "1: prb's backward pass on the replay kernel (as MH_FLAG_PRB_REPLAY)")                              \
    X(comm_timeout_s, "MH_COMM_TIMEOUT_S", Real, "", 0.001, 0, "1800", Release,                           \
      "deadline of a collective call's wait in seconds, at least 0.001 (read once)")                      \
    X(bvh_threads, "MH_BVH_THREADS", Int, "", 1, INT_MAX, "hardware threads, at most 32", Release,        \
      "threads of the host BVH build")                                                                    \
    X(wf_unfused, "MH_WF_FUSED", Is, "0", 0, 0, "fused", Diagnostic,                                      \
      "0: the three-kernel trace / shade / shadow pipeline instead of the fused bounce kernel")           \
    X(prb_bmp_wf_off, "MH_PRB_BMP_WF", Is, "0", 0, 0, "on", Diagnostic,                                   \
      "0: bitmap parameters on the replay kernel instead of the wavefront's record log")                  \
    X(prb_lds_tex_off, "MH_PRB_LDS_TEX", Is, "0", 0, 0, "on", Diagnostic,                                 \
      "0: bitmap texel gradients through global atomics, never an LDS accumulator")                       \
    X(pvp_nee_log_off, "MH_PVP_NEE_LOG", Is, "0", 0, 0, "on", Diagnostic,                                 \
      "0: prbvolpath's backward replays its NEE walks (no per-thread logs)")                              \
    X(pvp_single_off, "MH_PVP_SINGLE", Is, "0", 0, 0, "on", Diagnostic,                                   \
      "0: prbvolpath's backward without the MainLog (primal + adjoint replay per sample)")                \
    X(pvp_sched_off, "MH_PVP_SCHED", Is, "0", 0, 0, "on", Diagnostic,                                     \
      "0: prbvolpath's backward on the per-sample kernel instead of the phase scheduler")                 \
    X(pvp_main_cap, "MH_PVP_MAIN_CAP", Int, "", 1, INT_MAX, "256", Diagnostic,                            \
      "MainLog entries per thread of prbvolpath's backward")                                              \
    X(grid_corner_off, "MH_GRID_CORNER", Is, "0", 0, 0, "on", Diagnostic,                                 \
      "0: grid sigma_t gradients through direct atomics (no per-cell corner blocks)")                     \
    X(bvh4_off, "MH_BVH4", Is, "0", 0, 0, "on", Diagnostic,                                               \
      "0: BVH2 for every scene (no collapsed BVH4)")                                                      \
    X(bvh4q, "MH_BVH4Q", Is, "1", 0, 0, "off", Diagnostic,                                                \
      "1: the quantised BVH4 with compact primitive records")                                             \
    X(primc, "MH_PRIMC", Is, "1", 0, 0, "off", Diagnostic,                                                \
      "1: compact 48-byte triangle records beside the float BVH4")                                        \
    X(bvh_leaf, "MH_BVH_LEAF", Int, "", 2, 31, "12 (<= 64 primitives) or 8", Diagnostic,                  \
      "largest BVH leaf")                                                                                 \
    X(bvh_ct, "MH_BVH_CT", Real, "", 0, 0, "4 (<= 64 primitives) or 2", Diagnostic,                       \
      "SAH traversal cost of the BVH build (not clamped)")                                                \
    X(stream_stack, "MH_STREAM_STACK", Int, "", 4, INT_MAX, "20", Diagnostic,                             \
      "LDS entries of the stream engine's traversal stack; deeper ones go to global memory")              \
    X(packet_max_prims, "MH_PACKET_MAX_PRIMS", Int, "", 1, INT_MAX, "64", Diagnostic,                     \
      "largest scene (primitives) the packet engine traces (read once)")                                  \
    X(wf_bpc, "MH_WF_BPC", Int, "", 1, INT_MAX, "30, or 12 on a shared device", Diagnostic,               \
      "wavefront workgroups per CU")                                                                      \
    X(vs_bpc, "MH_VS_BPC", Int, "", 1, INT_MAX, "2 (one resident round)", Diagnostic,                     \
      "phase-scheduler workgroups per CU")                                                                \
    X(vw_bpc, "MH_VW_BPC", Int, "", 1, INT_MAX, "8", Diagnostic,                                          \
      "workgroups per CU of volpath's rounds mode")                                                       \
    X(vw_rounds, "MH_VW_ROUNDS", Int, "", 1, INT_MAX, "6", Diagnostic,                                    \
      "rounds of volpath's rounds mode before its finish launch")                                         \
    X(vs_notab, "MH_VS_NOTAB", Present, "", 0, 0, "unset", Diagnostic,                                    \
      "set: the phase scheduler without the LDS shading tables")                                          \
    X(vw_debug, "MH_VW_DEBUG", Present, "", 0, 0, "unset", Diagnostic,                                    \
      "set: volpath / prbvolpath print per-phase and per-round statistics to stderr")                     \
    X(pvp_nee_cap, "MH_PVP_NEE_CAP", Int, "", 1, INT_MAX, "256", TestHook,                                \
      "NeeLog entries per thread; small logs exercise the replay fallback")                               \
    X(test_fail_after_issue, "MH_TEST_FAIL_AFTER_ISSUE", Present, "", 0, 0, "unset", TestHook,            \
      "set: a call with MH_FLAG_REDUCE fails after it was issued (communicator failure semantics)")       \
    X(test_comm_scale, "MH_TEST_COMM_SCALE", Present, "", 0, 0, "unset", TestHook,                        \
      "set: a one-rank all-reduce doubles its buffer, so a test sees that it ran")

#define MH_ENV_ROW(fn, name, kind, val, lo, hi, dflt, use, doc) {name, Kind::kind, val, lo, hi, dflt, Use::use, doc},
constexpr Var kVars[] = {MH_ENV_TABLE(MH_ENV_ROW)};
#undef MH_ENV_ROW

// ---- the parse helpers, and one accessor per row ----------------------------
inline bool present(const char *name) { return getenv(name) != nullptr; }
inline bool is(const char *name, const char *val) {
    const char *e = getenv(name);
    return e && !strcmp(e, val);
}
inline int clamped(const char *name, int lo, int hi, int dflt) {
    const char *e = getenv(name);
    return e ? std::max(lo, std::min(hi, atoi(e))) : dflt;
}
inline double real(const char *name, double lo, double dflt) {  // lo: 0 = no clamp
    const char *e = getenv(name);
    return !e ? dflt : lo > 0 ? std::max(lo, atof(e)) : atof(e);
}
inline uint64_t at_least(const char *name, uint64_t lo) {  // 0: unset
    const char *e = getenv(name);
    return e ? std::max<uint64_t>(lo, strtoull(e, nullptr, 10)) : 0;
}
#define MH_ENV_FN_Present(fn, name, val, lo, hi) inline bool fn() { return present(name); }
#define MH_ENV_FN_Is(fn, name, val, lo, hi) inline bool fn() { return is(name, val); }
#define MH_ENV_FN_Int(fn, name, val, lo, hi) inline int fn(int dflt) { return clamped(name, lo, hi, dflt); }
#define MH_ENV_FN_U64(fn, name, val, lo, hi) inline uint64_t fn() { return at_least(name, lo); }
#define MH_ENV_FN_Real(fn, name, val, lo, hi) inline double fn(double dflt) { return real(name, lo, dflt); }
#define MH_ENV_FN(fn, name, kind, val, lo, hi, dflt, use, doc) MH_ENV_FN_##kind(fn, name, val, lo, hi)
MH_ENV_TABLE(MH_ENV_FN)
#undef MH_ENV_FN

// ---- the switches the planners consume (mh_plan.hpp) -------------------------
// A snapshot taken once at the top of a call, so that every decision of the
// call sees the same values; each call reads only what its planner consumes.
struct PlanEnv {
    bool deterministic = false, mode_mega = false, wf_one_stream = false;
    uint64_t wf_chunk = 0;  // 0: unset
    // mh_render_backward, and its prbvolpath branch (caps: 0 = unset)
    bool prb_replay = false, prb_bmp_wf_off = false, prb_lds_tex_off = false;
    bool pvp_nee_log_off = false, pvp_single_off = false, pvp_sched_off = false;
    uint32_t pvp_main_cap = 0, pvp_nee_cap = 0;
};
enum class Call { Render, Backward, BackwardVol, Forward };
inline PlanEnv plan_env(Call c) {
    PlanEnv e;
    e.deterministic = deterministic();
    e.mode_mega = mode_mega();
    if (c == Call::Forward) return e;
    e.wf_one_stream = wf_one_stream();
    e.wf_chunk = wf_chunk();
    if (c == Call::Render) return e;
    e.prb_replay = prb_replay();
    e.prb_bmp_wf_off = prb_bmp_wf_off();
    e.prb_lds_tex_off = prb_lds_tex_off();
    if (c == Call::Backward) return e;
    e.pvp_nee_log_off = pvp_nee_log_off();
    e.pvp_single_off = pvp_single_off();
    e.pvp_sched_off = pvp_sched_off();
    e.pvp_main_cap = (uint32_t)pvp_main_cap(0);
    e.pvp_nee_cap = (uint32_t)pvp_nee_cap(0);
    return e;
}

}  // namespace env
}  // namespace mh
