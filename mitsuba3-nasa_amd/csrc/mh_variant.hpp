// mh_variant.hpp — which kernel instance a launch uses, decided from plain
// values (host only).
//
// A launcher (mh_kernels.hip, mh_wavefront.hip, mh_volwave.hip) fills the
// facts of its scene and call and asks its kernel family's selector, which
// calls the launcher's generic lambda f with the kernel's template arguments
// as std::integral_constant values (through a key and dispatch(key, f) where
// a launcher uses one selection for several launches).  Every selector lists
// the values each argument may take, so exactly the instances that can be
// selected are compiled.  The selectors call neither HIP nor the environment
// and hold no state, so every rule is checked without a GPU
// (tools/variant_check.cpp, tests/test_variant_host.py).
#pragma once

#include <stdint.h>

#include <type_traits>

#include "../../include/mitsuba_hip.h"

namespace mh {
namespace variant {

// ---- runtime value -> template argument ---------------------------------------
// among<V0, V1, ...>(v): v is one of the listed values; flag(b): a bool.
template <class T, T... Vs>
struct Among {
    T v;
};
template <auto V0, auto... Vs>
constexpr Among<decltype(V0), V0, Vs...> among(decltype(V0) v) { return {v}; }
constexpr Among<bool, false, true> flag(bool v) { return {v}; }
// select(f, axes...): f(std::integral_constant<T, V>{}...) for the listed V
// that each axis holds; false (and no call) if some axis holds none of its list
template <class F>
bool select(F &&f) { return f(), true; }
template <class F, class T, T... Vs, class... Rest>
bool select(F &&f, Among<T, Vs...> a, Rest... rest) {
    return ((a.v == Vs && select([&](auto... cs) { f(std::integral_constant<T, Vs>{}, cs...); }, rest...)) || ...);
}

// ---- the facts ------------------------------------------------------------------
// the phase functions compiled into a volumetric kernel (mh_shading.hpp's
// kPh*), the stream engines (its kEng*) and DScene::vol_flags' bits
// (mh_device.hpp); mh_wavefront.hip asserts that they are the same values
constexpr int kPhExt = 1, kPhBlend = 2;
constexpr int kEngBvh2 = 0, kEngWide = 1, kEngQuant = 2, kEngWideC = 3;
constexpr uint32_t kVolPhaseExt = 4u, kVolPhaseBlend = 8u;

struct Facts {
    bool bvh_lds = false;  // the kernels stage the BVH in LDS (DScene::lds_bytes_bvh != 0)
    uint32_t n_prims = 0, packet_max_prims = 0;  // pair records exist up to wf_packet_max_prims()
    bool tables = false;   // shading tables to stage in LDS (DScene::tab_bytes != 0)
    uint32_t vol_flags = 0;
    int stream_eng = kEngBvh2;  // stream_engine(S): the engine of the scene's node format
    bool traversal_lane = false, vs_notab = false, wf_unfused = false;  // MH_TRAVERSAL=lane, MH_VS_NOTAB, MH_WF_FUSED=0
};

// wave-coherent packet traversal: scenes with pair records.  The wavefront
// takes an empty scene as a packet scene, the volumetric kernels do not.
inline bool wf_packet(const Facts &f) { return f.n_prims <= f.packet_max_prims && !f.traversal_lane; }
inline bool vol_packet(const Facts &f) { return f.n_prims > 0 && wf_packet(f); }
inline bool wf_fused(const Facts &f) { return wf_packet(f) && f.tables && !f.wf_unfused; }
inline bool blend(const Facts &f) { return (f.vol_flags & kVolPhaseBlend) != 0; }
// every volumetric kernel but volpath's scheduler machine is compiled with rayleigh and tabphase
inline int phase_level(const Facts &f) { return blend(f) ? kPhBlend : kPhExt; }

// where a volumetric kernel's traversal data lives (its <InLds, Pk[, Tab]>):
// global memory, LDS, packets, or packets with the shading tables in LDS
struct Home {
    bool lds, packet, tab;
};
inline Home home(const Facts &f, bool tab_ok) {
    const bool pk = vol_packet(f);
    return {!pk && f.bvh_lds, pk, pk && tab_ok && f.tables};
}
// f(axes..., InLds, Pk, Tab)
template <class F, class... A>
bool select_home(const Home &h, F &&f, A... axes) {
    return h.packet ? select(f, axes..., among<false>(h.lds), among<true>(h.packet), flag(h.tab))
                    : select(f, axes..., flag(h.lds), among<false>(h.packet), among<false>(h.tab));
}

// ---- k_vol_sched<M, InLds, Pk, Tab>: f(machine, InLds, Pk, Tab); mh_volwave.hip's VsMachines are the types
enum Machine {
    kVolMachineHg, kVolMachine, kVolMachineBlend, kPvMachine, kPvMachineBlend,
    kPvBwdMachine, kPvBwdMachineBlend, kPvBwdMachineEm, kPvBwdMachineEmBlend
};
struct VolSched {
    Machine machine;
    Home home;
};
inline VolSched vol_sched(const Facts &f, uint32_t type) {
    const bool pv = type == MH_INTEGRATOR_PRBVOLPATH;
    return {pv ? (blend(f) ? kPvMachineBlend : kPvMachine)
               : blend(f) ? kVolMachineBlend : (f.vol_flags & kVolPhaseExt) ? kVolMachine : kVolMachineHg,
            home(f, !f.vs_notab)};
}
inline VolSched vol_sched_bwd(const Facts &f, bool emitter) {
    return {emitter ? (blend(f) ? kPvBwdMachineEmBlend : kPvBwdMachineEm)
                    : (blend(f) ? kPvBwdMachineBlend : kPvBwdMachine),
            home(f, !f.vs_notab)};
}
template <class F>
bool dispatch(const VolSched &k, F &&f) {
    return select_home(k.home, f, among<kVolMachineHg, kVolMachine, kVolMachineBlend, kPvMachine, kPvMachineBlend,
                                        kPvBwdMachine, kPvBwdMachineBlend, kPvBwdMachineEm, kPvBwdMachineEmBlend>(k.machine));
}

// ---- k_vw_main<Fresh, InLds, Pk, Ph>, k_vw_finish<InLds, Pk, Ph>, k_vw_walk<InLds, Pk>; the per-lane
// ---- k_prbvol_backward<InLds, Ph>, k_pvb_replay_paths<InLds, Ph>, k_pvb_replay_walks<InLds>:
// ---- f(Fresh, Ph, InLds, Pk, Tab = false) -----------------------------------------------------
struct VolKernel {
    bool fresh;  // the first round: the paths start at the camera
    int ph;
    Home home;
};
inline VolKernel volwave(const Facts &f, bool first_round) { return {first_round, phase_level(f), home(f, false)}; }
inline VolKernel vol_lane(const Facts &f) { return {false, phase_level(f), {f.bvh_lds, false, false}}; }
template <class F>
bool dispatch(const VolKernel &k, F &&f) {
    return select_home(k.home, f, flag(k.fresh), among<kPhExt, kPhBlend>(k.ph));
}

// ---- the last argument of k_prbvol_backward<InLds, Ph, PhG> and k_render_forward<true, InLds, Ph, PhG>:
// ---- f(PhG), nested in the selections above and below.  PhG: the call lists an `hg` medium's asymmetry g
// (GradArgs::n_phase_g != 0) and gets the instances with its two adjoint terms; a call without one launches
// the kernels it launched before.  (The scheduler machines have no such instance: plan_backward turns `sched`
// off for such a call, mh_plan.hpp.)
template <class F>
bool phase_g(bool key_listed, F &&f) { return select(f, flag(key_listed)); }

// ---- k_render<Kind, InLds, Ph>: f(Kind, InLds, Ph).  Kind: mh_integrator::type (what is none of
// the others renders as `path`); kPhBlend: a volumetric integrator on a scene with a blend medium
template <class F>
bool render(const Facts &facts, uint32_t type, F &&f) {
    const auto lds = flag(facts.bvh_lds);
    if (type == MH_INTEGRATOR_VOLPATH || type == MH_INTEGRATOR_PRBVOLPATH)
        return select(f, among<(int)MH_INTEGRATOR_VOLPATH, (int)MH_INTEGRATOR_PRBVOLPATH>((int)type), lds,
                      among<kPhExt, kPhBlend>(phase_level(facts)));
    const int kind = type == MH_INTEGRATOR_PRB ? (int)MH_INTEGRATOR_PRB : (int)MH_INTEGRATOR_PATH;
    return select(f, among<(int)MH_INTEGRATOR_PATH, (int)MH_INTEGRATOR_PRB>(kind), lds, among<kPhExt>(kPhExt));
}
// ---- k_render_forward<Vol, InLds, Ph>: f(Vol, InLds, Ph).  Vol: prbvolpath, else prb
template <class F>
bool render_forward(const Facts &facts, uint32_t type, F &&f) {
    if (type == MH_INTEGRATOR_PRBVOLPATH)
        return select(f, among<true>(true), flag(facts.bvh_lds), among<kPhExt, kPhBlend>(phase_level(facts)));
    return select(f, among<false>(false), flag(facts.bvh_lds), among<kPhExt>(kPhExt));
}

// ---- k_develop<Fmt, Alpha>: f(Fmt, Alpha) ------------------------------------------------------
template <class F>
bool develop(uint32_t fmt, F &&f) {
    const int base = fmt == MH_PIXEL_Y || fmt == MH_PIXEL_YA       ? (int)MH_PIXEL_Y
                     : fmt == MH_PIXEL_XYZ || fmt == MH_PIXEL_XYZA ? (int)MH_PIXEL_XYZ : (int)MH_PIXEL_RGB;
    return select(f, among<(int)MH_PIXEL_Y, (int)MH_PIXEL_XYZ, (int)MH_PIXEL_RGB>(base),
                  flag(fmt == MH_PIXEL_RGBA || fmt == MH_PIXEL_YA || fmt == MH_PIXEL_XYZA));
}

// ---- the wavefront's trace kernels: k_wf_trace / k_wf_shadow<InLds, Packet, Eng>,
// ---- k_wf_shadow_prb<InLds, Packet, NR, Eng>: f(InLds, Packet, Eng, NR1) ------------------------
struct WfTrace {
    bool lds, packet;
    // the stream engine (an instance per node format, so each one's register allocation is that
    // of its own traversal engine); the packet and the LDS kernels are kEngBvh2's
    int eng;
    bool nr1;  // k_wf_shadow_prb: one rgb slot (NR = 1), else kMaxRgbParams
};
inline WfTrace wf_trace(const Facts &f, uint32_t n_rgb = 1) {
    const bool packet = wf_packet(f);
    return {f.bvh_lds, packet, f.bvh_lds || packet ? kEngBvh2 : f.stream_eng, n_rgb == 1};
}
template <class F>
bool dispatch(const WfTrace &k, F &&f) {
    if (k.lds || k.packet) return select(f, flag(k.lds), flag(k.packet), among<kEngBvh2>(k.eng), flag(k.nr1));
    return select(f, among<false>(k.lds), among<false>(k.packet),
                  among<kEngBvh2, kEngWide, kEngQuant, kEngWideC>(k.eng), flag(k.nr1));
}

// ---- k_wf_bounce<Gen, Two>: f(Gen, Two).  Gen: the launch generates the camera rays; Two: it also
// runs the bounce after the camera bounce, a survivor's state parked in the wave's LDS slab in between.
// The slab (kParkBytes per workgroup of four waves, 16 dwords per lane) lies behind the kernel's other
// dynamic LDS, and the two together stay within kFuse01MaxLds: five workgroups on a CU's 160 KB, the
// occupancy the bounce kernels' register budget targets.
#ifndef MH_WF_FUSE01
#define MH_WF_FUSE01 1  // 0: every bounce is a launch of its own (A/B builds)
#endif
constexpr uint32_t kParkDwords = 16, kParkBytes = 4u * 64u * kParkDwords * 4u, kFuse01MaxLds = 32768;
struct BouncePath {
    bool two;           // the first launch runs bounces 0 and 1
    uint32_t next;      // the bounce the host loop goes on with; its queue is in
    uint32_t next_buf;  // this ping-pong buffer, its length in counter block `next`
};
inline BouncePath bounce_path(const Facts &f, uint32_t max_depth, uint32_t fused_lds_bytes) {
    const bool two = MH_WF_FUSE01 && wf_fused(f) && max_depth >= 2 && fused_lds_bytes + kParkBytes <= kFuse01MaxLds;
    // bounce b reads buffer b & 1 and counter block b, and writes buffer (b + 1) & 1 and block b + 1
    return two ? BouncePath{true, 2, 0} : BouncePath{false, 1, 1};
}
template <class F>
bool bounce(bool first, bool two, F &&f) {
    if (first && two) return select(f, among<true>(true), among<true>(true));
    return select(f, flag(first), among<false>(false));
}

// ---- k_wf_bounce_prb<NR, Gen, Bm, Det, Em>: f(NR1, Gen, Bm, Det, Em).  NR1: at most one rgb slot
// (NR = 1), else kMaxRgbParams; Gen: the first bounce generates the camera rays; then the bitmap
// log, the deterministic workspace and the emitter slots present
template <class F>
bool bounce_prb(bool first, uint32_t n_rgb, bool bitmap_log, bool det_ws, bool emitter, F &&f) {
    return select(f, flag(n_rgb <= 1), flag(first), flag(bitmap_log), flag(det_ws), flag(emitter));
}
// ---- k_wf_shade_prb<Staged, NR, Em>: f(Staged, NR1, Em).  NR1: exactly one rgb slot
template <class F>
bool shade_prb(const Facts &facts, uint32_t n_rgb, bool emitter, F &&f) {
    return select(f, flag(facts.tables), flag(n_rgb == 1), flag(emitter));
}

// ---- k_wf_bitmap_scatter<InLds, Fx>: f(InLds, Fx).  InLds: per-workgroup LDS accumulation (float
// gradients only); Fx: deterministic, 1 the max pass, 2 the int64 pass; else 0
template <class F>
bool bitmap_scatter(bool deterministic, int fx_pass, bool fits_lds, F &&f) {
    if (deterministic) return select(f, among<false>(false), among<1, 2>(fx_pass));
    return select(f, flag(fits_lds), among<0>(0));
}

}  // namespace variant
}  // namespace mh
