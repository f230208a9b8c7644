// phase_g_check — the HG asymmetry's derivative (csrc/mh_phase_grad.hpp) and
// the planner's answer to a '<medium>.phase_function.g' key (csrc/mh_plan.hpp),
// checked on the host, one JSON line per case.  Plain C++17, no HIP:
//   c++ -std=c++17 -ffp-contract=off tools/phase_g_check.cpp -o phase_g_check
// tests/test_phase_g_host.py reads the lines.
//
// 1. hg_dlog_dg in float against a double-precision central difference of
//    ln eval_hg (hg.cpp:66-72), per g over 257 cosines including +-1.  The bound
//    is the float evaluation's own rounding, first order, doubled:
//      A = -2g / (1 - g^2):      |A| u (3 + g^2 / (1 - g^2))
//      temp = (1 + g^2) + 2g c:  u (g^2 + (1 + g^2) + 2 |g c| + temp) =: dt  (it cancels near g c = -1)
//      B = 3 (g + c) / temp:     |B| (3 u + dt / temp)
//      A - B:                    u |A - B|
//    with u = 2^-24, plus 1e-9 (1 + |value|) for the difference quotient itself
//    (step 1e-5: truncation h^2 f''' / 6 <= 1e-10 * 8000 / 6 at |g| = 0.95).
// 2. plan_backward with and without a phase key, over every combination of the
//    environment switches and the facts a prbvolpath or prb call can have: a
//    call without the key must get, field by field, the plan of the planner as
//    it was before the key existed (restated below); a call with it differs
//    in `sched` only, which is off.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../mitsuba3-nasa_amd/csrc/mh_phase_grad.hpp"
#include "../mitsuba3-nasa_amd/csrc/mh_plan.hpp"

using namespace mh;

static double ln_hg(double g, double c) {
    const double temp = 1.0 + g * g + 2.0 * g * c;
    return std::log((1.0 - g * g) / (4.0 * M_PI * temp * std::sqrt(temp)));
}

static int check_derivative() {
    const float gs[] = {-0.95f, -0.7f, -0.3f, 0.f, 1e-4f, 0.5f, 0.85f, 0.95f};
    const double u = std::ldexp(1.0, -24), h = 1e-5;
    int bad = 0;
    for (float gf : gs) {
        double worst = 0.0, worst_err = 0.0, worst_bound = 0.0, max_abs = 0.0;
        for (int i = 0; i <= 256; ++i) {
            const float cf = (float)(-1.0 + (double)i / 128.0);  // -1, ..., 0, ..., 1: exact in float
            const double g = gf, c = cf;
            const double fd = (ln_hg(g + h, c) - ln_hg(g - h, c)) / (2.0 * h);
            const double got = hg_dlog_dg(gf, cf);
            const double temp = 1.0 + g * g + 2.0 * g * c;
            const double A = -2.0 * g / (1.0 - g * g), B = 3.0 * (g + c) / temp;
            const double dt = u * (g * g + (1.0 + g * g) + 2.0 * std::fabs(g * c) + temp);
            const double bound = 2.0 * (std::fabs(A) * u * (3.0 + g * g / (1.0 - g * g)) +
                                        std::fabs(B) * (3.0 * u + dt / temp) + u * std::fabs(A - B)) +
                                 1e-9 * (1.0 + std::fabs(fd));
            const double err = std::fabs(got - fd);
            if (!(err <= bound)) ++bad;
            if (err / bound > worst) { worst = err / bound; worst_err = err; worst_bound = bound; }
            max_abs = std::fmax(max_abs, std::fabs(fd));
        }
        printf("{\"case\": \"dlog_dg\", \"g\": %.9g, \"n\": 257, \"worst_ratio\": %.6g, \"err\": %.6g, \"bound\": %.6g, "
               "\"max_abs\": %.9g}\n", (double)gf, worst, worst_err, worst_bound, max_abs);
    }
    // g = 0: -3 cos(theta) exactly, and no division by g anywhere
    const bool zero_ok = hg_dlog_dg(0.f, 1.f) == -3.f && hg_dlog_dg(0.f, -1.f) == 3.f && hg_dlog_dg(0.f, 0.f) == 0.f &&
                         hg_dlog_dg(0.f, 0.25f) == -0.75f;
    printf("{\"case\": \"dlog_dg_zero\", \"ok\": %d}\n", (int)zero_ok);
    return bad + (zero_ok ? 0 : 1);
}

// plan_backward as it was before Facts::n_phase_params existed
static plan::BackwardPlan plan_backward_before(const plan::Facts &f, const plan::PlanEnv &e) {
    using namespace plan;
    BackwardPlan p;
    const bool vol = f.type == MH_INTEGRATOR_PRBVOLPATH;
    p.determ = deterministic(f.flags, e.deterministic);
    p.fx = vol && p.determ;
    p.replay = (f.flags & MH_FLAG_PRB_REPLAY) || e.prb_replay;
    p.mega = megakernel(f.flags, e);
    p.fused = !vol && f.n_bmp == 0 && !p.replay;
    p.bmp_wf = !vol && f.n_bmp >= 1 && f.bmp_same_ch && !p.replay && !p.mega && f.wf_fused && f.max_depth >= 1 &&
               f.max_depth <= 32 && !e.prb_bmp_wf_off;
    p.wavefront = (p.fused && f.max_depth >= 1 && f.max_depth <= 64 && !p.mega) || p.bmp_wf;
    p.det_replay = p.determ && !vol && !p.wavefront;
    p.fxr = p.fx || p.det_replay;
    p.lds_tex = f.n_bmp == 1 && f.bmp_slot_bytes <= (48u << 10) && !e.prb_lds_tex_off;
    p.bmp_lds = !e.prb_lds_tex_off;
    if (p.wavefront) {
        p.max_samples = wf_chunk_samples(e, f.wf_max);
        p.n_depth = std::max<uint32_t>(1, f.max_depth - 1);
        if (p.bmp_wf) p.max_samples = std::min<uint64_t>(p.max_samples, bmp_record_cap(p.n_depth));
        p.chunks = split_chunks(f.n_px, f.spp, p.max_samples, two_streams_ok(f.flags, e));
        p.det_grad = p.determ && f.n_rgb > 0;
    } else if (vol && !e.pvp_nee_log_off) {
        p.pvp_log = true;
        p.main_cap = e.pvp_single_off ? 0u : e.pvp_main_cap ? e.pvp_main_cap : kPvpMainCap;
        p.nee_cap = e.pvp_nee_cap ? e.pvp_nee_cap : kPvpNeeCap;
        p.sched = p.main_cap && f.vs_ok && !e.pvp_sched_off;
    }
    return p;
}

// every field of a BackwardPlan; skip_sched leaves `sched` out
static bool same(const plan::BackwardPlan &a, const plan::BackwardPlan &b, bool skip_sched) {
    return a.replay == b.replay && a.mega == b.mega && a.fused == b.fused && a.bmp_wf == b.bmp_wf &&
           a.wavefront == b.wavefront && a.determ == b.determ && a.fx == b.fx && a.det_replay == b.det_replay &&
           a.fxr == b.fxr && a.det_grad == b.det_grad && a.lds_tex == b.lds_tex && a.bmp_lds == b.bmp_lds &&
           a.n_depth == b.n_depth && a.max_samples == b.max_samples && a.chunks.chunk_px == b.chunks.chunk_px &&
           a.chunks.n_chunks == b.chunks.n_chunks && a.chunks.two == b.chunks.two && a.pvp_log == b.pvp_log &&
           a.main_cap == b.main_cap && a.nee_cap == b.nee_cap && (skip_sched || a.sched == b.sched);
}
// a field added to BackwardPlan must be added to same() (x86-64: 12 bools, n_depth, max_samples, the 24-byte
// Split, pvp_log, the two caps and sched fill 64 bytes)
static_assert(sizeof(void *) != 8 || sizeof(plan::BackwardPlan) == 64, "same() lists every field of BackwardPlan");

static int check_plan() {
    unsigned long long n_plans = 0, n_sched_without = 0, n_sched_with = 0, n_diff_without = 0, n_diff_with = 0;
    const uint32_t flag_sets[] = {0u, MH_FLAG_DETERMINISTIC, MH_FLAG_PRB_REPLAY, MH_FLAG_MEGAKERNEL, MH_FLAG_SHARED_DEVICE};
    for (uint32_t type : {(uint32_t)MH_INTEGRATOR_PRBVOLPATH, (uint32_t)MH_INTEGRATOR_PRB})
    for (uint32_t flags : flag_sets)
    for (uint32_t depth : {0u, 1u, 8u, 33u, 65u})
    for (int vs_ok = 0; vs_ok < 2; ++vs_ok)
    for (uint32_t n_bmp : {0u, 1u})
    for (uint32_t envbits = 0; envbits < 512; ++envbits) {
        plan::Facts f;
        f.type = type;
        f.max_depth = depth;
        f.flags = flags;
        f.n_px = 1024;
        f.spp = 512;
        f.wf_fused = true;
        f.vs_ok = vs_ok;
        f.wf_max = 1ull << 25;
        f.vw_max = 1ull << 23;
        f.n_rgb = 2;
        f.n_bmp = n_bmp;
        f.bmp_slot_bytes = 4096;
        plan::PlanEnv e;
        e.deterministic = envbits & 1u;
        e.mode_mega = envbits & 2u;
        e.wf_one_stream = envbits & 4u;
        e.prb_replay = envbits & 8u;
        e.pvp_nee_log_off = envbits & 16u;
        e.pvp_single_off = envbits & 32u;
        e.pvp_sched_off = envbits & 64u;
        e.pvp_main_cap = (envbits & 128u) ? 2u : 0u;
        e.pvp_nee_cap = (envbits & 256u) ? 1u : 0u;
        const plan::BackwardPlan before = plan_backward_before(f, e);
        f.n_phase_params = 0;
        const plan::BackwardPlan without = plan::plan_backward(f, e);
        f.n_phase_params = 1;
        const plan::BackwardPlan with = plan::plan_backward(f, e);
        ++n_plans;
        n_sched_without += without.sched;
        n_sched_with += with.sched;
        n_diff_without += !same(without, before, false);
        n_diff_with += !same(with, before, true);
    }
    printf("{\"case\": \"plan_backward\", \"plans\": %llu, \"sched_without_key\": %llu, \"sched_with_key\": %llu, "
           "\"differ_without_key\": %llu, \"differ_with_key_beyond_sched\": %llu}\n",
           n_plans, n_sched_without, n_sched_with, n_diff_without, n_diff_with);
    // the default prbvolpath call: the scheduler without the key, the per-lane kernel with its logs with it
    plan::Facts f;
    f.type = MH_INTEGRATOR_PRBVOLPATH;
    f.max_depth = 8;
    f.n_px = 64;
    f.spp = 64;
    f.vs_ok = true;
    const plan::BackwardPlan a = plan::plan_backward(f, plan::PlanEnv{});
    f.n_phase_params = 1;
    const plan::BackwardPlan b = plan::plan_backward(f, plan::PlanEnv{});
    printf("{\"case\": \"plan_default\", \"sched_without_key\": %d, \"sched_with_key\": %d, \"pvp_log_with_key\": %d, "
           "\"main_cap_with_key\": %u, \"nee_cap_with_key\": %u}\n",
           (int)a.sched, (int)b.sched, (int)b.pvp_log, b.main_cap, b.nee_cap);
    return (n_diff_without || n_diff_with || n_sched_with || !n_sched_without) ? 1 : 0;
}

int main() {
    const int bad = check_derivative() + check_plan();
    printf("{\"case\": \"summary\", \"failures\": %d}\n", bad);
    return bad ? 1 : 0;
}
