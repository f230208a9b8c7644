// plan_check — the host-only planners (csrc/mh_plan.hpp) and the environment
// table (csrc/mh_env.hpp) on fixed cases, one JSON line per case.  Plain
// C++17, no HIP: c++ -std=c++17 tools/plan_check.cpp -o plan_check.
// tests/test_plan_host.py holds the expected values.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <utility>

#include "../mitsuba3-nasa_amd/csrc/mh_env.hpp"
#include "../mitsuba3-nasa_amd/csrc/mh_plan.hpp"

using namespace mh;
using Env = std::initializer_list<std::pair<const char *, const char *>>;

// the process environment holds exactly `vars` of the table's variables
static void set_env(Env vars) {
    for (const env::Var &v : env::kVars) unsetenv(v.name);
    for (const auto &kv : vars) setenv(kv.first, kv.second, 1);
}

static void put(const char *name, const plan::Split &c) {
    printf("{\"case\": \"%s\", \"chunk_px\": %u, \"n_chunks\": %llu, \"two\": %d}\n", name, c.chunk_px,
           (unsigned long long)c.n_chunks, (int)c.two);
}
static void put(const char *name, const plan::RenderPlan &p) {
    const char *engine = p.wavefront ? "wavefront" : p.sched ? "vol_sched" : p.volwave ? "vol_rounds" : "mega";
    printf("{\"case\": \"%s\", \"err\": %d, \"engine\": \"%s\", \"mode\": %u, \"determ\": %d, \"max_samples\": %llu, "
           "\"chunk_px\": %u, \"n_chunks\": %llu, \"two\": %d}\n",
           name, p.err, engine, p.mode, (int)p.determ, (unsigned long long)p.max_samples,
           p.chunks.chunk_px, (unsigned long long)p.chunks.n_chunks, (int)p.chunks.two);
}
static void put(const char *name, const plan::BackwardPlan &p) {
    printf("{\"case\": \"%s\", \"replay\": %d, \"mega\": %d, \"fused\": %d, \"bmp_wf\": %d, \"wavefront\": %d, "
           "\"fx\": %d, \"det_replay\": %d, \"fxr\": %d, \"det_grad\": %d, \"lds_tex\": %d, \"bmp_lds\": %d, "
           "\"max_samples\": %llu, \"chunk_px\": %u, \"n_chunks\": %llu, \"two\": %d, \"pvp_log\": %d, "
           "\"main_cap\": %u, \"nee_cap\": %u, \"sched\": %d}\n",
           name, (int)p.replay, (int)p.mega, (int)p.fused, (int)p.bmp_wf, (int)p.wavefront, (int)p.fx,
           (int)p.det_replay, (int)p.fxr, (int)p.det_grad, (int)p.lds_tex, (int)p.bmp_lds,
           (unsigned long long)p.max_samples, p.chunks.chunk_px, (unsigned long long)p.chunks.n_chunks,
           (int)p.chunks.two, (int)p.pvp_log, p.main_cap, p.nee_cap, (int)p.sched);
}
static void put(const char *name, const plan::ForwardPlan &p) {
    printf("{\"case\": \"%s\", \"wavefront\": %d, \"mode\": %u, \"chunk_px\": %u}\n", name, (int)p.wavefront, p.mode,
           p.chunk_px);
}

constexpr uint64_t kWfMax = 1ull << 25, kVwMax = 1ull << 23;  // wf_max_chunk(), vw_max_chunk()

// a Cornell-box-like call: fused packet-engine scene, w x h pixels at spp
static plan::Facts facts(uint32_t type, uint32_t depth, uint32_t w, uint32_t h, uint32_t spp, uint32_t flags = 0) {
    plan::Facts f;
    f.type = type;
    f.max_depth = depth;
    f.flags = flags;
    f.n_px = (uint64_t)w * h;
    f.spp = spp;
    f.wf_fused = true;
    f.vs_ok = f.vw_ok = type == MH_INTEGRATOR_VOLPATH;
    if (type == MH_INTEGRATOR_PRBVOLPATH) f.vs_ok = true;
    f.wf_max = kWfMax;
    f.vw_max = kVwMax;
    return f;
}
static void render(const char *name, plan::Facts f, Env vars = {}) {
    set_env(vars);
    f.vol_sched = !env::vol_mode_rounds();
    put(name, plan::plan_render(f, env::plan_env(env::Call::Render)));
}
static void backward(const char *name, const plan::Facts &f, Env vars = {}) {
    set_env(vars);
    put(name, plan::plan_backward(f, env::plan_env(f.type == MH_INTEGRATOR_PRBVOLPATH ? env::Call::BackwardVol : env::Call::Backward)));
}
static void forward(const char *name, const plan::Facts &f, Env vars = {}) {
    set_env(vars);
    put(name, plan::plan_forward(f, env::plan_env(env::Call::Forward)));
}

int main() {
    const uint32_t PATH = MH_INTEGRATOR_PATH, VOLPATH = MH_INTEGRATOR_VOLPATH, PRB = MH_INTEGRATOR_PRB,
                   PVP = MH_INTEGRATOR_PRBVOLPATH;
    // ---- split_chunks ----
    put("split_32x32_512", plan::split_chunks(32 * 32, 512, kWfMax, true));
    put("split_32x32_256", plan::split_chunks(32 * 32, 256, kWfMax, true));
    put("split_32x32_512_two_off", plan::split_chunks(32 * 32, 512, kWfMax, false));
    put("split_1px", plan::split_chunks(1, 1ull << 20, kWfMax, true));
    put("split_odd", plan::split_chunks(1025, 512, kWfMax, true));
    put("split_512x512_256", plan::split_chunks(512 * 512, 256, kWfMax, true));
    put("split_512x512_256_two_off", plan::split_chunks(512 * 512, 256, kWfMax, false));
    // the launch shapes of tests/ragged_cases.py (W x H pixels, S samples per pixel) at 1024 samples per chunk
    put("split_ragged_tiny", plan::split_chunks(7 * 1, 3, 1024, true));
    put("split_ragged_odd", plan::split_chunks(13 * 7, 5, 1024, true));
    put("split_ragged_over16", plan::split_chunks(20 * 9, 17, 1024, true));
    put("split_ragged_over32", plan::split_chunks(11 * 6, 33, 1024, true));
    put("split_ragged_chunks", plan::split_chunks(27 * 20, 12, 1024, true));
    put("split_ragged_chunks1s", plan::split_chunks(27 * 20, 12, 1024, false));
    put("split_ragged_slabs12_0_4", plan::split_chunks(27 * 5, 4, 1024, true));
    put("split_ragged_slabs12_4_7", plan::split_chunks(27 * 5, 3, 1024, true));
    put("split_ragged_slabs12_7_12", plan::split_chunks(27 * 5, 5, 1024, true));
    put("split_ragged_slab16_3_10", plan::split_chunks(13 * 7, 7, 1024, true));

    // ---- plan_render ----
    const plan::Facts big = facts(PATH, 8, 32, 32, 512), tiny = facts(PATH, 8, 16, 16, 8);
    render("render_default", big);
    render("render_256", facts(PATH, 8, 32, 32, 256));
    render("render_flag_deterministic", facts(PATH, 8, 32, 32, 512, MH_FLAG_DETERMINISTIC));
    render("render_env_deterministic", big, {{"MH_DETERMINISTIC", "1"}});
    render("render_env_deterministic_true", big, {{"MH_DETERMINISTIC", "true"}});
    render("render_shared_device", facts(PATH, 8, 32, 32, 512, MH_FLAG_SHARED_DEVICE));
    render("render_streams_1", big, {{"MH_WF_STREAMS", "1"}});
    render("render_streams_0", big, {{"MH_WF_STREAMS", "0"}});
    render("render_streams_2", big, {{"MH_WF_STREAMS", "2"}});
    render("render_chunk_10", tiny, {{"MH_WF_CHUNK", "10"}});
    render("render_chunk_1024", tiny, {{"MH_WF_CHUNK", "1024"}});
    render("render_chunk_huge", tiny, {{"MH_WF_CHUNK", "1099511627776"}});
    render("render_mode_mega", big, {{"MH_MODE", "mega"}});
    render("render_mode_other", big, {{"MH_MODE", "megakernel"}});
    render("render_flag_megakernel", facts(PATH, 8, 32, 32, 512, MH_FLAG_MEGAKERNEL));
    render("render_prb_flag_wavefront", facts(PRB, 8, 32, 32, 512, MH_FLAG_WAVEFRONT));
    render("render_depth_0", facts(PATH, 0, 32, 32, 512));
    render("render_depth_0_flag_wavefront", facts(PATH, 0, 32, 32, 512, MH_FLAG_WAVEFRONT));
    render("render_depth_1", facts(PATH, 1, 32, 32, 512));
    render("render_depth_64", facts(PATH, 64, 32, 32, 512));
    render("render_depth_65", facts(PATH, 65, 32, 32, 512));
    {
        plan::Facts f = big;
        f.n_passes = 2;
        render("render_passes_fused", f);
        f.wf_fused = false;
        render("render_passes_unfused", f);
        f.n_passes = 1;
        render("render_unfused", f);
    }
    const plan::Facts volp = facts(VOLPATH, 8, 32, 32, 512);
    render("render_volpath", volp);
    render("render_volpath_rounds", volp, {{"MH_VOL_MODE", "rounds"}});
    {
        plan::Facts f = volp;
        f.n_passes = 2;
        render("render_volpath_passes", f);
        render("render_volpath_rounds_passes", f, {{"MH_VOL_MODE", "rounds"}});
    }

    // ---- plan_backward ----
    plan::Facts rgb = facts(PRB, 8, 16, 16, 8), bmp = facts(PRB, 32, 16, 16, 8);
    rgb.n_rgb = 1;
    bmp.n_bmp = 1;
    bmp.bmp_slot_bytes = 48u << 10;
    backward("bwd_rgb", rgb);
    backward("bwd_rgb_chunk_1024", rgb, {{"MH_WF_CHUNK", "1024"}});
    backward("bwd_rgb_chunk_1024_one_stream", rgb, {{"MH_WF_CHUNK", "1024"}, {"MH_WF_STREAMS", "1"}});
    backward("bwd_rgb_mega", rgb, {{"MH_MODE", "mega"}});
    for (uint32_t depth : {0u, 1u, 64u, 65u}) {
        plan::Facts f = rgb;
        f.max_depth = depth;
        backward(("bwd_depth_" + std::to_string(depth)).c_str(), f);
    }
    backward("bwd_bmp_depth_32", bmp);
    {
        plan::Facts f = bmp;
        f.max_depth = 33;
        backward("bwd_bmp_depth_33", f);
        f = bmp;
        f.n_bmp = 2;
        f.bmp_same_ch = false;
        backward("bwd_bmp_mixed_channels", f);
        f = bmp;
        f.wf_fused = false;
        backward("bwd_bmp_unfused", f);
        f = bmp;
        f.flags = MH_FLAG_PRB_REPLAY;
        backward("bwd_bmp_flag_replay", f);
        f = bmp;
        f.bmp_slot_bytes += 4;
        backward("bwd_bmp_48k_plus_4", f, {{"MH_PRB_BMP_WF", "0"}});
    }
    backward("bwd_bmp_wf_off", bmp, {{"MH_PRB_BMP_WF", "0"}});
    backward("bwd_bmp_env_replay", bmp, {{"MH_PRB_REPLAY", "1"}});
    backward("bwd_bmp_lds_off", bmp, {{"MH_PRB_LDS_TEX", "0"}});
    backward("bwd_bmp_wf_off_lds_off", bmp, {{"MH_PRB_BMP_WF", "0"}, {"MH_PRB_LDS_TEX", "0"}});
    // deterministic: det_replay exactly when deterministic, not vol, not wavefront
    for (int det = 0; det < 2; ++det) {
        const uint32_t d = det ? (uint32_t)MH_FLAG_DETERMINISTIC : 0u;
        plan::Facts f = rgb;
        f.flags = d;
        backward(det ? "bwd_det_rgb_wavefront" : "bwd_nodet_rgb_wavefront", f);
        f.flags = d | MH_FLAG_PRB_REPLAY;
        backward(det ? "bwd_det_rgb_replay" : "bwd_nodet_rgb_replay", f);
        f = bmp;
        f.flags = d;
        backward(det ? "bwd_det_bmp_replay" : "bwd_nodet_bmp_replay", f, {{"MH_PRB_BMP_WF", "0"}});
        f = facts(PVP, 8, 16, 16, 8, d);
        backward(det ? "bwd_det_vol" : "bwd_nodet_vol", f);
    }
    backward("bwd_envdet_rgb_replay", rgb, {{"MH_DETERMINISTIC", "1"}, {"MH_PRB_REPLAY", "1"}});
    printf("{\"case\": \"bmp_record_cap\", \"depth_31\": %llu, \"depth_4096\": %llu}\n",
           (unsigned long long)plan::bmp_record_cap(31), (unsigned long long)plan::bmp_record_cap(4096));
    // the phase tables' LDS residency: a 28,848-byte table (1,801 nodes + 2 records) beside other LDS
    printf("{\"case\": \"phase_lds\", \"fits_exactly\": %u, \"one_over\": %u, \"no_table\": %u, \"alone\": %u, "
           "\"alone_over\": %u, \"huge_other\": %u}\n",
           plan::phase_lds_bytes(28848, 65536 - 28848), plan::phase_lds_bytes(28848, 65536 - 28848 + 1),
           plan::phase_lds_bytes(0, 1024), plan::phase_lds_bytes(65536, 0), plan::phase_lds_bytes(65552, 0),
           plan::phase_lds_bytes(16, ~0ull - 8));
    // prbvolpath
    const plan::Facts pvp = facts(PVP, 8, 16, 16, 8);
    backward("bwd_pvp", pvp);
    backward("bwd_pvp_nee_log_off", pvp, {{"MH_PVP_NEE_LOG", "0"}});
    backward("bwd_pvp_single_off", pvp, {{"MH_PVP_SINGLE", "0"}, {"MH_PVP_MAIN_CAP", "9"}});
    backward("bwd_pvp_caps", pvp, {{"MH_PVP_MAIN_CAP", "0"}, {"MH_PVP_NEE_CAP", "7"}});
    backward("bwd_pvp_sched_off", pvp, {{"MH_PVP_SCHED", "0"}});
    {
        plan::Facts f = pvp;
        f.vs_ok = false;
        backward("bwd_pvp_unsupported", f);
    }

    // ---- plan_forward ----
    forward("fwd_prb", facts(PRB, 8, 32, 32, 8));
    forward("fwd_prb_depth_0", facts(PRB, 0, 32, 32, 8));
    forward("fwd_prb_depth_1", facts(PRB, 1, 32, 32, 8));
    forward("fwd_prb_depth_64", facts(PRB, 64, 32, 32, 8));
    forward("fwd_prb_depth_65", facts(PRB, 65, 32, 32, 8));
    forward("fwd_prb_flag_megakernel", facts(PRB, 8, 32, 32, 8, MH_FLAG_MEGAKERNEL));
    forward("fwd_prb_mode_mega", facts(PRB, 8, 32, 32, 8), {{"MH_MODE", "mega"}});
    forward("fwd_pvp", facts(PVP, 8, 32, 32, 8));
    {
        plan::Facts f = facts(PRB, 8, 32, 32, 8);
        f.wf_fused = false;
        forward("fwd_prb_unfused", f);
    }
    forward("fwd_chunked", facts(PRB, 8, 4096, 4096, 8));

    // ---- accessors: presence-only variables, clamps ----
    set_env({{"MH_VW_DEBUG", ""}, {"MH_VS_NOTAB", "0"}, {"MH_BVH_LEAF", "99"}, {"MH_STREAM_STACK", "1"},
             {"MH_COMM_TIMEOUT_S", "0"}, {"MH_WF_FUSED", "1"}});
    printf("{\"case\": \"accessors_set\", \"vw_debug\": %d, \"vs_notab\": %d, \"test_fail\": %d, \"bvh_leaf\": %d, "
           "\"stream_stack\": %d, \"comm_timeout_ms\": %d, \"wf_unfused\": %d, \"wf_chunk\": %llu}\n",
           (int)env::vw_debug(), (int)env::vs_notab(), (int)env::test_fail_after_issue(), env::bvh_leaf(8),
           env::stream_stack(20), (int)(env::comm_timeout_s(1800.0) * 1000.0 + 0.5), (int)env::wf_unfused(),
           (unsigned long long)env::wf_chunk());
    set_env({});
    printf("{\"case\": \"accessors_unset\", \"vw_debug\": %d, \"vs_notab\": %d, \"test_fail\": %d, \"bvh_leaf\": %d, "
           "\"stream_stack\": %d, \"comm_timeout_ms\": %d, \"wf_unfused\": %d, \"wf_chunk\": %llu}\n",
           (int)env::vw_debug(), (int)env::vs_notab(), (int)env::test_fail_after_issue(), env::bvh_leaf(8),
           env::stream_stack(20), (int)(env::comm_timeout_s(1800.0) * 1000.0 + 0.5), (int)env::wf_unfused(),
           (unsigned long long)env::wf_chunk());
    return 0;
}
