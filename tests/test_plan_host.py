"""The host-only execution planner (csrc/mh_plan.hpp) and the environment
table (csrc/mh_env.hpp), checked without a GPU: tools/plan_check.cpp is
plain C++17 built with the host compiler; it prints the planners' decisions
for fixed calls, and the expected values below are literals worked out from
the rules as mh_api.hip spelled them before the planner existed.  The source
shape (one file reads the environment, the table and INTEGRATION.md list the
same variables) is asserted by reading the files."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mitsuba3-nasa_amd", "csrc")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def _build(tmp, name, *flags):
    exe = str(tmp / name)
    subprocess.run([CXX, "-std=c++17", "-Wall", *flags, os.path.join(ROOT, "tools", "plan_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    return exe


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [json.loads(line) for line in r.stdout.splitlines()]
    cases = {row.pop("case"): row for row in rows}
    assert len(cases) == len(rows)
    return cases


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    assert CXX, "a host C++ compiler"
    return _run(_build(tmp_path_factory.mktemp("plan"), "plan_check", "-O1"))


def test_plan_check_under_sanitizers(tmp_path, cases):
    # a stand-alone host program: the sanitizers' runtimes are linked in
    exe = _build(tmp_path, "plan_check_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    assert _run(exe) == cases


def _sub(case, **want):
    got = {k: case[k] for k in want}
    assert got == want


WF_MAX, VW_MAX = 1 << 25, 1 << 23


def test_split_threshold(cases):
    # 32 x 32 x 512 = 2^19 samples fit one chunk: split into two halves for the two streams
    assert cases["split_32x32_512"] == dict(chunk_px=512, n_chunks=2, two=1)
    assert cases["split_32x32_256"] == dict(chunk_px=1024, n_chunks=1, two=0)
    assert cases["split_32x32_512_two_off"] == dict(chunk_px=1024, n_chunks=1, two=0)
    assert cases["split_1px"] == dict(chunk_px=1, n_chunks=1, two=0)      # 2^20 samples, one pixel
    assert cases["split_odd"] == dict(chunk_px=513, n_chunks=2, two=1)    # (1025 + 1) / 2


def test_chunk_limit(cases):
    # 512 x 512 @ 256 under the 2^25 limit: 2^25 / 256 pixels per chunk
    assert cases["split_512x512_256"] == dict(chunk_px=131072, n_chunks=2, two=1)
    assert cases["split_512x512_256_two_off"] == dict(chunk_px=131072, n_chunks=2, two=0)


def test_split_ragged_shapes(cases):
    # tests/ragged_cases.py at 1024 samples per chunk: chunk_px = 1024 // S, no whole number of waves
    assert cases["split_ragged_tiny"] == dict(chunk_px=7, n_chunks=1, two=0)        # 341 > 7 pixels
    assert cases["split_ragged_odd"] == dict(chunk_px=91, n_chunks=1, two=0)        # 204 > 91
    assert cases["split_ragged_over16"] == dict(chunk_px=60, n_chunks=3, two=1)     # 1024 // 17, 180 pixels
    assert cases["split_ragged_over32"] == dict(chunk_px=31, n_chunks=3, two=1)     # 1024 // 33, 66 pixels
    assert cases["split_ragged_chunks"] == dict(chunk_px=85, n_chunks=7, two=1)     # 1024 // 12, 540 pixels
    assert cases["split_ragged_chunks1s"] == dict(chunk_px=85, n_chunks=7, two=0)
    for name in ("slabs12_0_4", "slabs12_4_7", "slabs12_7_12"):                     # 256, 341, 204 > 135
        assert cases["split_ragged_" + name] == dict(chunk_px=135, n_chunks=1, two=0)
    assert cases["split_ragged_slab16_3_10"] == dict(chunk_px=91, n_chunks=1, two=0)  # 146 > 91


def test_render_two_streams(cases):
    split = dict(engine="wavefront", mode=2, chunk_px=512, n_chunks=2, two=1, err=0)
    whole = dict(engine="wavefront", mode=2, chunk_px=1024, n_chunks=1, two=0, err=0)
    _sub(cases["render_default"], determ=0, max_samples=WF_MAX, **split)
    _sub(cases["render_256"], **whole)
    _sub(cases["render_flag_deterministic"], determ=1, **whole)
    _sub(cases["render_env_deterministic"], determ=1, **whole)
    _sub(cases["render_env_deterministic_true"], determ=0, **split)  # only "1" counts
    _sub(cases["render_shared_device"], determ=0, **whole)
    _sub(cases["render_streams_1"], **whole)                         # only "1" keeps one stream
    _sub(cases["render_streams_0"], **split)
    _sub(cases["render_streams_2"], **split)


def test_render_wf_chunk(cases):
    # 16 x 16 @ 8: 1024 samples per chunk are 128 pixels
    _sub(cases["render_chunk_10"], max_samples=1024, chunk_px=128, n_chunks=2, two=1)
    _sub(cases["render_chunk_1024"], max_samples=1024, chunk_px=128, n_chunks=2, two=1)
    _sub(cases["render_chunk_huge"], max_samples=WF_MAX, chunk_px=256, n_chunks=1, two=0)


def test_render_engine(cases):
    mega = dict(engine="mega", mode=0, max_samples=1 << 25, chunk_px=1024, n_chunks=1, two=0)
    _sub(cases["render_mode_mega"], err=0, **mega)
    _sub(cases["render_flag_megakernel"], err=0, **mega)
    _sub(cases["render_mode_other"], engine="wavefront", mode=2, two=1)   # only "mega" counts
    _sub(cases["render_prb_flag_wavefront"], err=4, engine="mega")        # MH_ERR_UNSUPPORTED
    _sub(cases["render_depth_64"], err=0, engine="wavefront", mode=2)
    _sub(cases["render_depth_65"], err=0, **mega)
    # max_depth 0: no bounce kernel would run, and the first one writes the positions
    _sub(cases["render_depth_0"], err=0, **mega)
    _sub(cases["render_depth_0_flag_wavefront"], err=4, engine="mega")
    _sub(cases["render_depth_1"], err=0, engine="wavefront", mode=2)
    _sub(cases["render_passes_fused"], engine="wavefront", mode=2, chunk_px=512, n_chunks=2, two=1)
    _sub(cases["render_passes_unfused"], **mega)
    _sub(cases["render_unfused"], engine="wavefront", mode=1, two=1)


def test_render_volpath(cases):
    vol = dict(err=0, mode=3, max_samples=VW_MAX, chunk_px=1024, n_chunks=1, two=0)
    _sub(cases["render_volpath"], engine="vol_sched", **vol)
    _sub(cases["render_volpath_rounds"], engine="vol_rounds", **vol)
    _sub(cases["render_volpath_passes"], engine="mega", mode=0, max_samples=1 << 25)
    _sub(cases["render_volpath_rounds_passes"], engine="mega", mode=0, max_samples=1 << 25)


def test_backward_engine(cases):
    _sub(cases["bwd_rgb"], fused=1, bmp_wf=0, wavefront=1, replay=0, mega=0, max_samples=WF_MAX, chunk_px=256,
         n_chunks=1, two=0)
    _sub(cases["bwd_rgb_chunk_1024"], wavefront=1, max_samples=1024, chunk_px=128, n_chunks=2, two=1)
    _sub(cases["bwd_rgb_chunk_1024_one_stream"], wavefront=1, chunk_px=128, n_chunks=2, two=0)
    _sub(cases["bwd_rgb_mega"], fused=1, mega=1, wavefront=0, n_chunks=0)
    # prb at max_depth 0 still sees the emitter (prb.py:121-135): the per-lane
    # kernel, as above 64 -- the wavefront would launch no bounce kernel
    _sub(cases["bwd_depth_0"], fused=1, mega=0, wavefront=0, n_chunks=0)
    _sub(cases["bwd_depth_1"], fused=1, wavefront=1, n_chunks=1)
    _sub(cases["bwd_depth_64"], fused=1, wavefront=1, n_chunks=1)
    _sub(cases["bwd_depth_65"], fused=1, mega=0, wavefront=0, n_chunks=0)
    _sub(cases["bwd_bmp_depth_32"], fused=0, bmp_wf=1, wavefront=1)
    for name in ("bwd_bmp_depth_33", "bwd_bmp_mixed_channels", "bwd_bmp_unfused", "bwd_bmp_wf_off"):
        _sub(cases[name], fused=0, bmp_wf=0, wavefront=0, replay=0)  # the replay kernel, not forced
    _sub(cases["bwd_bmp_env_replay"], bmp_wf=0, wavefront=0, replay=1)
    _sub(cases["bwd_bmp_flag_replay"], bmp_wf=0, wavefront=0, replay=1)


def test_backward_deterministic_and_lds(cases):
    # det_replay: deterministic, not prbvolpath, not on the wavefront
    _sub(cases["bwd_det_rgb_wavefront"], det_replay=0, fx=0, fxr=0, det_grad=1, two=0)
    _sub(cases["bwd_det_rgb_replay"], det_replay=1, fx=0, fxr=1, det_grad=0)
    _sub(cases["bwd_det_bmp_replay"], det_replay=1, fx=0, fxr=1, lds_tex=1)  # (det_replay then drops the accumulator)
    _sub(cases["bwd_det_vol"], det_replay=0, fx=1, fxr=1)
    _sub(cases["bwd_envdet_rgb_replay"], det_replay=1, fxr=1)
    for name in ("bwd_nodet_rgb_wavefront", "bwd_nodet_rgb_replay", "bwd_nodet_bmp_replay", "bwd_nodet_vol"):
        _sub(cases[name], det_replay=0, fx=0, fxr=0, det_grad=0)
    # the replay kernel's LDS texel accumulator: one bitmap of at most 48 KiB
    _sub(cases["bwd_bmp_wf_off"], lds_tex=1, bmp_lds=1)
    _sub(cases["bwd_bmp_48k_plus_4"], lds_tex=0, bmp_lds=1)
    _sub(cases["bwd_bmp_wf_off_lds_off"], lds_tex=0, bmp_lds=0)
    _sub(cases["bwd_bmp_lds_off"], bmp_wf=1, lds_tex=0, bmp_lds=0)
    _sub(cases["bwd_bmp_mixed_channels"], lds_tex=0)  # two bitmaps


def test_backward_bitmap_record_cap(cases):
    cap = (8 << 30) // (48 * 31)
    assert cap == 5772805
    assert cases["bmp_record_cap"] == dict(depth_31=cap, depth_4096=1 << 16)
    _sub(cases["bwd_bmp_depth_32"], max_samples=cap)
    _sub(cases["bwd_bmp_lds_off"], max_samples=cap)


def test_backward_prbvolpath(cases):
    _sub(cases["bwd_pvp"], wavefront=0, pvp_log=1, main_cap=256, nee_cap=256, sched=1)
    _sub(cases["bwd_pvp_nee_log_off"], pvp_log=0, sched=0)
    _sub(cases["bwd_pvp_single_off"], pvp_log=1, main_cap=0, nee_cap=256, sched=0)
    _sub(cases["bwd_pvp_caps"], pvp_log=1, main_cap=1, nee_cap=7, sched=1)  # MH_PVP_MAIN_CAP=0 clamps to 1
    _sub(cases["bwd_pvp_sched_off"], pvp_log=1, main_cap=256, sched=0)
    _sub(cases["bwd_pvp_unsupported"], pvp_log=1, main_cap=256, sched=0)


def test_forward(cases):
    on, off = dict(wavefront=1, mode=2), dict(wavefront=0, mode=0)
    for name in ("fwd_prb", "fwd_prb_depth_1", "fwd_prb_depth_64"):
        _sub(cases[name], chunk_px=1024, **on)
    for name in ("fwd_prb_depth_0", "fwd_prb_depth_65", "fwd_prb_flag_megakernel", "fwd_prb_mode_mega", "fwd_pvp",
                 "fwd_prb_unfused"):
        _sub(cases[name], chunk_px=1024, **off)
    _sub(cases["fwd_chunked"], chunk_px=(1 << 25) // 8, **on)  # 4096^2 pixels at 8 spp


def test_accessors(cases):
    # presence-only variables count when empty or "0"; integers keep their clamps
    assert cases["accessors_set"] == dict(vw_debug=1, vs_notab=1, test_fail=0, bvh_leaf=31, stream_stack=4,
                                          comm_timeout_ms=1, wf_unfused=0, wf_chunk=0)
    assert cases["accessors_unset"] == dict(vw_debug=0, vs_notab=0, test_fail=0, bvh_leaf=8, stream_stack=20,
                                            comm_timeout_ms=1800000, wf_unfused=0, wf_chunk=0)


# ---- source shape -------------------------------------------------------------
# the MH_* variables csrc/ passed to getenv before the table existed
VARIABLES = {
    "MH_BVH4", "MH_BVH4Q", "MH_BVH_CT", "MH_BVH_LEAF", "MH_BVH_THREADS", "MH_COMM_TIMEOUT_S", "MH_DETERMINISTIC",
    "MH_GRID_CORNER", "MH_MODE", "MH_PACKET_MAX_PRIMS", "MH_PRB_BMP_WF", "MH_PRB_LDS_TEX", "MH_PRB_REPLAY",
    "MH_PRIMC", "MH_PVP_MAIN_CAP", "MH_PVP_NEE_CAP", "MH_PVP_NEE_LOG", "MH_PVP_SCHED", "MH_PVP_SINGLE",
    "MH_STREAM_STACK", "MH_TEST_COMM_SCALE", "MH_TEST_FAIL_AFTER_ISSUE", "MH_TRAVERSAL", "MH_VOL_MODE", "MH_VS_BPC",
    "MH_VS_NOTAB", "MH_VW_BPC", "MH_VW_DEBUG", "MH_VW_ROUNDS", "MH_WF_BPC", "MH_WF_CHUNK", "MH_WF_FUSED",
    "MH_WF_STREAMS",
}


def _read(*path):
    with open(os.path.join(*path), encoding="utf-8") as f:
        return f.read()


def _table_names():
    rows = re.findall(r'^\s*X\(\w+, "(MH_[A-Z0-9_]+)", \w+,', _read(CSRC, "mh_env.hpp"), re.M)
    assert len(rows) == len(set(rows))
    return set(rows)


def test_only_the_env_header_reads_the_environment():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".cpp", ".hpp", ".h")) and name != "mh_env.hpp":
            assert "getenv(" not in _read(CSRC, name), name
    assert "getenv(" in _read(CSRC, "mh_env.hpp")
    for name in ("mh_env.hpp", "mh_plan.hpp"):  # host only
        assert "hip_runtime" not in _read(CSRC, name), name


def test_table_is_the_set_of_variables():
    assert _table_names() == VARIABLES
    # ... and no MH_* string of the header stands outside the table
    assert set(re.findall(r'"(MH_[A-Z0-9_]+)"', _read(CSRC, "mh_env.hpp"))) == VARIABLES


def test_integration_md_lists_the_table():
    text = _read(ROOT, "INTEGRATION.md")
    m = re.search(r"^## (?:\d+\. )?Environment variables\n(.*?)(?=^## |\Z)", text, re.M | re.S)
    assert m, "INTEGRATION.md: section 'Environment variables'"
    listed = re.findall(r"^\| `(MH_[A-Z0-9_]+)` \|", m.group(1), re.M)
    assert len(listed) == len(set(listed))
    assert set(listed) == _table_names()
