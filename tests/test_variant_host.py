"""The host-only kernel-variant selectors (csrc/mh_variant.hpp), checked
without a GPU: tools/variant_check.cpp is plain C++17 built with the host
compiler; it prints, for the whole input space of every kernel family, the
selector's key (where the family has one) and the template arguments that the
selector hands to the launcher.  The expected arguments below are the launchers' if-chains as they
stood before the selectors existed, one function per ladder, transcribed from
that text (not from the header)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mitsuba3-nasa_amd", "csrc")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")

PATH, VOLPATH, PRB, PRBVOLPATH = 0, 1, 2, 3               # MH_INTEGRATOR_*
PIXEL_RGB, PIXEL_Y, PIXEL_XYZ, PIXEL_RGBA, PIXEL_YA, PIXEL_XYZA = range(6)
PH_EXT, PH_BLEND = 1, 2                                   # kPhExt, kPhBlend
ENG_BVH2, ENG_WIDE, ENG_QUANT, ENG_WIDEC = range(4)       # kEng*
VOL_PHASE_EXT, VOL_PHASE_BLEND = 4, 8                     # kVolPhaseExt, kVolPhaseBlend
PACKET_MAX_PRIMS = 64                                     # what variant_check sets


def _read(*path):
    with open(os.path.join(*path), encoding="utf-8") as f:
        return f.read()


def _enum(name):
    body = re.search(r"enum %s \{(.*?)\};" % name, _read(CSRC, "mh_variant.hpp"), re.S).group(1)
    return [w.strip() for w in body.split(",")]


def _build(tmp, name, *flags):
    exe = str(tmp / name)
    subprocess.run([CXX, "-std=c++17", "-Wall", *flags, os.path.join(ROOT, "tools", "variant_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    return exe


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    assert CXX, "a host C++ compiler"
    return _run(_build(tmp_path_factory.mktemp("variant"), "variant_check", "-O1"))


@pytest.fixture(scope="module")
def rows(output):
    """family -> [(inputs, key, handed)], each a tuple of ints"""
    out = {}
    for line in output.splitlines():
        family, *cols = [c.strip() for c in line.split("|")]
        assert len(cols) == 3 and "none" not in cols[2], line  # every selection is dispatched
        out.setdefault(family, []).append(tuple(tuple(int(w) for w in c.split()) for c in cols))
    return out


def test_variant_check_under_sanitizers(tmp_path, output):
    # a stand-alone host program: the sanitizers' runtimes are linked in
    exe = _build(tmp_path, "variant_check_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    assert _run(exe) == output


# ---- the launchers' ladders before the selectors --------------------------------
# a scene and environment row: lds n_prims tables vol_flags eng lane notab unfused
def vol_packet(n_prims, lane):   # mh_volwave.hip
    return n_prims > 0 and n_prims <= PACKET_MAX_PRIMS and not lane


def use_packet(n_prims, lane):   # mh_wavefront.hip
    if n_prims > PACKET_MAX_PRIMS:
        return False
    return not lane


def lpt(lds, n_prims, tables, lane, notab):
    """launch_vol_sched(_bwd): the (L, P, T) home of k_vol_sched"""
    pk, tab = vol_packet(n_prims, lane), tables and not notab
    if pk and tab:
        return (0, 1, 1)
    if pk:
        return (0, 1, 0)
    if lds:
        return (1, 0, 0)
    return (0, 0, 0)


def launch_vol_sched(lds, n_prims, tables, vol_flags, eng, lane, notab, unfused, type_):
    blend, pv = vol_flags & VOL_PHASE_BLEND, type_ == PRBVOLPATH
    if pv and blend:
        m = "PvMachineBlend"
    elif pv:
        m = "PvMachine"
    elif blend:
        m = "VolMachineBlend"
    elif vol_flags & VOL_PHASE_EXT:
        m = "VolMachine"
    else:
        m = "VolMachineHg"
    return (m,) + lpt(lds, n_prims, tables, lane, notab)


def launch_vol_sched_bwd(lds, n_prims, tables, vol_flags, eng, lane, notab, unfused, emitter_off):
    blend = vol_flags & VOL_PHASE_BLEND
    if emitter_off and blend:
        m = "PvBwdMachineEmBlend"
    elif emitter_off:
        m = "PvBwdMachineEm"
    elif blend:
        m = "PvBwdMachineBlend"
    else:
        m = "PvBwdMachine"
    return (m,) + lpt(lds, n_prims, tables, lane, notab)


def launch_volwave(lds, n_prims, tables, vol_flags, eng, lane, notab, unfused, first):
    """k_vw_main<F, L, P, Ph>; k_vw_finish<L, P, Ph> and k_vw_walk<L, P> take the same L, P"""
    pk = vol_packet(n_prims, lane)
    ph = PH_BLEND if vol_flags & VOL_PHASE_BLEND else PH_EXT
    if pk:
        flp = (1, 0, 1) if first else (0, 0, 1)
    elif first:
        flp = (1, 1, 0) if lds else (1, 0, 0)
    else:
        flp = (0, 1, 0) if lds else (0, 0, 0)
    return (flp[0], ph, flp[1], flp[2], 0)  # as handed: Fresh, Ph, L, P, no tables


def launch_lane_vol(lds, n_prims, tables, vol_flags, eng, lane, notab, unfused):
    """k_prbvol_backward<L, Ph> (launch_prb_backward), k_pvb_replay_paths<L, Ph> (launch_vol_sched_bwd_replays)"""
    blend = vol_flags & VOL_PHASE_BLEND
    if lds and blend:
        lp = (1, PH_BLEND)
    elif blend:
        lp = (0, PH_BLEND)
    elif lds:
        lp = (1, PH_EXT)
    else:
        lp = (0, PH_EXT)
    return (0, lp[1], lp[0], 0, 0)  # as handed: not fresh, Ph, L, no packets, no tables


def launch_render(lds, n_prims, tables, vol_flags, eng, lane, notab, unfused, type_):
    blend = vol_flags & VOL_PHASE_BLEND
    if type_ == PRB:
        return (PRB, lds, PH_EXT)
    if type_ == VOLPATH and blend:
        return (VOLPATH, lds, PH_BLEND)
    if type_ == VOLPATH:
        return (VOLPATH, lds, PH_EXT)
    if type_ == PRBVOLPATH and blend:
        return (PRBVOLPATH, lds, PH_BLEND)
    if type_ == PRBVOLPATH:
        return (PRBVOLPATH, lds, PH_EXT)
    return (PATH, lds, PH_EXT)


def launch_render_forward(lds, n_prims, tables, vol_flags, eng, lane, notab, unfused, type_):
    vol = type_ == PRBVOLPATH
    blend = vol and vol_flags & VOL_PHASE_BLEND
    if blend and lds:
        return (1, 1, PH_BLEND)
    if blend:
        return (1, 0, PH_BLEND)
    if vol and lds:
        return (1, 1, PH_EXT)
    if vol:
        return (1, 0, PH_EXT)
    if lds:
        return (0, 1, PH_EXT)
    return (0, 0, PH_EXT)


def wf_dispatch(lds, n_prims, tables, vol_flags, eng, lane, notab, unfused, n_rgb):
    """MH_WF_DISPATCH(_NR): K<L, P, [NR,] Eng>; NR = 1 where n_rgb == 1, else kMaxRgbParams"""
    packet = use_packet(n_prims, lane)
    if lds and packet:
        k = (1, 1, ENG_BVH2)
    elif lds:
        k = (1, 0, ENG_BVH2)
    elif packet:
        k = (0, 1, ENG_BVH2)
    elif eng == ENG_QUANT:
        k = (0, 0, ENG_QUANT)
    elif eng == ENG_WIDEC:
        k = (0, 0, ENG_WIDEC)
    elif eng == ENG_WIDE:
        k = (0, 0, ENG_WIDE)
    else:
        k = (0, 0, ENG_BVH2)
    return k + (1 if n_rgb == 1 else 0,)


def shade_prb(lds, n_prims, tables, vol_flags, eng, lane, notab, unfused, n_rgb, em):
    """k_wf_shade_prb<Staged, NR, Em> (and k_wf_shade<Staged>)"""
    if n_rgb == 1:
        return (1, 1, em) if tables else (0, 1, em)
    return (1, 0, em) if tables else (0, 0, em)


def wf_fused(lds, n_prims, tables, vol_flags, eng, lane, notab, unfused):
    return (int(bool(use_packet(n_prims, lane) and tables and not unfused)),)


def bounce_prb(first, n_rgb, with_bmp, det_on, em):
    """k_wf_bounce_prb<NR, Gen, Bm, Det, Em>; NR = 1 where n_rgb <= 1"""
    if with_bmp and det_on:
        gbd = (1, 1, 1) if first else (0, 1, 1)
    elif with_bmp:
        gbd = (1, 1, 0) if first else (0, 1, 0)
    elif det_on:
        gbd = (1, 0, 1) if first else (0, 0, 1)
    else:
        gbd = (1, 0, 0) if first else (0, 0, 0)
    return (1 if n_rgb <= 1 else 0,) + gbd + (em,)


def launch_develop(fmt):
    return {PIXEL_Y: (PIXEL_Y, 0), PIXEL_XYZ: (PIXEL_XYZ, 0), PIXEL_RGBA: (PIXEL_RGB, 1), PIXEL_YA: (PIXEL_Y, 1),
            PIXEL_XYZA: (PIXEL_XYZ, 1)}.get(fmt, (PIXEL_RGB, 0))


def bitmap_scatter(fx, fx_pass, in_lds):
    if fx:
        return (0, fx_pass)
    if in_lds:
        return (1, 0)
    return (0, 0)


# ---- the comparison -----------------------------------------------------------------
def _check(rows, family, n_cases, ladder, named=None):
    """every row of the family: dispatch hands on what the ladder launched"""
    assert len(rows[family]) == n_cases
    assert len({r[0] for r in rows[family]}) == n_cases  # distinct inputs
    for inputs, key, handed in rows[family]:
        want = tuple(int(v) if not isinstance(v, str) else named.index("k" + v) for v in ladder(*inputs))
        assert handed == want, (family, inputs, key)


FACTS = 2 * 4 * 2 * 5 * 4 * 8  # each_facts of variant_check.cpp


def test_vol_sched(rows):
    machines = _enum("Machine")
    _check(rows, "vol_sched", FACTS * 4, launch_vol_sched, machines)
    _check(rows, "vol_sched_bwd", FACTS * 2, launch_vol_sched_bwd, machines)
    for family in ("vol_sched", "vol_sched_bwd"):
        for inputs, key, handed in rows[family]:
            assert key[0] == handed[0]
    # mh_volwave.hip's type list is in the enum's order
    types = re.search(r"using VsMachines = std::tuple<(.*?)>;", _read(CSRC, "mh_volwave.hip"), re.S).group(1)
    assert ["k" + t.strip() for t in types.split(",")] == machines
    # the k_vol_sched instances: 9 machines x 4 homes, each reached by some input
    reached = {h for f in ("vol_sched", "vol_sched_bwd") for _, _, h in rows[f]}
    assert len(reached) == 36


def test_volwave_and_lane_kernels(rows):
    _check(rows, "volwave", FACTS * 2, launch_volwave)
    _check(rows, "vol_lane", FACTS, launch_lane_vol)
    assert len({h for _, _, h in rows["volwave"]}) == 12  # k_vw_main's instances


def test_render(rows):
    _check(rows, "render", FACTS * 6, launch_render)
    _check(rows, "render_forward", FACTS * 6, launch_render_forward)
    assert len({h for _, _, h in rows["render"]}) == 12
    assert len({h for _, _, h in rows["render_forward"]}) == 6


def test_wavefront(rows):
    _check(rows, "wf_trace", FACTS * 4, wf_dispatch)
    _check(rows, "shade_prb", FACTS * 8, shade_prb)
    _check(rows, "bounce_prb", 64, bounce_prb)
    assert len({h[:3] for _, _, h in rows["wf_trace"]}) == 7  # 3 + the four stream engines
    for inputs, key, handed in rows["wf_fused"]:
        assert key == wf_fused(*inputs)
    assert len(rows["wf_fused"]) == FACTS


def test_packet_rules_differ_on_the_empty_scene(rows):
    # vol_packet has an n_prims > 0 term that use_packet has not
    vw = {i[:8]: h for i, _, h in rows["volwave"] if i[8] == 0}
    wf = {i[:8]: h for i, _, h in rows["wf_trace"] if i[8] == 1}
    for facts in vw:
        lane, n_prims = facts[5], facts[1]
        assert vw[facts][3] == int(0 < n_prims <= PACKET_MAX_PRIMS and not lane)
        assert wf[facts][1] == int(n_prims <= PACKET_MAX_PRIMS and not lane)


def test_develop_scatter(rows):
    _check(rows, "develop", 8, launch_develop)
    _check(rows, "bitmap_scatter", 6, bitmap_scatter)


# ---- source shape ---------------------------------------------------------------------
def test_header_is_host_only():
    text = _read(CSRC, "mh_variant.hpp")
    assert "hip_runtime" not in text and "getenv" not in text and "mh_env.hpp" not in text


def test_no_launch_macros_remain():
    gone = ("MH_VS1", "MH_VSB", "MH_VW_FIN", "MH_VW_MAIN(", "MH_VW_WALK(", "MH_LAUNCH_RENDER", "MH_SPLAT_PX",
            "MH_SPLAT_GEN", "MH_SPLAT_GATHER", "MH_PRB_BACKWARD", "MH_WF_DISPATCH", "MH_BOUNCE_FWD", "MH_BOUNCE_PRB(",
            "MH_BOUNCE_PRB_NR", "MH_SHADE_PRB")
    for name in ("mh_kernels.hip", "mh_wavefront.hip", "mh_volwave.hip"):
        text = _read(CSRC, name)
        for macro in gone:
            assert macro not in text, (name, macro)
        assert not re.search(r"#define MH_VS\(", text), name
