"""When the fused wavefront runs the camera bounce and the bounce after it in
one launch (variant::bounce_path, csrc/mh_variant.hpp), checked without a GPU:
tools/fuse01_check.cpp is plain C++17 built with the host compiler and prints
the rule's answer on plain values.  The expected answers below are the rule as
the design states it, not a transcription of the header."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mitsuba3-nasa_amd", "csrc")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")

PARK_BYTES = 4 * 64 * 16 * 4   # four waves, 64 lanes, 16 dwords
MAX_LDS = 32768                # five workgroups on a CU's 160 KB


def _build(tmp, name, *flags):
    exe = str(tmp / name)
    subprocess.run([CXX, "-std=c++17", "-Wall", *flags, os.path.join(ROOT, "tools", "fuse01_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    return exe


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _rows(output):
    out = {}
    for line in output.splitlines():
        family, *cols = [c.strip() for c in line.split("|")]
        out.setdefault(family, []).append(tuple(tuple(int(w) for w in c.split()) for c in cols))
    return out


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    assert CXX, "a host C++ compiler"
    return _run(_build(tmp_path_factory.mktemp("fuse01"), "fuse01_check", "-O1"))


@pytest.fixture(scope="module")
def rows(output):
    return _rows(output)


@pytest.fixture(scope="module")
def cases(rows):
    """(tables, unfused, max_depth, lds) -> ((two, next, next_buf), (Gen, Two))"""
    got = {i: (k, h) for i, k, h in rows["bounce_path"]}
    assert len(got) == len(rows["bounce_path"]) == 2 * 2 * 5 * 6
    return got


def test_fuse01_check_under_sanitizers(tmp_path, output):
    # a stand-alone host program: the sanitizers' runtimes are linked in
    exe = _build(tmp_path, "fuse01_check_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    assert _run(exe) == output


def test_limits(rows):
    (on, dwords, park, max_lds), = rows["limits"][0][:1]
    assert on == 1  # the default build
    assert dwords <= 16 and park == PARK_BYTES == 16384 and max_lds == MAX_LDS
    assert 5 * max_lds <= 160 * 1024 < 6 * max_lds  # five workgroups per CU, not six


def test_rule(cases):
    for (tables, unfused, max_depth, lds), (key, handed) in cases.items():
        fused = bool(tables) and not unfused  # (a 32-primitive packet scene)
        want = fused and max_depth >= 2 and lds + PARK_BYTES <= MAX_LDS
        assert key[0] == int(want), (tables, unfused, max_depth, lds)
        assert handed == (1, int(want))  # the first launch generates; Two only by the rule


def test_max_depth(cases):
    assert cases[(1, 0, 1, 13856)][0][0] == 0
    assert cases[(1, 0, 2, 13856)][0][0] == 1
    assert cases[(1, 0, 64, 13856)][0][0] == 1


def test_unfused_scene(cases):
    for max_depth in (1, 2, 8):
        assert cases[(1, 1, max_depth, 13856)][0][0] == 0  # MH_WF_FUSED=0
        assert cases[(0, 0, max_depth, 13856)][0][0] == 0  # no shading tables in LDS


def test_lds_threshold(cases):
    assert cases[(1, 0, 8, 16384)][0][0] == 1
    assert cases[(1, 0, 8, 16385)][0][0] == 0
    assert cases[(1, 0, 8, 13856)][0][0] == 1  # the cornell box: 13,856 + 16,384 = 30,240 B


def test_loop_continues_where_bounce_1_left_off(cases):
    # bounce b reads ping-pong buffer b & 1 and counter block b; it writes buffer (b + 1) & 1 and
    # block b + 1.  So bounce 1 writes buffer 0 and block 2, and bounce 0 alone buffer 1 and block 1.
    for (key, _) in cases.values():
        two, nxt, buf = key
        last = 1 if two else 0  # the last bounce the first launch ran
        assert nxt == last + 1 and buf == (last + 1) & 1


def test_later_launches(rows):
    assert rows["later"][0][2] == (0, 0)


def test_switch_off_builds_the_parent_launches(tmp_path):
    out = _rows(_run(_build(tmp_path, "fuse01_check_off", "-O1", "-DMH_WF_FUSE01=0")))
    assert out["limits"][0][0][0] == 0
    for _, key, handed in out["bounce_path"]:
        assert key == (0, 1, 1) and handed == (1, 0)


def test_rule_is_host_only():
    text = open(os.path.join(CSRC, "mh_variant.hpp"), encoding="utf-8").read()
    assert "bounce_path" in text and "hip_runtime" not in text and "getenv" not in text
