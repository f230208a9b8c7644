"""The host-only slot, meta-block and fixed-point layouts (csrc/mh_slots.hpp),
checked without a GPU: tools/slots_check.cpp is plain C++17 built with the
host compiler; it prints the layouts of fixed cases, and the expected values
below are literals worked out from the rules (the offsets the kernels read,
the padding of the slot block, the error texts of the C-ABI), not from the
header's own output."""
import json
import math
import os
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mitsuba3-nasa_amd", "csrc")
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")


def _build(tmp, name, *flags):
    exe = str(tmp / name)
    subprocess.run([CXX, "-std=c++17", "-Wall", *flags, os.path.join(ROOT, "tools", "slots_check.cpp"), "-o", exe],
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
    return _run(_build(tmp_path_factory.mktemp("slots"), "slots_check", "-O1"))


def test_slots_check_under_sanitizers(tmp_path, cases):
    # a stand-alone host program: the sanitizers' runtimes are linked in
    exe = _build(tmp_path, "slots_check_san", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    assert _run(exe) == cases


def _sub(case, **want):
    got = {k: case[k] for k in want}
    assert got == want


def test_constants(cases):
    # four register-accumulated and four large slots; the fixed-point words as the kernels read them
    assert cases["constants"] == dict(max_rgb=4, max_bitmap=4, max_params=8, fx_max_off=0, fx_scale_off=64,
                                      fx_sum_off=192, fx_word_bytes=512)
    # u32 maxima (grid + 8 slots), 8 double scales, 3 x 4 int64 sums: none overlaps the next
    assert 0 + 4 * 9 <= 64 and 64 + 8 * 8 <= 192 and 192 + 8 * 12 <= 512


FX_EXP = {  # name: (float bits, S)
    "zero": (0x00000000, 31),
    "inf": (0x7F800000, 31),
    "nan": (0x7FC00000, 31),
    "one": (0x3F800000, 30),
    "two_31": (0x4F000000, -1),
    "denormal_min": (0x00000001, 179),  # 2^-149
    "flt_max": (0x7F7FFFFF, -97),
    "three_quarters": (0x3F400000, 31),  # 0.75 < 2^0
}


@pytest.mark.parametrize("name", sorted(FX_EXP))
def test_fx_exp(cases, name):
    bits, S = FX_EXP[name]
    assert cases["fx_exp_" + name] == dict(bits=bits, S=S)
    x = struct.unpack("<f", struct.pack("<I", bits))[0]
    if math.isfinite(x) and x > 0:  # round(x * 2^S) fits an int32, and no larger S does
        assert math.ldexp(x, S) < 2.0 ** 31 <= math.ldexp(x, S + 1)


def test_fx_exp_bit_patterns():
    f = lambda b: struct.unpack("<f", struct.pack("<I", b))[0]
    assert f(0x3F800000) == 1.0 and f(0x4F000000) == 2.0 ** 31 and f(0x00000001) == 2.0 ** -149
    assert f(0x7F7FFFFF) == (2.0 - 2.0 ** -23) * 2.0 ** 127 and math.isinf(f(0x7F800000)) and math.isnan(f(0x7FC00000))


def test_fx_scales(cases):
    # maxima: grid 1.0 (S 30), slot 0 nothing (31), slot 1 2^31 (-1), slot 4 FLT_MAX (-97)
    c = cases["fx_scales"]
    assert c["scale"] == 2.0 ** 30 and c["inv"] == 2.0 ** -30
    assert c["slot_scale"] == [2.0 ** 31, 2.0 ** -1, 2.0 ** -97]
    assert c["slot_inv"] == [2.0 ** -31, 2.0 ** 1, 2.0 ** 97]
    assert c["product"] == 1.0


def test_slot_block(cases):
    # every slot padded to whole float4s, one after the other
    _sub(cases["block_mixed"], off=[0, 4, 8, 8, 8, 20, 20, 20], total=20, alloc_floats=20, bmp_floats=12,
         bmp_off=[0, 12, 12, 12], padded=[4, 4, 0, 0, 12, 0, 0, 0])
    _sub(cases["block_empty"], off=[0] * 8, total=0, alloc_floats=1, bmp_floats=0, bmp_off=[0] * 4)
    # 60 | 4 | 7 -> 8 | 1 -> 4 floats behind the one small slot
    _sub(cases["block_bitmaps"], off=[0, 4, 4, 4, 4, 64, 68, 76], total=80, alloc_floats=80, bmp_floats=76,
         bmp_off=[0, 60, 64, 72])


def test_meta_layout(cases):
    # slot, is_rgb, bufs, sigma, albedo, phase, corner, emitter, size
    _sub(cases["meta_3_2_1"], offsets=[0, 16, 48, 112, 128, 136, 144, 208, 224], contracts=1)
    # an empty scene: every table holds one entry
    _sub(cases["meta_empty"], offsets=[0, 16, 48, 112, 128, 132, 144, 208, 224], contracts=1, emitter_off=0)


@pytest.mark.parametrize("n_media", [1, 2, 5])
def test_meta_phase_table_follows_albedo(cases, n_media):
    # the kernels read the g slot of medium m as albedo_slot[n_media + m]
    c = cases[f"meta_media_{n_media}"]
    albedo, phase = c["offsets"][4], c["offsets"][5]
    assert phase - albedo == 4 * n_media and c["contracts"] == 1


def test_meta_emitter_offset(cases):
    # listed: the table's non-zero byte offset from slot_of_tex; not listed: 0 (the kernels without the emitter terms)
    assert cases["meta_3_2_1"]["emitter_off"] == 208
    assert cases["meta_media_5"]["emitter_off"] == cases["meta_media_5"]["offsets"][7] != 0
    _sub(cases["meta_emitter_unlisted"], emitter_off=0, contracts=1)
    for name in ("meta_media_1", "meta_media_2"):
        assert cases[name]["emitter_off"] == 0


def test_meta_image(cases):
    # albedo of medium 0 -> slot 0, its g -> slot 1, the radiance of emitter 1 -> slot 2; two media, two emitters
    # ten textures: 48 | 80 | 144 | 160 168 | 176 | 240 | 256
    assert cases["meta_image"] == dict(size=256, albedo=[0, -1], g_after_albedo=[1, -1], emitter_by_offset=[-1, 2],
                                       contracts=1)


def test_build_slots_kinds(cases):
    # tex 0 (rgb), tex 1 (4 x 5 x 3 bitmap), sigma_t of medium 0 (homogeneous) and 1 (a 2 x 3 x 4 grid),
    # albedo and g of medium 0: small slots count up from 0, large ones from 4
    c = cases["build_kinds"]
    _sub(c, code=0, failed=0, msg="", slot_of_param=[0, 4, 1, 5, 2, 3], counts=[3, 1, 3, 1, 60, 24, 0, 0],
         is_rgb=[1, 1, 1, 1, 0, 0, 0, 0], n_rgb=4, n_bmp=2, n_medium_params=4, n_emitter_params=0, n_phase_params=1,
         bmp_tex=1, sigma_slot=[1, 5], albedo_slot=[2, -1], phase_slot=[3, -1], emitter_slot=[-1, -1],
         slot_of_tex=[0, 4] + [-1] * 8)
    assert c["grid_res"] == [0] * 15 + [2, 3, 4] + [0] * 6  # slot 5 only
    # an emitter's radiance is a small slot of 3; textures need no prbvolpath
    _sub(cases["build_emitter"], code=0, slot_of_param=[0, 1, 4], counts=[3, 3, 0, 0, 4, 0, 0, 0], n_rgb=2, n_bmp=1,
         n_emitter_params=1, n_medium_params=0, emitter_slot=[-1, 0], bmp_tex=3)
    _sub(cases["build_none"], code=0, slot_of_param=[], counts=[0] * 8, n_rgb=0, n_bmp=0)
    _sub(cases["build_four_each"], code=0, slot_of_param=[0, 1, 2, 3, 4, 5, 6, 7], counts=[3, 3, 3, 3, 60, 4, 3, 3],
         n_rgb=4, n_bmp=4)


INVALID, UNSUPPORTED = 1, 4  # MH_ERR_INVALID_ARGUMENT, MH_ERR_UNSUPPORTED
NOT_VOL = "(): medium parameters require the 'prbvolpath' integrator"
ERRORS = {
    "build_too_many_rgb": (UNSUPPORTED, "mh_render_backward: too many rgb parameters"),
    "build_too_many_small_mixed": (UNSUPPORTED, "mh_render_backward: too many rgb parameters"),
    "build_too_many_bitmap": (UNSUPPORTED, "mh_render_backward: too many bitmap parameters"),
    "build_too_many_large_mixed": (UNSUPPORTED, "mh_render_backward: too many bitmap parameters"),
    "build_duplicate": (INVALID, "mh_render_backward: duplicate parameter"),
    "build_duplicate_medium": (INVALID, "mh_render_backward: duplicate parameter"),
    "build_texture_range": (INVALID, "mh_render_backward: texture index out of bounds"),
    "build_medium_range": (INVALID, "mh_render_backward: medium index out of bounds"),
    "build_phase_range": (INVALID, "mh_render_backward: medium index out of bounds"),
    "build_emitter_range": (INVALID, "mh_render_backward: emitter index out of bounds"),
    "build_medium_not_vol": (UNSUPPORTED, "render_backward" + NOT_VOL),
    "build_phase_not_vol": (UNSUPPORTED, "render_forward" + NOT_VOL),
    "build_phase_not_hg": (UNSUPPORTED, "render_backward(): MH_PARAM_MEDIUM_PHASE_G needs a medium whose phase function "
                                        "is MH_PHASE_HG (other phase functions' parameters are not differentiable)"),
    "build_unknown_kind": (INVALID, "mh_render_backward: unknown parameter kind"),
    "build_forward_names": (INVALID, "mh_render_forward: texture index out of bounds"),
}


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_build_slots_errors(cases, name):
    code, msg = ERRORS[name]
    assert cases[name] == dict(code=code, failed=1, msg=msg)


def test_corner_layout(cases):
    # a (2, 3, 4) grid: 3 x 4 x 5 padded cells of 8 corner values; the slot's block starts the allocation
    use = [0] * 5 + [1, 0, 0]
    _sub(cases["corner_2_3_4"], use=use, off=[0] * 6 + [480, 480], values=480, corner_floats=480, bytes=1920, fits=1)
    _sub(cases["corner_2_3_4_fx"], use=use, values=480, bytes=3840, fits=1)  # int64 sums
    # 2^32 corners: no block (the kernels index corners with 32 bits)
    _sub(cases["corner_two_32"], use=[0] * 8, values=0, fits=0)
    _sub(cases["corner_below_two_32"], use=use, values=(2 ** 32 - 2 ** 16) * 8, fits=0)
    # the 16 GiB (float) and 32 GiB limits are inclusive
    _sub(cases["corner_16_gib"], use=use, values=2 ** 32, bytes=16 << 30, fits=1)
    _sub(cases["corner_32_gib_fx"], use=use, values=2 ** 32, bytes=32 << 30, fits=1)
    _sub(cases["corner_over_16_gib"], use=use, fits=0)
    _sub(cases["corner_over_32_gib_fx"], use=use, fits=0)
    _sub(cases["corner_none"], use=[0] * 8, values=0, bytes=0, fits=0)


def test_source_shape():
    """mh_slots.hpp is host-only, and the layouts' numbers live nowhere else."""
    hdr = open(os.path.join(CSRC, "mh_slots.hpp")).read()
    assert "hip/" not in hdr and "getenv" not in hdr and "static " not in hdr.replace("static_assert", "")
    api = open(os.path.join(CSRC, "mh_api.hip")).read()
    shading = open(os.path.join(CSRC, "mh_shading.hpp")).read()
    assert "+ 3) / 4 * 4" not in api
    for text in (api, shading):
        for line in text.splitlines():
            if "fx_word" in line or "fx_max" in line:
                code = line.split("//")[0]
                assert "+ 64" not in code and "+ 192" not in code and "alloc(512)" not in code, line
