"""The host-only scene build (csrc/mh_scene_build.hpp, mh_records.hpp), checked
without a GPU.  tools/scene_check.cpp is a stand-alone program: it reads the
descriptions and tables this test writes to files and prints what the header
makes of them; every expected value below is a literal or a numpy / struct
restatement of the rule, never the header's own output.  The program is built
twice, the second time with AddressSanitizer and UBSan, and both must print
the same.

assemble's media list: 0 tabulated (3 nodes); 1 a blend (hg, tabulated) whose
child table arrives in the second step; 2 and 3 blends with 4 x 4 x 4 and
5 x 3 x 2 weight grids, set in the third step behind 128 floats of the media's
own grids; 4 tabulated, its table arriving last."""
import json
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import phase_cases
import scene_cases as SC
from mitsuba_hip import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mitsuba3-nasa_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
INV = A.INVALID


def _build(tmp, name, *flags):
    # the checker as plain C++, mh_bvh.cpp the way tests/test_bvh_build.py builds it; no contraction, as the library
    exe = str(tmp / name)
    subprocess.run([HIPCC, "-std=c++17", "-Wall", "-ffp-contract=off", *flags, os.path.join(ROOT, "tools", "scene_check.cpp"),
                    "-x", "hip", "--offload-arch=gfx950", os.path.join(CSRC, "mh_bvh.cpp"), "-o", exe, "-lpthread"],
                   check=True, capture_output=True)
    return exe


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("scene")


@pytest.fixture(scope="module")
def exes(work):
    """the checker, and the checker under the sanitizers (a stand-alone host program: their runtimes are linked in)"""
    return (_build(work, "scene_check", "-O1"),
            _build(work, "scene_check_san", "-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                   "-Xarch_host", "-fno-sanitize-recover=all"))


def _run(exes, *args):
    outs = []
    for exe in exes:
        r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1], "the sanitized build prints something else"
    return [json.loads(line) for line in outs[0].splitlines()]


def _file(work, name, data):
    path = str(work / name)
    with open(path, "wb") as f:
        f.write(data)
    return path


def _f32(words):
    return np.array(words, np.uint32).view(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).ravel().tolist()


# ---------------------------------------------------------------------------
# validate
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def verdicts(work, exes):
    names = ["valid"] + sorted(SC.FAULTS) + sorted(SC.ORDER)
    files = [_file(work, n, (SC.base() if n == "valid" else SC.faulty(n)).blob()) for n in names]
    rows = _run(exes, "validate", *files)
    return {r["case"]: (r["code"], r["msg"]) for r in rows}


def test_valid_description_passes(verdicts):
    assert verdicts["valid"] == (0, "")


@pytest.mark.parametrize("name", sorted(SC.FAULTS))
def test_each_rejection(verdicts, name):
    assert verdicts[name] == SC.FAULTS[name][1:]


@pytest.mark.parametrize("name", sorted(SC.ORDER))
def test_first_failure_order(verdicts, name):
    assert verdicts[name] == SC.ORDER[name][1:]


def test_every_rejection_of_the_header_has_a_case():
    hdr = open(os.path.join(CSRC, "mh_scene_build.hpp")).read()
    body = hdr[hdr.index("inline Error validate("):hdr.index("inline std::vector<BuildPrim> build_prims(")]
    texts = {t for _, _, t in SC.FAULTS.values()}
    found = re.findall(r'(?:invalid\(|unsupported\(|MH_ERR_INVALID_ARGUMENT, )"([^"]+)"', body) + \
        re.findall(r'\{d\.\w+, [^,]+, "([^"]+)"\}', body)
    assert len(found) >= 30
    for text in found:  # (the first piece of a literal that spans lines)
        assert any(text in t for t in texts), text


# ---------------------------------------------------------------------------
# build_prims, key_table, pair_records, records
# ---------------------------------------------------------------------------
def seven_prims():
    """the rectangle and a six-triangle fan; a second (2 x 2 x 2) grid medium behind the first"""
    d = SC.base()
    ang = np.linspace(0, 2 * np.pi, 7)[:6]
    d.positions = np.concatenate([[[0.05, -1.0, 0.02]], np.stack([np.cos(ang), -1 + 0.01 * ang, np.sin(ang)], 1)]).astype(np.float32)
    d.faces = np.array([[0, 1 + k, 1 + (k + 1) % 6] for k in range(6)], np.uint32)
    d.shapes[1].face_count, d.shapes[1].vertex_count = 6, 7
    het2 = A.Medium()
    het2.type, het2.phase, het2.scale, het2.max_density = A.MEDIUM_HETEROGENEOUS, A.PHASE_TABULATED, 0.5, 8.0
    het2.grid_res[:] = [2, 2, 2]
    het2.grid_offset = 30
    d.media.append(het2)
    d.grid = np.concatenate([d.grid, np.arange(8, dtype=np.float32) + 100])
    d.shapes[1].interior_medium = 2
    return d


@pytest.fixture(scope="module")
def built(work, exes):
    d = seven_prims()
    path = _file(work, "seven", d.blob())
    return d, _run(exes, "build", path, 7)[0], _run(exes, "build", path, 6)[0]


def test_build_prims_bits(built):
    d, out, _ = built
    assert out["prim_bytes"] == 84  # lo[3] hi[3] rec[12] shape prim type
    prims = np.array(out["prims"], np.uint32).reshape(-1, 21)
    assert len(prims) == 7
    # the rectangle: per axis min / max over the corners of m0 * cx + m1 * cy + m3, in float32, in this order
    m = np.array(d.shapes[0].to_world[:], np.float32).reshape(3, 4)
    corners = [(-1, -1), (-1, 1), (1, -1), (1, 1)]
    q = np.array([[(m[a, 0] * np.float32(cx) + m[a, 1] * np.float32(cy)) + m[a, 3] for a in range(3)] for cx, cy in corners],
                 np.float32)
    assert q.dtype == np.float32
    assert prims[0, :3].tolist() == _bits(q.min(0)) and prims[0, 3:6].tolist() == _bits(q.max(0))
    assert prims[0, 6:18].tolist() == _bits(np.array(d.shapes[0].to_object[:], np.float32))
    assert prims[0, 18:].tolist() == [0, INV, A.SHAPE_RECTANGLE]
    # the triangles: v0, e1 = v1 - v0, e2 = v2 - v0 (float32 subtractions that round)
    rounds = 0
    for f, (i0, i1, i2) in enumerate(d.faces.tolist()):
        v0, v1, v2 = d.positions[i0], d.positions[i1], d.positions[i2]
        e1, e2 = v1 - v0, v2 - v0
        assert e1.dtype == np.float32
        rounds += int((e1.astype(np.float64) != v1.astype(np.float64) - v0.astype(np.float64)).any())
        p = prims[1 + f]
        assert p[:3].tolist() == _bits(np.minimum(v0, np.minimum(v1, v2)))
        assert p[3:6].tolist() == _bits(np.maximum(v0, np.maximum(v1, v2)))
        rec = _f32(p[6:18])
        assert p[6:9].tolist() == _bits(v0) and p[10:13].tolist() == _bits(e1) and p[14:17].tolist() == _bits(e2)
        assert rec[3] == 0 and rec[7] == 0 and rec[11] == 0
        assert p[18:].tolist() == [1, f, A.SHAPE_MESH]
    assert rounds >= 3, "the case is meant to round"


def test_key_table_inverts_the_leaf_order(built):
    d, out, _ = built
    assert out["n_prims"] == 7
    leaf = np.array(out["bvh_prims"], np.uint32).reshape(7, 16)  # a b c info; info = shape, prim, type, key
    keys = leaf[:, 15].tolist()
    assert sorted(keys) == list(range(7))
    table = np.array(out["key_table"], np.uint32).reshape(7, 2)
    for i, k in enumerate(keys):
        assert table[k].tolist() == leaf[i, 12:14].tolist()
    # the key is the scene order: the rectangle, then the faces
    assert table.tolist() == [[0, INV]] + [[1, f] for f in range(6)]


def test_pair_records(built):
    _, out, small = built
    leaf = np.array(out["bvh_prims"], np.uint32).reshape(7, 16)
    pairs = np.array(out["pairs"], np.uint32).reshape(7, 16, 2)
    for i in range(7):
        assert pairs[i, :, 0].tolist() == leaf[i].tolist()
        assert pairs[i, :, 1].tolist() == leaf[min(i + 1, 6)].tolist()
    assert small["pairs"] == [] and small["key_table"] == out["key_table"]  # 7 primitives above a limit of 6


def _pad(xs, n):
    return list(xs) + [0.0] * (n - len(xs))


def test_record_bytes(built):
    d, out, _ = built
    f32 = np.float32
    shapes = b""
    for s in d.shapes:
        shapes += struct.pack("<8I12f12ff3I", s.type, s.bsdf, s.emitter, s.face_offset, s.vertex_offset, s.has_normals,
                              s.has_texcoords, 0, *s.to_world, *_pad(s.frame_s, 4), *_pad(s.frame_t, 4), *_pad(s.frame_n, 4),
                              s.inv_area, s.interior_medium, s.exterior_medium, 0)
    assert len(shapes) == 144 * 2 and np.frombuffer(shapes, np.uint32).tolist() == out["shapes"]
    media, grid_off = b"", [0, 0, 128]
    for i, m in enumerate(d.media):
        maj = f32(m.sigma_t_const) * f32(m.scale) if m.type == A.MEDIUM_HOMOGENEOUS else f32(m.scale) * f32(m.max_density)
        media += struct.pack("<4I4f4f4IQ2I12f4f4f", m.type, m.phase, m.flags, 0, m.g, m.scale, maj, m.sigma_t_const,
                             *_pad(m.albedo, 4), *m.grid_res, 0, grid_off[i], 0, 0, *m.grid_to_local, *_pad(m.bbox_min, 4),
                             *_pad(m.bbox_max, 4))
    assert len(media) == 160 * 3 and np.frombuffer(media, np.uint32).tolist() == out["media"]
    assert out["grid_offsets"] == grid_off
    # the majorants themselves, as literals: 0.7 * 1.3 and 2.5 * 1.9 in float32
    maj = _f32(np.array(out["media"], np.uint32).reshape(3, 40)[:, 6])
    assert maj.tolist() == [f32(f32(0.7) * f32(1.3)), f32(f32(2.5) * f32(1.9)), f32(4.0)]
    assert out["bsdf_type"] == [A.BSDF_DIFFUSE, A.BSDF_DIFFUSE] and out["bsdf_tex"] == [0, 1]
    tex = b""
    for t in d.textures:
        tex += struct.pack("<4IQ2I4f8f", t.type, t.width, t.height, t.channels, t.data_offset, t.filter, t.wrap,
                           *_pad(t.value, 4), *_pad(t.to_uv, 8))
    assert len(tex) == 80 * 2 and np.frombuffer(tex, np.uint32).tolist() == out["textures"]
    em = b""
    for e in d.emitters:
        em += struct.pack("<4I4f4f4f", e.type, e.shape, 0, 0, *_pad(e.radiance, 4), *_pad(e.direction, 4), *e.scene_center,
                          e.scene_radius)
    assert len(em) == 64 and np.frombuffer(em, np.uint32).tolist() == out["emitters"]


def grid_index(x, y, z, rx, ry):
    """4 x 4 x 4 bricks of 64 floats, bricks x-fastest, texels x-fastest inside a brick"""
    nbx, nby = (rx + 3) // 4, (ry + 3) // 4
    return (((z // 4) * nby + y // 4) * nbx + x // 4) * 64 + ((z % 4) * 16 + (y % 4) * 4 + x % 4)


def test_bricked_grids(built):
    d, out, _ = built
    grid = _f32(out["grid"])
    assert grid.size == 128 + 64  # 5 x 3 x 2 -> 2 x 1 x 1 bricks; 2 x 2 x 2 -> 1 brick, behind it
    want = np.zeros(192, np.float32)
    for (rx, ry, rz), src, dst in (((5, 3, 2), 0, 0), ((2, 2, 2), 30, 128)):
        for z in range(rz):
            for y in range(ry):
                for x in range(rx):
                    want[dst + grid_index(x, y, z, rx, ry)] = d.grid[src + (z * ry + y) * rx + x]
    assert grid.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    assert np.count_nonzero(grid[:128]) == 30 and np.count_nonzero(grid[128:]) == 8  # the rest is zero padding
    assert grid_index(4, 2, 1, 5, 3) == 64 + 16 + 8 and grid_index(3, 3, 3, 8, 8) == 63 and grid_index(0, 4, 0, 8, 8) == 128


# ---------------------------------------------------------------------------
# facts
# ---------------------------------------------------------------------------
def counts_only(**counts):
    d = SC.Desc()
    d.counts.update(counts)
    return d


def facts(work, exes, d, node_bytes=64, prim_bytes=64, n_prims=1, depth=1, packet_max=64, shade=1, bvh4_off=0,
          stream_stack=20, stream_threads=1000, depth4=1):
    path = _file(work, "facts_desc", d.blob())
    return _run(exes, "facts", path, node_bytes, prim_bytes, n_prims, depth, packet_max, shade, bvh4_off, stream_stack,
                stream_threads, depth4)[0]


def tab_total(n_shapes, n_bsdfs, n_textures, n_emitters, n_vertices, n_faces, normals, texcoords):
    al = lambda x: (x + 15) // 16 * 16
    return (al(n_shapes * 144) + 2 * al(n_bsdfs * 4) + al(n_textures * 80) + al(n_emitters * 64) + al(n_vertices * 12) +
            (al(n_vertices * 12) if normals else 0) + (al(n_vertices * 8) if texcoords else 0) + al(n_faces * 12))


def test_tables_in_lds_up_to_16_kib(work, exes):
    # 1365 vertices: 16380 -> 16384 bytes; one face more: 16400
    assert tab_total(0, 0, 0, 0, 1365, 0, False, False) == 16384 and tab_total(0, 0, 0, 0, 1365, 1, False, False) == 16400
    at = facts(work, exes, counts_only(n_vertices=1365))
    assert (at["tab_total"], at["tab_bytes"], at["shade_records"]) == (16384, 16384, 1)
    over = facts(work, exes, counts_only(n_vertices=1365, n_faces=1))
    assert (over["tab_total"], over["tab_bytes"], over["shade_records"]) == (16400, 0, 0)
    # every table of the base description, normals and texture coordinates included
    d = SC.base()
    d.normals, d.texcoords = np.zeros((4, 3), np.float32), np.zeros((4, 2), np.float32)
    assert facts(work, exes, d)["tab_total"] == tab_total(2, 2, 2, 1, 4, 2, True, True) == 288 + 32 + 160 + 64 + 48 + 48 + 32 + 32


def test_bvh_in_lds_up_to_32_kib(work, exes):
    d = counts_only()
    at = facts(work, exes, d, node_bytes=16384, prim_bytes=16384, n_prims=256)
    assert (at["lds_bytes_bvh"], at["wide_bvh"]) == (32768, 0)
    over = facts(work, exes, d, node_bytes=16384 + 64, prim_bytes=16384, n_prims=256)
    assert (over["lds_bytes_bvh"], over["wide_bvh"]) == (0, 1)
    # a wide BVH: only above 64 primitives, only when not switched off
    assert facts(work, exes, d, node_bytes=40000, n_prims=64)["wide_bvh"] == 0
    assert facts(work, exes, d, node_bytes=40000, n_prims=65)["wide_bvh"] == 1
    assert facts(work, exes, d, node_bytes=40000, n_prims=65, bvh4_off=1)["wide_bvh"] == 0


def test_too_deep_on_both_sides_of_64_kib(work, exes):
    d = counts_only()
    # depth + 2 entries of 256 x 4 bytes beside the staged BVH
    a = facts(work, exes, d, node_bytes=40000, depth=62)
    assert (a["stack_size"], a["too_deep"]) == (64, 0)
    assert facts(work, exes, d, node_bytes=40000, depth=63)["too_deep"] == 1
    assert facts(work, exes, d, node_bytes=16384, prim_bytes=16384, depth=30)["too_deep"] == 0   # 32768 + 32768
    assert facts(work, exes, d, node_bytes=16384, prim_bytes=16384, depth=31)["too_deep"] == 1
    # the wide BVH's stack, 3 * depth4 + 2: adopted up to 64 entries
    assert facts(work, exes, d, depth=10, depth4=2)["wide_stack"] == 12
    assert facts(work, exes, d, depth=10, depth4=20)["wide_stack"] == 62
    assert facts(work, exes, d, depth=10, depth4=21)["wide_stack"] == 0


def test_stack_cap_and_overflow_columns(work, exes):
    d = counts_only()
    for depth, words in ((17, 0), (18, 0), (19, 1000), (40, 22000)):  # stack 19, 20, 21, 42 against a cap of 20
        assert facts(work, exes, d, depth=depth)["ovf_words"] == words
    assert facts(work, exes, d, depth=10, depth4=10, stream_stack=12, stream_threads=512)["ovf_words_wide"] == (32 - 12) * 512


VOL = {  # (media of shape 0: interior, exterior), phases of the media -> vol_flags
    "none": ((INV, INV), (A.PHASE_HG, A.PHASE_ISOTROPIC), 0),
    "homogeneous": ((0, INV), (A.PHASE_HG, A.PHASE_ISOTROPIC), 2),
    "heterogeneous": ((INV, 1), (A.PHASE_HG, A.PHASE_ISOTROPIC), 1),
    "both": ((0, 1), (A.PHASE_ISOTROPIC, A.PHASE_ISOTROPIC), 3),
    "rayleigh": ((0, INV), (A.PHASE_RAYLEIGH, A.PHASE_ISOTROPIC), 2 | 4),
    "tabulated_unreferenced": ((INV, INV), (A.PHASE_HG, A.PHASE_TABULATED), 4),
    "blend": ((INV, 1), (A.PHASE_HG, A.PHASE_BLEND), 1 | 8),
    "blend_and_tabulated": ((0, 1), (A.PHASE_TABULATED, A.PHASE_BLEND), 3 | 4 | 8),
}


@pytest.mark.parametrize("name", sorted(VOL))
def test_vol_flags(work, exes, name):
    (interior, exterior), phases, want = VOL[name]
    d = SC.base()
    d.shapes[0].interior_medium, d.shapes[0].exterior_medium = interior, exterior
    d.media[0].phase, d.media[1].phase = phases
    d.media[0].g = 0.0
    assert facts(work, exes, d)["vol_flags"] == want


def test_host_divided_floats(work, exes):
    f32 = np.float32
    d = counts_only(n_emitters=3)
    d.sensor.width, d.sensor.height = 48, 7
    got = _f32(facts(work, exes, d)["floats"])
    want = [f32(1) / f32(48), f32(1) / f32(7), f32(1) / f32(3), f32(3), f32(0.07957747154594766788) * (f32(1) / f32(3))]
    assert got.view(np.uint32).tolist() == np.array(want, f32).view(np.uint32).tolist()
    none = _f32(facts(work, exes, counts_only())["floats"])
    assert np.isposinf(none[2]) and none[3] == 0 and np.isposinf(none[4])


# ---------------------------------------------------------------------------
# phase tables
# ---------------------------------------------------------------------------
def _table_file(work, name, cost, values):
    cost, values = np.asarray(cost, np.float32), np.asarray(values, np.float32)
    return _file(work, name, struct.pack("<I", cost.size) + cost.tobytes() + values.tobytes())


@pytest.fixture(scope="module")
def phase_rows(work, exes):
    files = [_table_file(work, "table_" + k, *phase_cases.TABLES[k]) for k in sorted(phase_cases.TABLES)]
    files += [_table_file(work, name, c, v) for name, (c, v, _) in sorted(PHASE_FAULTS.items())]
    return {r["case"]: r for r in _run(exes, "phase_table", *files)}


@pytest.mark.parametrize("key", sorted(phase_cases.TABLES))
def test_phase_table_matches_the_distribution(phase_rows, key):
    cost, values = phase_cases.TABLES[key]
    D = phase_cases.Distr(cost, values, np.float32)
    row = phase_rows["table_" + key]
    assert row["code"] == 0 and row["valid"] == D.valid[0] | D.valid[1] << 16
    n = cost.size
    tab = _f32(row["tab"]).reshape(n + 2, 4)
    cdf = np.concatenate([D.cdf, D.cdf[-1:]])        # the last node repeats cdf[n - 2]
    prev = np.concatenate([[np.float32(0)], cdf[:-1]]).astype(np.float32)
    want = np.zeros((n + 2, 4), np.float32)
    want[0] = (D.integral, D.normalization, cost[0], cost[-1])
    want[1:n + 1] = np.stack([cost, values, prev, cdf], 1)
    want[n + 1] = (np.inf, 0, D.integral, D.integral)
    assert tab.view(np.uint32).tolist() == want.view(np.uint32).tolist()


I = "IrregularContinuousDistribution: "
PHASE_FAULTS = {  # name: (cost, values, text)
    "one_entry": ([0.0], [1.0], I + "needs at least two entries!"),
    "too_many": (np.linspace(-1, 1, 65537), np.ones(65537), "more than 65536 entries"),
    "cost_nan": ([np.nan, 0, 1], [1, 1, 1], "entries must be finite"),  # (a later NaN fails the ordering check of its predecessor first)
    "value_inf": ([-1, 0, 1], [1, np.inf, 1], "entries must be finite"),
    "cost_range": ([-1, 0, 1.5], [1, 1, 1], "'cost' must lie in [-1, 1]"),
    "negative": ([-1, 0, 1], [1, -0.5, 1], I + "entries must be non-negative!"),
    "not_increasing": ([-1, 0.5, 0.5, 1], [1, 1, 1, 1], I + "node positions must be strictly increasing!"),
    "no_mass": ([-1, 0, 1], [0, 0, 0], I + "no probability mass found!"),
    "denormal_integral": ([-1, 1], [1e-44, 1e-44], "the table's integral is not a normal float"),
}


@pytest.mark.parametrize("name", sorted(PHASE_FAULTS))
def test_phase_table_rejections(phase_rows, name):
    row = phase_rows[name]
    assert (row["code"], row["msg"]) == (SC.INVALID_ARGUMENT, "fn: " + PHASE_FAULTS[name][2])


def test_assemble_phase_data(exes):
    rows = {r.pop("case"): r for r in _run(exes, "assemble")}
    api = "api: medium "
    # per medium [tab_offset, tab_n]; per blend [set, tab_offset 0, tab_n 0, tab_offset 1, tab_n 1, grid_offset,
    # the record in `all` equals the host's]
    none = [0, 0, 0, 0, 0, 0, 1]
    # medium 0's table: header + 3 nodes + sentinel = 5 records; the blend's record takes 8 behind them
    assert rows["assemble_child_missing"] == dict(
        code=0, records=13, grid_total=128, media=[[0, 3], [5, 0], [13, 0], [13, 0], [0, 0]],
        blends=[none, [1, 0, 0, 0, 0, 0, 1], none, none, none], check_code=1,
        check_msg=api + "1 has a blend phase function with a tabulated child but no table for it "
                        "(call mh_scene_set_phase_blend_table after mh_scene_set_phase_blend)")
    # the child's 2 nodes: 4 records at 13
    assert rows["assemble_child_arrived"] == dict(
        code=0, records=17, grid_total=128, media=[[0, 3], [5, 1], [17, 0], [17, 0], [0, 0]],
        blends=[none, [1, 0, 0, 13, 2, 0, 1], none, none, none], check_code=1,
        check_msg=api + "2 has a blend phase function but no blend (call mh_scene_set_phase_blend after mh_scene_create)")
    # two records of 8; the weight grids: one brick at grid_floats, two bricks behind it
    assert rows["assemble_two_grids"] == dict(
        code=0, records=33, grid_total=128 + 64 + 128, media=[[0, 3], [5, 1], [17, 1], [25, 1], [0, 0]],
        blends=[none, [1, 0, 0, 13, 2, 0, 1], [1, 0, 0, 0, 0, 128, 1], [1, 0, 0, 0, 0, 192, 1], none], check_code=1,
        check_msg=api + "4 has a tabulated phase function but no table (call mh_scene_set_phase_table after mh_scene_create)")
    # not a regrid: the grids keep their offsets
    assert rows["assemble_all_ready"] == dict(
        code=0, records=37, grid_total=128, media=[[0, 3], [5, 1], [17, 1], [25, 1], [33, 2]],
        blends=[none, [1, 0, 0, 13, 2, 0, 1], [1, 0, 0, 0, 0, 128, 1], [1, 0, 0, 0, 0, 192, 1], none], check_code=0,
        check_msg="")


BLEND = {
    "blend_ok": "", "blend_grid_ok": "",
    "blend_null": "NULL argument",
    "blend_medium_range": "medium index out of bounds",
    "blend_not_blend": "the medium's phase function is not MH_PHASE_BLEND",
    "blend_nested": "a child must be MH_PHASE_ISOTROPIC, MH_PHASE_HG, MH_PHASE_RAYLEIGH or MH_PHASE_TABULATED "
                    "(a nested blend is not supported)",
    "blend_g": "The asymmetry parameter must lie in the interval (-1, 1)!",
    "blend_rayleigh": "a rayleigh child is supported with depolarization = 0 only",
    "blend_weight": "the weight must be finite",
    "blend_partial_res": "a weight grid needs three non-zero resolutions",
    "blend_null_grid": "NULL weight grid data",
    "blend_grid_nan": "the weight grid and its transform must be finite",
    "blend_transform_nan": "the weight grid and its transform must be finite",
    "blend_grid_2_32": "weight grid above 2^32 texels",
}


def test_check_blend(exes):
    rows = {r["case"]: (r["code"], r["msg"]) for r in _run(exes, "check_blend")}
    assert rows == {k: ((1, "fn: " + t) if t else (0, "")) for k, t in BLEND.items()}


def test_source_shape():
    """The two headers are host-only, and mh_api.hip keeps no copy of what moved."""
    for name in ("mh_scene_build.hpp", "mh_records.hpp"):
        hdr = open(os.path.join(CSRC, name)).read()
        assert "hip/" not in hdr and "getenv" not in hdr and "hipStream" not in hdr and "hipError" not in hdr, name
    api = open(os.path.join(CSRC, "mh_api.hip")).read()
    for gone in ("IrregularContinuousDistribution: ", "mesh range out of bounds", "for (DevBuf *b :", "kBlendRecs"):
        assert gone not in api, gone
    i = api.index("int mh_scene_destroy(")
    destroy = api[i:api.index("\n}\n", i)]
    assert destroy.index("comm_attach") < destroy.index("hipSetDevice") < destroy.index("hipStreamSynchronize(s->stream2)") \
        < destroy.index("hipStreamDestroy") < destroy.index("delete s")
