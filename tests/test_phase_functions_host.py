"""CPU: the tabulated (phase/tabphase.cpp) and Rayleigh (phase/rayleigh.cpp)
phase functions at the loader and at the C ABI, without a device: both
plugins load from a dictionary and from XML, the inputs the reference's
IrregularContinuousDistribution rejects are rejected with its messages, and
the three new entry points exist with their documented signatures."""
import ctypes as C

import numpy as np
import pytest


def _mi():
    import mitsuba_hip as mi
    mi.set_variant("hip_ad_rgb")
    return mi


def _scene(mi, phase):
    d = mi.volume_cube(16, 16, 4, grid_res=8, scale=4.0)
    d["medium1"]["phase"] = phase
    return d


def test_load_dict_accepts_tabphase_and_rayleigh():
    mi = _mi()
    from mitsuba_hip import _abi as A
    sc = mi.load_dict(_scene(mi, {"type": "tabphase", "cost": "-1, -0.5 0.2,0.9, 1", "values": "0, 0.3, 0, 2, 40"}))
    assert sc.medium(0).phase == A.PHASE_TABULATED == 3
    c, v = sc.phase_tables[0]
    assert c.dtype == np.float32 and v.dtype == np.float32
    np.testing.assert_array_equal(c, np.float32([-1, -0.5, 0.2, 0.9, 1]))
    np.testing.assert_array_equal(v, np.float32([0, 0.3, 0, 2, 40]))
    sc = mi.load_dict(_scene(mi, {"type": "tabphase", "cost": np.linspace(-1, 1, 7), "values": np.ones(7)}))
    assert sc.phase_tables[0][0].size == 7
    sc = mi.load_dict(_scene(mi, {"type": "rayleigh", "depolarization": 0}))
    assert sc.medium(0).phase == A.PHASE_RAYLEIGH == 2 and sc.medium(0).g == 0.0
    assert mi.load_dict(_scene(mi, {"type": "rayleigh"})).medium(0).phase == A.PHASE_RAYLEIGH


XML = """<scene version="3.0.0">
    <integrator type="volpath"><integer name="max_depth" value="6"/></integrator>
    <sensor type="perspective">
        <transform name="to_world"><lookat origin="0, 0, 4" target="0, 0, 0" up="0, 1, 0"/></transform>
        <film type="hdrfilm"><integer name="width" value="8"/><integer name="height" value="8"/></film>
    </sensor>
    <medium type="homogeneous" id="fog">
        <float name="sigma_t" value="1"/>
        <rgb name="albedo" value="0.8"/>
        PHASE
    </medium>
    <shape type="cube"><bsdf type="null"/><ref name="interior" id="fog"/></shape>
    <emitter type="constant"><rgb name="radiance" value="1"/></emitter>
</scene>"""


def test_load_string_accepts_tabphase_and_rayleigh():
    mi = _mi()
    from mitsuba_hip import _abi as A
    sc = mi.load_string(XML.replace("PHASE", '<phase type="tabphase"><string name="cost" value="-1, 0, 1"/>'
                                             '<string name="values" value="0.5, 1, 4"/></phase>'))
    assert sc.medium(0).phase == A.PHASE_TABULATED
    np.testing.assert_array_equal(sc.phase_tables[0][0], np.float32([-1, 0, 1]))
    np.testing.assert_array_equal(sc.phase_tables[0][1], np.float32([0.5, 1, 4]))
    sc = mi.load_string(XML.replace("PHASE", '<phase type="rayleigh"><float name="depolarization" value="0"/></phase>'))
    assert sc.medium(0).phase == A.PHASE_RAYLEIGH


@pytest.mark.parametrize("phase, message", [
    ({"type": "tabphase", "cost": "-1, 0, 1", "values": "1, 1"}, "must have the same size"),
    ({"type": "tabphase", "cost": "-1, 0.5, 0.5, 1", "values": "1, 1, 1, 1"}, "strictly increasing"),
    ({"type": "tabphase", "cost": "-1, 0.5, 0.2, 1", "values": "1, 1, 1, 1"}, "strictly increasing"),
    ({"type": "tabphase", "cost": "-1, 0, 1", "values": "1, -0.1, 1"}, "non-negative"),
    ({"type": "tabphase", "cost": "-1, 0, 1", "values": "0, 0, 0"}, "no probability mass"),
    ({"type": "tabphase", "cost": "-1, 0, 1.5", "values": "1, 1, 1"}, r"\[-1, 1\]"),
    ({"type": "tabphase", "cost": "-1", "values": "1"}, "at least two entries"),
    ({"type": "rayleigh", "depolarization": 0.1}, "depolarization = 0 only.*sampling weight is not 1"),
])
def test_rejected_inputs(phase, message):
    mi = _mi()
    with pytest.raises(RuntimeError, match=message):
        mi.load_dict(_scene(mi, phase))


def test_values_parameter_is_listed_and_not_differentiable():
    mi = _mi()
    from mitsuba_hip import _abi as A
    sc = mi.load_dict(_scene(mi, {"type": "tabphase", "cost": "-1, 0, 1", "values": "0.5, 1, 4"}))
    params = mi.traverse(sc)
    key = "medium1.phase_function.values"
    assert key in params and tuple(params[key].shape) == (3,)
    with pytest.raises(A.MitsubaHipError, match="not differentiable"):
        params.param_id(key)
    params[key] = [1.0, 1.0, 2.0]     # no device handle yet: the host copy is replaced
    params.update()
    np.testing.assert_array_equal(sc.phase_tables[0][1], np.float32([1, 1, 2]))
    params[key] = [0.0, 0.0, 0.0]
    with pytest.raises(RuntimeError, match="no probability mass"):
        params.update()


def test_c_abi_entry_points():
    from mitsuba_hip import _abi as A
    L = A.lib()
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    assert {"mh_scene_set_phase_table", "mh_phase_sample", "mh_phase_eval"} <= set(A.EXPORTS)
    assert L.mh_scene_set_phase_table.argtypes == [vp, u32, u32, A.PF, A.PF]
    assert L.mh_phase_sample.argtypes == [vp, u32, u64, vp, vp, vp, u32]
    assert L.mh_phase_eval.argtypes == [vp, u32, u64, vp, vp, u32]
    for f in (L.mh_scene_set_phase_table, L.mh_phase_sample, L.mh_phase_eval):
        assert f.restype == C.c_int
    c = (C.c_float * 2)(-1.0, 1.0)
    v = (C.c_float * 2)(1.0, 1.0)
    assert L.mh_scene_set_phase_table(None, 0, 2, c, v) == A.MH_ERR_INVALID_ARGUMENT
    assert b"mh_scene_set_phase_table" in L.mh_last_error()
    assert L.mh_phase_sample(None, 0, 0, None, None, None, 0) == A.MH_ERR_INVALID_ARGUMENT
    assert b"mh_phase_sample" in L.mh_last_error()
    assert L.mh_phase_eval(None, 0, 0, None, None, 0) == A.MH_ERR_INVALID_ARGUMENT
    assert b"mh_phase_eval" in L.mh_last_error()
    assert (A.PHASE_ISOTROPIC, A.PHASE_HG, A.PHASE_RAYLEIGH, A.PHASE_TABULATED) == (0, 1, 2, 3)


def test_phase_table_lds_rule(tmp_path):
    """plan::phase_lds_bytes at its boundary (tools/plan_check.cpp, host C++):
    a table is staged when it fills a workgroup's 64 KiB exactly beside the
    launch's other LDS, and stays in global memory one byte over."""
    import json
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path / "plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(root, "tools", "plan_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout
    rows = {r["case"]: r for r in map(json.loads, out.splitlines())}
    assert rows["phase_lds"] == dict(case="phase_lds", fits_exactly=28848, one_over=0, no_table=0, alone=65536,
                                     alone_over=0, huge_other=0)
