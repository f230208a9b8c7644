"""CPU: the blend phase function (phase/blendphase.cpp: two nested phase
functions mixed by the volume weight_0) at the loader and at the C ABI, without
a device: it loads from a dictionary and from XML with a float, a constvolume
or a gridvolume weight, what the hip_ad_rgb variant does not support is refused
with a message that names the limit, its parameters are listed, updatable and
not differentiable, and the new entry points exist with their documented
signatures and struct layout."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from blend_cases import blend, tab, weight_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mitsuba_hip.h")


def _mi():
    import mitsuba_hip as mi
    mi.set_variant("hip_ad_rgb")
    return mi


def _scene(mi, phase, **kw):
    d = mi.volume_cube(16, 16, 4, grid_res=8, scale=4.0, **kw)
    d["medium1"]["phase"] = phase
    return d


HG, ISO, RAY = {"type": "hg", "g": 0.6}, {"type": "isotropic"}, {"type": "rayleigh"}


def test_load_dict_accepts_blendphase():
    mi = _mi()
    from mitsuba_hip import _abi as A
    sc = mi.load_dict(_scene(mi, blend(RAY, tab("b"), 0.2)))
    assert sc.medium(0).phase == A.PHASE_BLEND == 4
    assert 0 not in sc.phase_tables          # the children are stored apart from the plain tabphase media's tables
    b = sc.phase_blends[0]
    assert [c["phase"] for c in b.children] == [A.PHASE_RAYLEIGH, A.PHASE_TABULATED]
    assert b.value.dtype == np.float32 and b.value == np.float32(0.2) and b.data is None
    c, v = b.children[1]["table"]
    assert c.dtype == np.float32 and v.dtype == np.float32
    np.testing.assert_array_equal(c, np.float32([-1, -0.5, 0.2, 0.9, 1]))
    np.testing.assert_array_equal(v, np.float32([0, 0.3, 0, 2, 40]))
    # declaration order, not the names: "a" after "z"
    sc = mi.load_dict(_scene(mi, {"type": "blendphase", "z": HG, "weight_0": {"type": "constvolume", "value": 0.75},
                                  "a": ISO}))
    b = sc.phase_blends[0]
    assert [c["phase"] for c in b.children] == [A.PHASE_HG, A.PHASE_ISOTROPIC]
    assert b.children[0]["g"] == float(np.float32(0.6)) and b.value == np.float32(0.75)
    # a child may carry any name but the volume's own
    sc = mi.load_dict(_scene(mi, {"type": "blendphase", "weight_air": RAY, "weight_0": 0.5, "weight_1": HG}))
    assert [c["phase"] for c in sc.phase_blends[0].children] == [A.PHASE_RAYLEIGH, A.PHASE_HG]
    # a grid of its own resolution and to_world, on a homogeneous medium too
    for kw in ({}, {"medium_type": "homogeneous"}):
        g = weight_grid(mi, (2, 3, 4))
        sc = mi.load_dict(_scene(mi, blend(ISO, HG, g), **kw))
        b = sc.phase_blends[0]
        assert b.value is None and b.data.dtype == np.float32 and b.data.shape == (4, 3, 2)
        np.testing.assert_array_equal(b.data, g["data"])
        inv = np.linalg.inv(g["to_world"].matrix)[:3, :].reshape(-1).astype(np.float32)
        np.testing.assert_array_equal(b.to_local, inv)
        rec = b.record()
        assert list(rec.grid_res) == [2, 3, 4] and list(rec.phase) == [A.PHASE_ISOTROPIC, A.PHASE_HG]
        assert rec.g[1] == np.float32(0.6)


XML = """<scene version="3.0.0">
    <integrator type="volpath"><integer name="max_depth" value="6"/></integrator>
    <sensor type="perspective">
        <transform name="to_world"><lookat origin="0, 0, 4" target="0, 0, 0" up="0, 1, 0"/></transform>
        <film type="hdrfilm"><integer name="width" value="8"/><integer name="height" value="8"/></film>
    </sensor>
    <medium type="homogeneous" id="fog">
        <float name="sigma_t" value="1"/>
        <rgb name="albedo" value="0.8"/>
        <phase type="blendphase">
            <phase type="tabphase"><string name="cost" value="-1, 0, 1"/><string name="values" value="0.5, 1, 4"/></phase>
            WEIGHT
            <phase type="hg"><float name="g" value="-0.3"/></phase>
        </phase>
    </medium>
    <shape type="cube"><bsdf type="null"/><ref name="interior" id="fog"/></shape>
    <emitter type="constant"><rgb name="radiance" value="1"/></emitter>
</scene>"""


def test_load_string_accepts_blendphase(tmp_path):
    mi = _mi()
    from mitsuba_hip import _abi as A
    sc = mi.load_string(XML.replace("WEIGHT", '<float name="weight_0" value="0.25"/>'))
    assert sc.medium(0).phase == A.PHASE_BLEND
    b = sc.phase_blends[0]
    assert [c["phase"] for c in b.children] == [A.PHASE_TABULATED, A.PHASE_HG]      # document order
    assert b.children[1]["g"] == float(np.float32(-0.3)) and b.value == np.float32(0.25)
    np.testing.assert_array_equal(b.children[0]["table"][1], np.float32([0.5, 1, 4]))
    sc = mi.load_string(XML.replace("WEIGHT", '<volume name="weight_0" type="constvolume"><float name="value" value="0.5"/></volume>'))
    assert sc.phase_blends[0].value == np.float32(0.5)
    data = np.random.default_rng(0).random((4, 3, 2, 1)).astype(np.float32)
    path = str(tmp_path / "w.vol")
    mi.VolumeGrid(data).write(path)
    sc = mi.load_string(XML.replace("WEIGHT", f'<volume name="weight_0" type="gridvolume"><string name="filename" value="{path}"/></volume>'))
    np.testing.assert_array_equal(sc.phase_blends[0].data, data[..., 0])


@pytest.mark.parametrize("phase, message", [
    ({"type": "blendphase", "weight_0": 0.5, "a": HG}, "At least two child phase functions"),
    ({"type": "blendphase", "weight_0": 0.5, "a": HG, "b": ISO, "c": RAY}, "exactly two child phase functions"),
    (blend(HG, blend(ISO, RAY, 0.5), 0.5), "nested in a blendphase is not supported"),
    (blend(HG, {"type": "rayleigh", "depolarization": 0.2}, 0.5), "depolarization = 0 only"),
    (blend(HG, ISO, {"type": "gridvolume", "data": np.zeros((2, 2, 2, 3), np.float32)}), "must have one channel"),
    (blend(HG, ISO, {"type": "gridvolume", "data": np.zeros((2, 2, 2), np.float32), "filter_type": "nearest"}),
     "filter_type='trilinear', wrap_mode='clamp'"),
    (blend(HG, ISO, {"type": "gridvolume", "data": np.zeros((2, 2, 2), np.float32), "wrap_mode": "repeat"}),
     "filter_type='trilinear', wrap_mode='clamp'"),
    ({"type": "blendphase", "a": HG, "b": ISO}, '"weight_0" has not been specified'),
    (blend({"type": "hg", "g": 1.0}, ISO, 0.5), r"interval \(-1, 1\)"),
    (blend(HG, {"type": "sggx"}, 0.5), 'plugin "sggx" is not available'),
])
def test_rejected_inputs(phase, message):
    mi = _mi()
    with pytest.raises(RuntimeError, match=message):
        mi.load_dict(_scene(mi, phase))


def test_parameters_are_listed_updatable_and_not_differentiable():
    mi = _mi()
    from mitsuba_hip import _abi as A
    sc = mi.load_dict(_scene(mi, blend(HG, {"type": "tabphase", "cost": "-1, 0, 1", "values": "0.5, 1, 4"}, 0.2)))
    params = mi.traverse(sc)
    keys = ["medium1.phase_function.weight_0.value", "medium1.phase_function.phase_0.g",
            "medium1.phase_function.phase_1.values"]
    for k in keys:
        assert k in params
        with pytest.raises(A.MitsubaHipError, match="not differentiable"):
            params.param_id(k)
    assert "medium1.sigma_t.data" in params and "medium1.albedo.value" in params
    params[keys[0]] = [0.7]       # no device handle yet: the host copies are replaced
    params[keys[1]] = [-0.4]
    params[keys[2]] = [1.0, 1.0, 2.0]
    params.update()
    b = sc.phase_blends[0]
    assert b.value == np.float32(0.7) and b.children[0]["g"] == float(np.float32(-0.4))
    np.testing.assert_array_equal(b.children[1]["table"][1], np.float32([1, 1, 2]))
    params[keys[2]] = [0.0, 0.0, 0.0]
    with pytest.raises(RuntimeError, match="no probability mass"):
        params.update()
    sc = mi.load_dict(_scene(mi, blend(HG, ISO, weight_grid(mi, (2, 3, 4)))))
    params = mi.traverse(sc)
    key = "medium1.phase_function.weight_0.data"
    assert tuple(params[key].shape) == (4, 3, 2, 1)
    with pytest.raises(A.MitsubaHipError, match="not differentiable"):
        params.param_id(key)
    new = np.random.default_rng(1).random((4, 3, 2, 1)).astype(np.float32)
    params[key] = new
    params.update()
    np.testing.assert_array_equal(sc.phase_blends[0].data, new[..., 0])


def test_c_abi_entry_points():
    from mitsuba_hip import _abi as A
    L = A.lib()
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    names = ["mh_scene_set_phase_blend", "mh_scene_set_phase_blend_table", "mh_scene_update_phase_blend_weight",
             "mh_phase_sample_at", "mh_phase_eval_at"]
    assert set(names) <= set(A.EXPORTS)
    assert L.mh_scene_set_phase_blend.argtypes == [vp, u32, C.POINTER(A.PhaseBlend)]
    assert L.mh_scene_set_phase_blend_table.argtypes == [vp, u32, u32, u32, A.PF, A.PF]
    assert L.mh_scene_update_phase_blend_weight.argtypes == [vp, u32, A.PF, u64]
    assert L.mh_phase_sample_at.argtypes == [vp, u32, u64, vp, vp, vp, vp, u32]
    assert L.mh_phase_eval_at.argtypes == [vp, u32, u64, vp, vp, vp, u32]
    for n in names:
        assert getattr(L, n).restype == C.c_int
    c = (C.c_float * 2)(-1.0, 1.0)
    v = (C.c_float * 2)(1.0, 1.0)
    rec = A.PhaseBlend()
    calls = {
        "mh_scene_set_phase_blend": lambda: L.mh_scene_set_phase_blend(None, 0, C.byref(rec)),
        "mh_scene_set_phase_blend_table": lambda: L.mh_scene_set_phase_blend_table(None, 0, 0, 2, c, v),
        "mh_scene_update_phase_blend_weight": lambda: L.mh_scene_update_phase_blend_weight(None, 0, c, 1),
        "mh_phase_sample_at": lambda: L.mh_phase_sample_at(None, 0, 0, None, None, None, None, 0),
        "mh_phase_eval_at": lambda: L.mh_phase_eval_at(None, 0, 0, None, None, None, 0),
    }
    for n, call in calls.items():
        assert call() == A.MH_ERR_INVALID_ARGUMENT, n
        assert L.mh_last_error().startswith(n.encode()), (n, L.mh_last_error())
    assert A.PHASE_BLEND == 4 and A.ABI_VERSION == 2


def test_struct_layout_matches_header():
    """mh_phase_blend in the header and _abi.PhaseBlend (test_abi.py's method)."""
    from mitsuba_hip import _abi as A
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', "int main(void) {",
             'printf("sizeof %zu\\n", sizeof(mh_phase_blend));', 'printf("MH_PHASE_BLEND %d\\n", (int)MH_PHASE_BLEND);']
    for f in A.PhaseBlend._fields_:
        lines.append(f'printf("{f[0]} %zu\\n", offsetof(mh_phase_blend, {f[0]}));')
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "layout.c")
        open(src, "w").write("\n".join(lines))
        exe = os.path.join(d, "layout")
        subprocess.run(["gcc", "-std=c11", "-o", exe, src], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    for ln in out.splitlines():
        field, val = ln.split()
        if field == "MH_PHASE_BLEND":
            got = A.PHASE_BLEND
        else:
            got = C.sizeof(A.PhaseBlend) if field == "sizeof" else getattr(A.PhaseBlend, field).offset
        assert got == int(val), (field, got, val)
