"""CPU: emitter radiance as a scene parameter on the host side -- traverse()
lists the reference's keys ('<shape>.emitter.radiance.value',
'<name>.radiance.value', '<name>.irradiance.value'), update() writes the
scene description, the parameter id is MH_PARAM_EMITTER_RADIANCE | index, and
the native library exports mh_scene_update_emitter.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mitsuba_hip.h")

KEYS = {"light.emitter.radiance.value": [18.387, 13.9873, 6.75357],
        "sky.radiance.value": [0.3, 0.4, 0.5],
        "sun.irradiance.value": [2.0, 2.0, 2.0]}


@pytest.fixture(scope="module")
def mi():
    import mitsuba_hip as mi
    mi.set_variant("hip_ad_rgb")
    return mi


def _scene(mi):
    d = mi.cornell_box()
    d["sky"] = {"type": "constant", "radiance": {"type": "rgb", "value": [0.3, 0.4, 0.5]}}
    d["sun"] = {"type": "directional", "direction": [0.2, -0.5, -1.0], "irradiance": {"type": "rgb", "value": 2.0}}
    return mi.load_dict(d)


def test_traverse_lists_emitter_keys(mi):
    scene = _scene(mi)
    params = mi.traverse(scene)
    for k, v in KEYS.items():
        assert k in params, k
        assert tuple(params[k].shape) == (3,)
        assert np.allclose(params[k].numpy(), v, atol=1e-5), k
    # one parameter per emitter, each naming its own emitter
    idx = sorted(scene.params[k][1] for k in KEYS)
    assert idx == list(range(scene.desc.n_emitters)) == [0, 1, 2]


def test_param_id_is_kind_tag_or_index(mi):
    from mitsuba_hip import _abi as A
    scene = _scene(mi)
    params = mi.traverse(scene)
    for k in KEYS:
        kind, i = scene.params[k]
        assert kind == "emitter_radiance"
        assert params.param_id(k) == 0x30000000 | i
        assert params.param_id(k) & A.PARAM_KIND_MASK == A.PARAM_EMITTER_RADIANCE
    # the other kinds keep their ids
    assert params.param_id("white.reflectance.value") == scene.params["white.reflectance.value"][1]


def test_update_without_device_writes_the_description(mi):
    scene = _scene(mi)
    params = mi.traverse(scene)
    new = {"light.emitter.radiance.value": [0.0, 0.5, 0.0], "sky.radiance.value": [1.0, 2.0, 3.0],
           "sun.irradiance.value": [0.25, 0.5, 0.75]}
    for k, v in new.items():
        params[k] = v
    params.update()
    assert not scene._handles   # no device copy was created
    for k, v in new.items():
        i = scene.params[k][1]
        assert list(scene.desc.emitters[i].radiance) == pytest.approx(v), k
        assert list(scene.emitter(i).radiance) == pytest.approx(v), k
    # untouched fields of the emitter stay
    sun = scene.desc.emitters[scene.params["sun.irradiance.value"][1]]
    d = np.array([0.2, -0.5, -1.0]) / np.linalg.norm([0.2, -0.5, -1.0])
    assert np.allclose(list(sun.direction), d, atol=1e-6)


def test_abi_constant_matches_header():
    from mitsuba_hip import _abi as A
    m = re.search(r"#define\s+MH_PARAM_EMITTER_RADIANCE\s+(0x[0-9a-fA-F]+)u", open(HEADER).read())
    assert m, "MH_PARAM_EMITTER_RADIANCE is not defined in the header"
    assert int(m.group(1), 16) == A.PARAM_EMITTER_RADIANCE == 0x30000000
    # the ABI version is unchanged: the new kind and entry point are additions
    assert re.search(r"#define MH_ABI_VERSION 2u", open(HEADER).read())


def test_library_exports_update_emitter():
    from mitsuba_hip import _abi as A
    assert "mh_scene_update_emitter" in A.EXPORTS
    L = A.lib()
    assert hasattr(L, "mh_scene_update_emitter")
    assert L.mh_scene_update_emitter.argtypes == [C.c_void_p, C.c_uint32, A.PF]
    # NULL scene: the documented argument error, no device needed
    v = (C.c_float * 3)(1.0, 1.0, 1.0)
    assert L.mh_scene_update_emitter(None, 0, v) == A.MH_ERR_INVALID_ARGUMENT
    assert b"mh_scene_update_emitter" in L.mh_last_error()
