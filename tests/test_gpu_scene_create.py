"""mh_scene_create / mh_scene_destroy through the C ABI on the device.

Every faulty description of scene_cases.py is refused with the code and text
the host check gives (tests/test_scene_host.py) -- before any device work, so
nothing faulty reaches a kernel; a refused create leaves the library able to
create and render the valid 2-shape scene exactly as a fresh process does; and
scenes that own their buffers give all device memory back."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # the fresh process of test_valid_create_after_a_refused_one
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(ROOT, "mitsuba3-nasa_amd"), os.path.join(ROOT, "tests")]

import scene_cases as SC
from mitsuba_hip import _abi as A

pytestmark = pytest.mark.gpu

W = H = 16
SPP = 4


def valid_scene():
    """scene_cases.base() under the Cornell box's camera: the light under the ceiling, the floor below"""
    import mitsuba_hip as mi
    mi.set_variant("hip_ad_rgb")
    spec = mi.cornell_box()
    spec["sensor"]["film"]["width"], spec["sensor"]["film"]["height"] = W, H
    d = SC.base()
    d.sensor = A.Sensor.from_buffer_copy(bytes(mi.load_dict(spec).desc.sensor))
    return d


def create(d):
    """(code, message, handle) of mh_scene_create on device 0"""
    L = A.lib()
    desc, keep = d.ctypes_desc()
    h = C.c_void_p()
    rc = L.mh_scene_create(C.byref(desc), 0, None, C.byref(h))
    return rc, L.mh_last_error().decode() if rc else "", h


def render_samples(h):
    integ = A.Integrator(A.INTEGRATOR_PATH, 6, 3, 0)
    out = np.zeros(5 * W * H * SPP, np.float32)
    A.check(A.lib().mh_render_samples(h, C.byref(integ), 7, SPP, 0, 0, out.ctypes.data_as(C.c_void_p), 0))
    return out


@pytest.mark.parametrize("name", sorted(SC.FAULTS) + sorted(SC.ORDER))
def test_faulty_description_is_refused(name):
    code, text = (SC.FAULTS.get(name) or SC.ORDER[name])[1:]
    rc, msg, h = create(SC.faulty(name))
    assert (rc, msg, h.value) == (code, text, None)


def test_valid_create_after_a_refused_one(tmp_path):
    L = A.lib()
    assert create(SC.faulty("face_index"))[0] == SC.INVALID_ARGUMENT
    assert create(SC.faulty("null_media"))[0] == SC.INVALID_ARGUMENT
    rc, msg, h = create(valid_scene())
    assert rc == 0, msg
    try:
        nodes, prims, depth = C.c_uint32(), C.c_uint32(), C.c_uint32()
        A.check(L.mh_scene_bvh_info(h, C.byref(nodes), C.byref(prims), C.byref(depth)))
        assert prims.value == 3  # the rectangle and two triangles
        got = render_samples(h)
    finally:
        assert L.mh_scene_destroy(h) == 0
    path = str(tmp_path / "fresh.npy")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    fresh = np.load(path)
    assert got.view(np.uint32).tolist() == fresh.view(np.uint32).tolist()
    L_rgb = got[:3 * W * H * SPP]
    assert np.isfinite(got).all() and (L_rgb > 0).any(), "the camera sees the lit floor"


def test_destroy_gives_the_memory_back():
    """create -> mh_scene_set_phase_blend -> destroy, 20 times.  The blend's weight grid is 64^3 floats (1 MiB
    bricked) and the call rebuilds the grid buffer and the phase tables aside and moves them into the scene, so a
    buffer that destroy forgot would hold 20 MiB at the end; the bound is one allocation granule of the device
    memory (2 MiB: the driver hands VRAM out in fragments of that size)."""
    import torch
    L = A.lib()
    d = valid_scene()
    d.media[0].phase, d.media[0].g = A.PHASE_BLEND, 0.0
    res = 64
    weights = np.full(res ** 3, 0.25, np.float32)
    b = A.PhaseBlend()
    b.phase[:] = [A.PHASE_HG, A.PHASE_ISOTROPIC]
    b.g[:] = [0.6, 0.0]
    b.grid_res[:] = [res] * 3
    b.grid_to_local[:] = [0.5, 0, 0, 0.5, 0, 0.5, 0, 0.5, 0, 0, 0.5, 0.5]
    b.grid_data = weights.ctypes.data_as(A.PF)

    def cycle():
        rc, msg, h = create(d)
        assert rc == 0, msg
        rc = L.mh_scene_set_phase_blend(h, 0, C.byref(b))
        msg = L.mh_last_error().decode() if rc else ""
        assert L.mh_scene_destroy(h) == 0
        assert rc == 0, msg

    cycle()  # (the first scene loads the code objects)
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info(0)[0]
    for _ in range(20):
        cycle()
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info(0)[0]
    print(f"free device memory: {before} before, {after} after 20 cycles")
    assert abs(before - after) <= 2 << 20


if __name__ == "__main__":
    rc, msg, h = create(valid_scene())
    assert rc == 0, msg
    np.save(sys.argv[1], render_samples(h))
    assert A.lib().mh_scene_destroy(h) == 0
