"""What the host planner (csrc/mh_plan.hpp, checked on the CPU by
test_plan_host.py) decides is what the library does, seen through mh_stats
alone: the engine as `mode`, the chunk count as `n_aux_launches` (mh_render:
one splat per chunk) and the bitmap record log as `aux_items`.  Small Cornell
box calls; every expectation also holds for the library before the planner
existed."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ENV = ("MH_WF_STREAMS", "MH_WF_CHUNK", "MH_MODE", "MH_DETERMINISTIC", "MH_PRB_BMP_WF", "MH_PRB_REPLAY")


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def _mi():
    import mitsuba_hip as mi
    if not mi.is_available():
        pytest.fail("no HIP device / native library: the GPU tests need an MI355X")
    mi.set_variant("hip_ad_rgb")
    return mi


def _box(mi, w, h):
    d = mi.cornell_box()
    d["sensor"]["film"]["width"], d["sensor"]["film"]["height"] = w, h
    return mi.load_dict(d)


def _film(mi, scene, spp, **kw):
    from mitsuba_hip import _abi as A
    st = A.Stats()
    f = mi.render_film(scene, mi.load_dict({"type": "path", "max_depth": 8}), seed=5, spp=spp, stats=st, **kw)
    return f.cpu().numpy(), st


# ---- mh_render, `path`, depth 8 ----------------------------------------------
def test_render_split_threshold():
    mi = _mi()
    s = _box(mi, 32, 32)
    _, st = _film(mi, s, 512)  # 2^19 samples in one chunk: split in two for the two streams
    assert (st.mode, st.n_aux_launches) == (2, 2)
    _, st = _film(mi, s, 256)
    assert (st.mode, st.n_aux_launches) == (2, 1)


def test_render_megakernel_flag():
    mi = _mi()
    _, st = _film(mi, _box(mi, 32, 32), 256, mode="mega")
    assert (st.mode, st.n_aux_launches) == (0, 1)


def test_render_chunk_env_and_one_stream(monkeypatch):
    mi = _mi()
    s = _box(mi, 16, 16)
    monkeypatch.setenv("MH_WF_CHUNK", "1024")  # 1024 samples per chunk: 128 of the 256 pixels at 8 spp
    f2, st2 = _film(mi, s, 8)
    d2, sd2 = _film(mi, s, 8, deterministic=True)
    monkeypatch.setenv("MH_WF_STREAMS", "1")
    f1, st1 = _film(mi, s, 8)
    d1, sd1 = _film(mi, s, 8, deterministic=True)
    assert [x.n_aux_launches for x in (st2, sd2, st1, sd1)] == [2, 2, 2, 2]
    assert [x.mode for x in (st2, sd2, st1, sd1)] == [2, 2, 2, 2]
    assert st2.rays_closest == st1.rays_closest
    assert np.array_equal(d2, d1)  # the fixed-order splat: the same bits
    np.testing.assert_allclose(f2, f1, rtol=2e-5, atol=1e-6)  # float atomics: summation order only
    np.testing.assert_allclose(d2, f1, rtol=2e-5, atol=1e-6)


# ---- mh_render_backward, `prb`, 16 x 16 @ 8 -----------------------------------
def test_backward_engines_agree(monkeypatch):
    mi = _mi()
    import torch
    from mitsuba_hip import _abi as A
    prb = mi.load_dict({"type": "prb", "max_depth": 8})
    gi = torch.from_numpy(np.random.default_rng(1).random((16, 16, 3)).astype(np.float32) / (16 * 16 * 3)).cuda()

    def run(scene, key):
        st = A.Stats()
        (g,) = mi.render_backward(scene, mi.traverse(scene), gi, [key], prb, seed=11, spp=8, stats=st)
        return g.cpu().numpy(), st

    g_rgb, st_rgb = run(_box(mi, 16, 16), "white.reflectance.value")
    bmp = mi.load_dict(mi.cornell_box_bitmap(tex_res=8, width=16, height=16, spp=8))
    g_wf, st_wf = run(bmp, "white.reflectance.data")
    monkeypatch.setenv("MH_PRB_BMP_WF", "0")
    g_rp, st_rp = run(bmp, "white.reflectance.data")
    # rgb: fused wavefront, no record log; bitmap: wavefront + texel scatter; MH_PRB_BMP_WF=0: replay kernel
    assert (st_rgb.mode, st_wf.mode, st_rp.mode) == (1, 1, 0)
    assert st_rgb.aux_items == 0 and st_rp.aux_items == 0 and st_wf.aux_items > 0
    assert (st_rgb.n_aux_launches, st_wf.n_aux_launches, st_rp.n_aux_launches) == (0, 1, 0)
    scale = np.abs(g_rp).max()
    assert scale > 0
    np.testing.assert_allclose(g_wf, g_rp, rtol=2e-3, atol=1e-9 + 2e-4 * scale)
    # the bitmap holds the rgb constant in every texel and its bilinear weights
    # sum to one: the constant's gradient is the sum of the texels'
    for g in (g_wf, g_rp):
        np.testing.assert_allclose(g.reshape(-1, 3).sum(0), g_rgb.reshape(3), rtol=2e-3)


# ---- mh_render_forward, `prb` --------------------------------------------------
@pytest.mark.parametrize("mega", [False, True])
def test_forward_mode(mega):
    mi = _mi()
    import torch
    from mitsuba_hip import _abi as A
    s = _box(mi, 16, 16)
    params = mi.traverse(s)
    ic = mi.load_dict({"type": "prb", "max_depth": 8}).c()
    h = s.handle(0, torch.cuda.current_stream(0).cuda_stream)
    tan = torch.ones(params["white.reflectance.value"].shape, dtype=torch.float32, device="cuda:0").contiguous()
    ids = (C.c_uint32 * 1)(params.param_id("white.reflectance.value"))
    ptrs = (C.c_void_p * 1)(tan.data_ptr())
    film = torch.zeros((16, 16, A.film_channels(s.desc.sensor.pixel_format)), dtype=torch.float32, device="cuda:0")
    st = A.Stats()
    flags = A.FLAG_DEVICE_POINTERS | (A.FLAG_MEGAKERNEL if mega else 0)
    A.check(A.lib().mh_render_forward(h, C.byref(ic), 3, 8, 0, 0, 1, ids, ptrs, C.c_void_p(film.data_ptr()), flags,
                                      C.byref(st)))
    assert st.mode == (0 if mega else 2)
    assert float(film[..., :3].abs().max()) > 0
