"""The two-bounce generating launch of the fused wavefront (k_wf_bounce<Gen, Two>,
DESIGN.md §3): the camera bounce and the bounce after it in one launch, a
survivor's state parked in the wave's LDS slab in between.

Every comparison is between a call that variant::bounce_path sends to the
two-bounce instance (a fused packet scene, max_depth >= 2, the Cornell box's
13.9 KB of LDS; tests/test_fuse01_host.py pins the rule) and one it does not
send there: the trace / shade / shadow kernels of MH_WF_FUSED=0, max_depth 1,
or the per-lane megakernel (a multi-pass render has no unfused wavefront).
The oracle is the third party.

Criteria: positions identical; L identical, for every sample, to the unfused
wavefront's and to the oracle's (none of these scenes has one of the BVH-vs-
brute-force ties of DESIGN.md §4); rays_closest / rays_shadow equal.  The
developed film: test_gpu_shade_records.py's film tolerance.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_py as O

pytestmark = pytest.mark.gpu

SEED = 3


def _mi():
    import mitsuba_hip as mi
    if not mi.is_available():
        pytest.fail("no HIP device / native library: the GPU tests need an MI355X")
    mi.set_variant("hip_ad_rgb")
    return mi


def _dict(mi, w, h, spp, kind="cbox", fmt=None, box=False):
    d = mi.cornell_box()
    film = d["sensor"]["film"]
    film["width"], film["height"] = w, h
    d["sensor"]["sampler"]["sample_count"] = spp
    if kind == "sky":  # no back wall, a sky behind it: the film's middle sees no surface
        d.pop("back")
        d["sky"] = {"type": "constant", "radiance": {"type": "rgb", "value": [0.3, 0.4, 0.5]}}
    if fmt:
        film["pixel_format"] = fmt
    if box:
        film["rfilter"] = {"type": "box"}
    return d


def _samples(scene, integ, flags=None):
    """(L, pos, alpha): mh_render_samples' planes, alpha only for a film that has it"""
    from mitsuba_hip import _abi as A
    spp = scene.sample_count()
    n = scene.width * scene.height * spp
    alpha = A.pixel_has_alpha(scene.desc.sensor.pixel_format)
    out = np.full((6 if alpha else 5) * n, np.nan, np.float32)
    ic = integ.c()
    A.check(A.lib().mh_render_samples(scene.handle(0), C.byref(ic), SEED, spp, 0, 0, out.ctypes.data_as(C.c_void_p),
                                      A.FLAG_WAVEFRONT if flags is None else flags))
    p = out.reshape(-1, n)
    return p[:3].T.copy(), p[3:5].T.copy(), (p[5].copy() if alpha else None)


def _film(mi, scene, integ, mode="wavefront", **kw):
    from mitsuba_hip import _abi as A
    st = A.Stats()
    film = mi.render_film(scene, integ, seed=SEED, stats=st, mode=mode, **kw).cpu().numpy()
    return film, st


def _check(mi, monkeypatch, d, what, **integ_kw):
    """fused (two-bounce launch) vs unfused vs oracle on one scene; returns the fused planes and the oracle's"""
    scene = mi.load_dict(d)
    integ = mi.load_dict({"type": "path", **integ_kw})
    spp = scene.sample_count()
    L, pos, alpha = _samples(scene, integ)
    film, st = _film(mi, scene, integ)
    assert st.mode == 2  # the fused wavefront
    assert st.n_trace_launches % integ_kw["max_depth"] == 0 and st.n_trace_launches > 0  # bounces, not launches
    rL, rpos, rvalid = O.sample_range(scene, integ, SEED, spp, 0, L.shape[0])
    monkeypatch.setenv("MH_WF_FUSED", "0")
    uscene = mi.load_dict(d)
    U, upos, ualpha = _samples(uscene, integ)
    ufilm, ust = _film(mi, uscene, integ)
    monkeypatch.delenv("MH_WF_FUSED")
    assert ust.mode == 1  # trace / shade / shadow kernels
    exact = np.all(L == rL, axis=1)
    print(f"{what}: {L.shape[0]} samples, bit-exact vs the oracle {exact.mean():.6f}, vs unfused "
          f"{np.all(L == U, axis=1).mean():.6f}; rays {st.rays_closest} / {st.rays_shadow} "
          f"(unfused {ust.rays_closest} / {ust.rays_shadow}); mean L {rL.mean():.4f}")
    assert not np.isnan(L).any() and not np.isnan(pos).any()
    np.testing.assert_array_equal(pos, rpos)
    np.testing.assert_array_equal(pos, upos)
    np.testing.assert_array_equal(L, U)
    np.testing.assert_array_equal(L, rL)
    assert rL.mean() > 0
    assert (st.rays_closest, st.rays_shadow) == (ust.rays_closest, ust.rays_shadow)
    assert st.samples == ust.samples == L.shape[0]
    if alpha is not None:
        np.testing.assert_array_equal(alpha, ualpha)
        np.testing.assert_array_equal(alpha, rvalid.astype(np.float32))
    return L, alpha, rL, rvalid, film, st


@pytest.mark.parametrize("max_depth", [2, 3, 8])
def test_cbox_samples(max_depth, monkeypatch):
    """16 x 16 @ 64: four pixels per queue segment, a wave per pixel.  max_depth 2: bounce 1 is the last
    (nothing survives the launch); 3: the launch's survivors feed one more launch; 8: the bench's depth."""
    mi = _mi()
    _check(mi, monkeypatch, _dict(mi, 16, 16, 64), f"cbox depth {max_depth}", max_depth=max_depth)


def test_ragged_last_wave(monkeypatch):
    """7 x 5 @ 3: 105 paths over 64 segments of 2 (the last ones short or empty): every wave is ragged."""
    mi = _mi()
    _check(mi, monkeypatch, _dict(mi, 7, 5, 3), "7x5@3", max_depth=8)


def test_wave_reuses_its_slab(monkeypatch):
    """MH_WF_BPC=1: 256 workgroups, 16 waves (1,024 paths) per iteration and segment; 40 x 40 @ 64 is 1,600
    paths per segment, so every wave runs a second, partly filled iteration over the same slab."""
    mi = _mi()
    monkeypatch.setenv("MH_WF_BPC", "1")
    _check(mi, monkeypatch, _dict(mi, 40, 40, 64), "bpc 1", max_depth=3)


def test_max_depth_1_falls_back(monkeypatch):
    """max_depth 1: one bounce, so the rule keeps the one-bounce generating launch"""
    mi = _mi()
    _, _, rL, _, _, st = _check(mi, monkeypatch, _dict(mi, 16, 16, 64), "cbox depth 1", max_depth=1)
    assert st.rays_shadow == 0 and st.rays_closest == st.samples  # the camera rays alone


def test_roulette_at_bounce_0(monkeypatch):
    """rr_depth 1: the roulette ends paths at the camera bounce, so the second trip runs with holes"""
    mi = _mi()
    d = _dict(mi, 16, 16, 64)
    _check(mi, monkeypatch, d, "rr_depth 1", max_depth=8, rr_depth=1)
    scene = mi.load_dict(d)
    # not vacuous: at max_depth 2 the closest-hit rays beyond the camera rays are bounce 1's; the
    # roulette ends some of them, not all
    a = _film(mi, scene, mi.load_dict({"type": "path", "max_depth": 2, "rr_depth": 1}))[1]
    b = _film(mi, scene, mi.load_dict({"type": "path", "max_depth": 2, "rr_depth": 5}))[1]
    assert 0 < a.rays_closest - a.samples < b.rays_closest - b.samples


@pytest.mark.parametrize("hide", [True, False])
def test_film_partly_sees_nothing(hide, monkeypatch):
    """No back wall (rgba film): a pixel in the film's middle sees only the sky, so its wave has no
    survivor at all and skips the second trip; pixels at the wall's edge mix both; alpha plane included."""
    mi = _mi()
    L, alpha, rL, rvalid, _, _ = _check(mi, monkeypatch, _dict(mi, 16, 16, 64, kind="sky", fmt="rgba"),
                                        f"sky hide={hide}", max_depth=8, hide_emitters=hide)
    if hide:
        miss = (alpha == 0).reshape(256, 64)  # escaped with the environment hidden
        assert miss.all(1).any(), "a wave without survivors"
        assert (miss.any(1) & ~miss.all(1)).any(), "a wave with holes"
        assert (L[alpha == 0] == 0).all()
    else:
        assert (alpha == 1).all()  # the sky counts as valid
        sky = np.all(L == np.array([0.3, 0.4, 0.5], np.float32), axis=1).reshape(256, 64)  # ended at the camera bounce
        assert sky.all(1).any(), "a wave without survivors"
        assert (sky.any(1) & ~sky.all(1)).any(), "a wave with holes"


def test_rgba_alpha_plane(monkeypatch):
    """the closed box with an rgba film: alpha 1 everywhere, written by the first trip only"""
    mi = _mi()
    _, alpha, _, _, film, _ = _check(mi, monkeypatch, _dict(mi, 16, 16, 64, fmt="rgba"), "rgba", max_depth=8)
    assert film.shape[-1] == 5 and alpha is not None


def test_film_sums(monkeypatch):
    """The developed film of a fused call against the per-pixel sums of the unfused wavefront's samples
    (box filter: a sample lands in its own pixel with weight 1)."""
    mi = _mi()
    d = _dict(mi, 16, 16, 64, box=True)
    scene = mi.load_dict(d)
    integ = mi.load_dict({"type": "path", "max_depth": 8})
    film, st = _film(mi, scene, integ)
    img = mi.develop(scene, mi.render_film(scene, integ, seed=SEED, mode="wavefront")).cpu().numpy()
    monkeypatch.setenv("MH_WF_FUSED", "0")
    U, upos, _ = _samples(mi.load_dict(d), integ)
    monkeypatch.delenv("MH_WF_FUSED")
    px = np.floor(upos).astype(np.int64)
    assert (px[:, 0] + 16 * px[:, 1] == np.repeat(np.arange(256), 64)).all()  # pixel-major, own pixel
    ref = U.astype(np.float64).reshape(16, 16, 64, 3).mean(2)
    assert img.shape == ref.shape and np.abs(ref).max() > 0
    np.testing.assert_allclose(film[..., 3], 64.0)
    dlt = np.abs(img - ref)
    ok = dlt <= 1e-4 + 2e-3 * np.abs(ref)
    print(f"film sums: {(~ok).sum()} of {ok.size} channels off, max {dlt.max():.3e}")
    assert ok.mean() >= 0.995, f"{(~ok).sum()} of {ok.size} channels off, max {dlt.max():.3e}"
    assert dlt.mean() / np.abs(ref).mean() < 1e-3


def test_two_passes():
    """8 x 8 @ 2^26 spp is 2^32 samples: two passes of 2^25 spp (config 5's carry path); lanes [4, 6) of
    every pass-pixel.  Pass 2 generates from the PCG32 state a lane left in `carry`, which a path writes
    in whichever trip it ends.  Against the megakernel (every pass of a lane in one thread) and the oracle."""
    mi = _mi()
    spp = 1 << 26
    scene = mi.load_dict(_dict(mi, 8, 8, spp))
    integ = mi.load_dict({"type": "path", "max_depth": 8})
    wf, st = _film(mi, scene, integ, spp=spp, spp_begin=4, spp_end=6)
    assert st.mode == 2 and st.samples == 8 * 8 * 2 * 2
    assert st.n_trace_launches % (2 * 8) == 0  # chunks x two passes x eight bounces
    mega, sm = _film(mi, scene, integ, mode="mega", spp=spp, spp_begin=4, spp_end=6)
    ref = O.render(scene, integ, seed=SEED, spp=spp, spp_begin=4, spp_end=6)
    assert ref[..., 3].sum() > 0 and (st.rays_closest, st.rays_shadow) == (sm.rays_closest, sm.rays_shadow)
    for other, name in ((mega, "megakernel"), (ref, "oracle")):
        ok = np.all(np.abs(wf - other) <= 1e-4 * np.maximum(1.0, np.abs(other)), axis=-1)
        print(f"two passes vs {name}: {ok.mean():.4f} of the pixels within 1e-4, max |d| {np.abs(wf - other).max():.3e}")
        assert ok.mean() >= 0.995, name
    # the second pass is not the first again: one pass of the same lanes gives another film
    one, _ = _film(mi, mi.load_dict(_dict(mi, 8, 8, 1 << 25)), integ, spp=1 << 25, spp_begin=4, spp_end=6)
    assert not np.allclose(2 * one[..., :3], wf[..., :3], rtol=1e-3)
