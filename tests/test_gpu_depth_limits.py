"""GPU: the four integrators at the edges of max_depth and rr_depth, against
the CPU oracle, on the scenes of depth_cases.py (a closed room of
reflectances near one; a dense homogeneous cube) in which the depth limit
and the roulette decide what a sample returns.  test_depth_oracle.py pins the
oracle itself and shows that the boundary cases here are not vacuous (about
80 % of the room's samples change at each of 31 -> 32, 32 -> 33, 63 -> 64 and
64 -> 65; 2.7-3.0 % of the dense cube's at 1023 -> 1024 and 1024 -> 1025).

Depths at which another engine runs (mh_plan.hpp, tests/test_plan_host.py):
  path        the wavefront for 1 <= max_depth <= 64, else the per-lane kernel
  prb         backward / forward on the fused wavefront for 1 <= max_depth <=
              64; bitmap gradients on it up to 32, the replay kernel above
  volpath     the phase scheduler / the rounds for max_depth <= 1024
  prbvolpath  the phase scheduler for max_depth <= 1024
MH_FLAG_WAVEFRONT on a depth the wavefront cannot take is refused
(MH_ERR_UNSUPPORTED); the default call runs the per-lane kernel.

Criteria, the project's own (test_gpu_parity.py): positions
identical; L bit-identical for >= 99.9 % of the samples and within 1e-4 *
max(1, |L|) for >= 99.9 %; film within 1e-4 * max(1, |ref|) for >= 99.5 % of
the pixels; prb gradients rtol 1e-3; bitmap texels and prbvolpath gradients
rtol 2e-3 with an absolute floor of 2e-4 of the largest entry.
"""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import depth_cases as DC
import oracle_py as O

pytestmark = pytest.mark.gpu

SEED = 3
UNBOUNDED = 0xFFFFFFFF


def _mi():
    import mitsuba_hip as mi
    if not mi.is_available():
        pytest.fail("no HIP device / native library: the GPU tests need an MI355X")
    mi.set_variant("hip_ad_rgb")
    return mi


def _depth(max_depth):
    return UNBOUNDED if max_depth == -1 else max_depth


def _path_wavefront_ok(max_depth):
    return 1 <= _depth(max_depth) <= 64


def _vol_wavefront_ok(max_depth):
    return _depth(max_depth) <= 1024


# ---------------------------------------------------------------------------
# scenes and oracle results: built once, shared, read-only
# ---------------------------------------------------------------------------
def _open_box(mi, w=24, h=20, spp=8):
    """The open Cornell box: camera rays at the film's border miss it."""
    d = mi.cornell_box()
    d["sensor"]["film"]["width"], d["sensor"]["film"]["height"] = w, h
    d["sensor"]["sampler"]["sample_count"] = spp
    return d


def _sky_box(mi):
    """test_hide_emitters_path_parity's scene: no back wall, a sky behind it."""
    d = _open_box(mi)
    d.pop("back")
    d["sky"] = {"type": "constant", "radiance": {"type": "rgb", "value": [0.3, 0.4, 0.5]}}
    return d


@functools.lru_cache(maxsize=None)
def _scene(name, fmt=None):
    mi = _mi()
    if name == "room":
        d = DC.room(mi)
    elif name == "room_bitmap":
        d = DC.room(mi, bitmap=(5, 7, 3))
    elif name == "open_box":
        d = _open_box(mi)
    elif name == "sky_box":
        d = _sky_box(mi)
    else:
        kind, itype = name.split(":")
        kw = {"dense": {}, "dense20": {"scale": 20.0, "albedo": 0.99},
              "dense_small": {"w": 8, "h": 8, "spp": 4, "albedo": 0.99}}[kind]
        d = DC.dense(mi, itype, **kw)
    if fmt:
        d["sensor"]["film"]["pixel_format"] = fmt
    return mi.load_dict(d)


def _fresh_scene(name):
    """A scene of its own for a test that changes the engine through the
    environment: its device handle is created under that environment."""
    return _scene.__wrapped__(name)


def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _ref_samples(name, fmt, itype, max_depth, rr_depth, hide=False):
    scene = _scene(name, fmt)
    integ = DC.integrator(_mi(), itype, max_depth, rr_depth, hide_emitters=hide)
    spp = scene.sample_count()
    return _frozen(O.sample_range(scene, integ, SEED, spp, 0, scene.width * scene.height * spp))


@functools.lru_cache(maxsize=None)
def _ref_film(name, fmt, itype, max_depth, rr_depth):
    scene = _scene(name, fmt)
    return _frozen([O.render(scene, DC.integrator(_mi(), itype, max_depth, rr_depth), SEED, scene.sample_count())])[0]


def _gpu_samples(scene, integ, flags=0):
    """(rc, L, pos, valid): mh_render_samples' planes; valid only for a film with alpha."""
    from mitsuba_hip import _abi as A
    spp = scene.sample_count()
    n = scene.width * scene.height * spp
    alpha = A.pixel_has_alpha(scene.desc.sensor.pixel_format)
    out = np.full((6 if alpha else 5) * n, np.nan, np.float32)
    ic = integ.c()
    rc = A.lib().mh_render_samples(scene.handle(0), C.byref(ic), SEED, spp, 0, 0, out.ctypes.data_as(C.c_void_p), flags)
    p = out.reshape(-1, n)
    return rc, p[:3].T, p[3:5].T, (p[5] if alpha else None)


def _assert_unsupported(rc):
    from mitsuba_hip import _abi as A
    assert rc == A.MH_ERR_UNSUPPORTED, rc
    assert "wavefront" in A.lib().mh_last_error().decode()


def _assert_samples(L, pos, ref, what=""):
    rL, rpos, _ = ref
    np.testing.assert_array_equal(pos, rpos)
    exact = np.all(L == rL, axis=1)
    close = np.all(np.abs(L - rL) <= 1e-4 * np.maximum(1, np.abs(rL)), axis=1)
    print(f"{what}: bit-exact {exact.mean():.5f}, close {close.mean():.5f}, mean L {rL.mean():.4f}")
    assert exact.mean() >= 0.999, f"bit-exact fraction {exact.mean()}"
    assert close.mean() >= 0.999, f"close fraction {close.mean()}"


def _film_close(a, b, frac=0.995):
    ok = np.all(np.abs(a - b) <= 1e-4 * np.maximum(1.0, np.abs(b)), axis=-1)
    assert ok.mean() >= frac, f"film parity {ok.mean()}"


# ---------------------------------------------------------------------------
# per-sample primal: path and prb on the room
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("max_depth,rr_depth", DC.GRID_PATH)
@pytest.mark.parametrize("itype,engine", [("path", "mega"), ("path", "wavefront"), ("path", "wavefront-lane"),
                                          ("path", "wavefront-unfused"), ("prb", "mega")])
def test_room_per_sample(itype, engine, max_depth, rr_depth, monkeypatch):
    """mega: k_render; wavefront: the fused bounce kernel; -lane / -unfused:
    trace / shade / shadow kernels with the per-lane / the packet engine.  At
    (32 | 33 | 64 | 65, 1000) every path runs to max_depth; at (-1, 1) and
    (-1, 5) the roulette alone ends it, at the 0.95 clamp for many vertices;
    (8, 9) never starts the roulette, (8, 1) and (3, 1) start it at once."""
    from mitsuba_hip import _abi as A
    if engine == "wavefront-lane":
        monkeypatch.setenv("MH_TRAVERSAL", "lane")
    if engine == "wavefront-unfused":
        monkeypatch.setenv("MH_WF_FUSED", "0")
    mi = _mi()
    scene = _scene("room") if engine in ("mega", "wavefront") else _fresh_scene("room")
    integ = DC.integrator(mi, itype, max_depth, rr_depth)
    wavefront = engine != "mega"
    rc, L, pos, _ = _gpu_samples(scene, integ, A.FLAG_WAVEFRONT if wavefront else 0)
    if wavefront and not _path_wavefront_ok(max_depth):
        return _assert_unsupported(rc)   # refused, not rendered
    A.check(rc)
    _assert_samples(L, pos, _ref_samples("room", None, itype, max_depth, rr_depth), f"{itype} {engine}")


@pytest.mark.parametrize("max_depth,rr_depth", DC.GRID_PATH)
@pytest.mark.parametrize("itype", ["path", "prb"])
def test_room_default_film_and_mode(itype, max_depth, rr_depth):
    """mh_render without an engine flag: the film against the oracle's, and
    the engine mh_stats reports -- test_plan_host.py's render_depth_0 / _1 /
    _64 / _65: 2 (fused wavefront) for path at 1 .. 64, else 0."""
    mi = _mi()
    from mitsuba_hip import _abi as A
    scene = _scene("room")
    integ = DC.integrator(mi, itype, max_depth, rr_depth)
    st = A.Stats()
    film = mi.render_film(scene, integ, seed=SEED, stats=st).cpu().numpy()
    assert st.mode == (2 if itype == "path" and _path_wavefront_ok(max_depth) else 0), st.mode
    _film_close(film, _ref_film("room", None, itype, max_depth, rr_depth))
    if itype == "path":
        if _path_wavefront_ok(max_depth):
            wf = mi.render_film(scene, integ, seed=SEED, mode="wavefront").cpu().numpy()
            _film_close(wf, _ref_film("room", None, itype, max_depth, rr_depth))
        else:
            with pytest.raises(A.MitsubaHipError, match="wavefront"):
                mi.render_film(scene, integ, seed=SEED, mode="wavefront")


# ---------------------------------------------------------------------------
# per-sample primal: volpath and prbvolpath on the dense cube
# ---------------------------------------------------------------------------
VOL_ENGINES = [("volpath", "mega"), ("volpath", "wavefront"), ("volpath", "wavefront-rounds"),
               ("volpath", "wavefront-finish1"), ("prbvolpath", "mega"), ("prbvolpath", "wavefront")]


def _vol_engine(engine, monkeypatch):
    if engine in ("wavefront-rounds", "wavefront-finish1"):
        monkeypatch.setenv("MH_VOL_MODE", "rounds")
    if engine == "wavefront-finish1":
        monkeypatch.setenv("MH_VW_ROUNDS", "1")
    return engine != "mega"


def _vol_per_sample(kind, itype, engine, max_depth, rr_depth, monkeypatch):
    from mitsuba_hip import _abi as A
    wavefront = _vol_engine(engine, monkeypatch)
    mi = _mi()
    name = f"{kind}:{itype}"
    scene = _scene(name) if engine in ("mega", "wavefront") else _fresh_scene(name)
    integ = DC.integrator(mi, itype, max_depth, rr_depth)
    rc, L, pos, _ = _gpu_samples(scene, integ, A.FLAG_WAVEFRONT if wavefront else 0)
    if wavefront and not _vol_wavefront_ok(max_depth):
        return _assert_unsupported(rc)
    A.check(rc)
    _assert_samples(L, pos, _ref_samples(name, None, itype, max_depth, rr_depth), f"{kind} {itype} {engine}")


@pytest.mark.parametrize("max_depth,rr_depth", DC.GRID_VOL)
@pytest.mark.parametrize("itype,engine", VOL_ENGINES)
def test_dense_per_sample(itype, engine, max_depth, rr_depth, monkeypatch):
    """mega: k_render; wavefront: k_vol_sched; -rounds: k_vw_main / k_vw_walk
    rounds (max_depth + 1 of them) then k_vw_finish; -finish1: one round, then
    the finish kernel.  (1024 | 1025, 100000): the last depth the wavefront
    takes and the first it refuses; (-1, ...) is stored as 0xFFFFFFFF."""
    _vol_per_sample("dense", itype, engine, max_depth, rr_depth, monkeypatch)


@pytest.mark.parametrize("max_depth,rr_depth", [(6, 1), (64, 100000)])
@pytest.mark.parametrize("itype,engine", VOL_ENGINES)
def test_scale20_per_sample(itype, engine, max_depth, rr_depth, monkeypatch):
    """The thinner medium (scale 20, albedo 0.99): paths reach the far side."""
    _vol_per_sample("dense20", itype, engine, max_depth, rr_depth, monkeypatch)


@pytest.mark.parametrize("max_depth,rr_depth", DC.GRID_VOL)
@pytest.mark.parametrize("itype", ["volpath", "prbvolpath"])
def test_dense_default_film_and_mode(itype, max_depth, rr_depth):
    """mh_render without an engine flag: 3 (the phase scheduler) up to 1024,
    else 0 (vs_supported; test_plan_host.py's render_volpath cases)."""
    mi = _mi()
    from mitsuba_hip import _abi as A
    name = f"dense:{itype}"
    scene = _scene(name)
    integ = DC.integrator(mi, itype, max_depth, rr_depth)
    st = A.Stats()
    film = mi.render_film(scene, integ, seed=SEED, stats=st).cpu().numpy()
    assert st.mode == (3 if _vol_wavefront_ok(max_depth) else 0), st.mode
    _film_close(film, _ref_film(name, None, itype, max_depth, rr_depth))
    if not _vol_wavefront_ok(max_depth):
        with pytest.raises(A.MitsubaHipError, match="wavefront"):
            mi.render_film(scene, integ, seed=SEED, mode="wavefront")


# ---------------------------------------------------------------------------
# alpha at max_depth 0 and 1; hide_emitters at 1 and 2
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["mega", "wavefront"])
@pytest.mark.parametrize("max_depth", [0, 1])
@pytest.mark.parametrize("name", ["room", "open_box"])
def test_alpha_at_depth_0_and_1(name, max_depth, engine):
    """path with an rgba film: max_depth 0 returns { 0, false } (path.cpp:103-104)
    whatever the sample planes held before; at 1 a sample is valid where its
    camera ray hits a surface (in the open box the film's border misses)."""
    mi = _mi()
    from mitsuba_hip import _abi as A
    scene = _scene(name, "rgba")
    integ = DC.integrator(mi, "path", max_depth, 5)
    rL, rpos, rvalid = _ref_samples(name, "rgba", "path", max_depth, 5)
    if max_depth == 0:
        assert not rvalid.any()
    elif name == "open_box":
        assert 0.01 < 1 - rvalid.mean() < 0.5
    wavefront = engine == "wavefront"
    rc, L, pos, valid = _gpu_samples(scene, integ, A.FLAG_WAVEFRONT if wavefront else 0)
    if wavefront and max_depth == 0:
        _assert_unsupported(rc)
        with pytest.raises(A.MitsubaHipError, match="wavefront"):
            mi.render_film(scene, integ, seed=SEED, mode="wavefront")
        return
    A.check(rc)
    np.testing.assert_array_equal(pos, rpos)
    np.testing.assert_array_equal(valid, rvalid.astype(np.float32))
    assert np.all(L == rL, axis=1).mean() >= 0.999
    img = mi.develop(scene, mi.render_film(scene, integ, seed=SEED, mode=engine)).cpu().numpy()
    ref = O.develop(_ref_film(name, "rgba", "path", max_depth, 5), scene.desc.sensor.pixel_format)
    assert img.shape == ref.shape == (scene.height, scene.width, 4)
    _film_close(img, ref)
    np.testing.assert_allclose(img[..., 3], ref[..., 3], atol=1e-5)


@pytest.mark.parametrize("engine", ["wavefront", "mega", "wavefront-unfused"])
@pytest.mark.parametrize("max_depth", [1, 2])
def test_hide_emitters_at_depth_1_and_2(max_depth, engine, monkeypatch):
    """hide_emitters with a sky (test_hide_emitters_path_parity's scene and
    modes): at max_depth 1 only the directly visible light is left."""
    if engine == "wavefront-unfused":
        monkeypatch.setenv("MH_WF_FUSED", "0")
    mi = _mi()
    from mitsuba_hip import _abi as A
    scene = _scene("sky_box") if engine != "wavefront-unfused" else _fresh_scene("sky_box")
    integ = DC.integrator(mi, "path", max_depth, 5, hide_emitters=True)
    ref = _ref_samples("sky_box", None, "path", max_depth, 5, True)
    assert (ref[0].sum(1) == 0).mean() > 0.05 and ref[0].mean() > 0
    rc, L, pos, _ = _gpu_samples(scene, integ, A.FLAG_WAVEFRONT if engine != "mega" else 0)
    A.check(rc)
    _assert_samples(L, pos, ref, f"hide_emitters {engine}")


# ---------------------------------------------------------------------------
# prb gradients on the room
# ---------------------------------------------------------------------------
GRID_PRB_GRAD = [(0, 5), (1, 5), (2, 5), (3, 1), (64, 1000), (65, 1000), (-1, 1)]
PRB_KEYS = DC.RGB_KEYS + [DC.LIGHT_KEY]


def _grad_in(h, w, seed=7):
    """a fixed non-uniform upstream gradient (test_gpu_emitter_grad's)"""
    return (np.random.default_rng(seed).random((h, w, 3)) / (h * w * 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _ref_prb_grads(name, max_depth, rr_depth):
    """The reflectance gradients from the oracle's render_backward.  The
    light's from the oracle's primal: the film is linear in the radiance at a
    fixed seed (test_gpu_emitter_grad.py), so d/d radiance[c] = sum_px
    grad_in[px, c] * I_c[px, c] with I_c the render at radiance e_c."""
    mi = _mi()
    scene = _scene(name)
    integ = DC.integrator(mi, "prb", max_depth, rr_depth)
    params = mi.traverse(scene)
    spp = scene.sample_count()
    gi = _grad_in(scene.height, scene.width)
    ref = O.render_backward(scene, integ, SEED, spp, gi, [params.texture_of(k) for k in DC.RGB_KEYS],
                            [(3,)] * len(DC.RGB_KEYS))
    e = scene.params[DC.LIGHT_KEY][1]
    keep = list(scene.emitter(e).radiance)
    light = np.zeros(3)
    for c in range(3):
        scene.emitter(e).radiance[:] = [0.0, 0.0, 0.0]
        scene.emitter(e).radiance[c] = 1.0
        img = O.develop(O.render(scene, integ, SEED, spp)).astype(np.float64)
        light[c] = (gi[..., c].astype(np.float64) * img[..., c]).sum()
    scene.emitter(e).radiance[:] = keep
    return _frozen(ref + [light])


def _assert_prb_grads(g, ref, max_depth, what):
    for k, a, b in zip(PRB_KEYS, g, ref):
        a = a.cpu().numpy()
        rel = np.abs(a - b)[b != 0] / np.abs(b[b != 0])
        print(f"{what} {k}: got {a} want {b}, max rel {rel.max() if rel.size else 0.0:.2e}")
        np.testing.assert_allclose(a, b, rtol=1e-3, atol=1e-7, err_msg=f"{what} {k}")
    assert np.all(ref[3] > 0) and np.all(g[3].cpu().numpy() != 0)   # the light is seen at every depth
    if _depth(max_depth) <= 1:   # no bounce: no reflectance is ever evaluated
        for a, b in zip(g[:3], ref[:3]):
            assert not b.any() and not a.cpu().numpy().any()
    else:
        assert np.abs(ref[0]).max() > 0


@pytest.mark.parametrize("max_depth,rr_depth", GRID_PRB_GRAD)
@pytest.mark.parametrize("mode", ["auto", "mega", "replay"])
def test_prb_backward_room(mode, max_depth, rr_depth):
    """auto: the fused wavefront for 1 <= max_depth <= 64 (mh_stats mode 1),
    else the per-lane kernel -- at max_depth 0 too (test_plan_host.py's
    bwd_depth_0): prb still adds the light its camera ray sees
    (prb.py:121-135), and a wavefront of zero bounces would return no gradient
    for its radiance; mega: prb_fused; replay: prb_sample<Grad>."""
    mi = _mi()
    import torch
    from mitsuba_hip import _abi as A
    scene = _scene("room")
    integ = DC.integrator(mi, "prb", max_depth, rr_depth)
    params = mi.traverse(scene)
    gi = torch.from_numpy(_grad_in(scene.height, scene.width)).cuda()
    st = A.Stats()
    g = mi.render_backward(scene, params, gi, PRB_KEYS, integ, seed=SEED, mode=mode, stats=st)
    assert st.mode == (1 if mode == "auto" and _path_wavefront_ok(max_depth) else 0), st.mode
    _assert_prb_grads(g, _ref_prb_grads("room", max_depth, rr_depth), max_depth, f"{mode} ({max_depth}, {rr_depth})")


def test_prb_backward_room_deterministic():
    """MH_FLAG_DETERMINISTIC at (64, 1000): per-path sums of 64 vertices
    reduced in a fixed order -- the same bits twice, and the oracle's values."""
    mi = _mi()
    import torch
    scene = _scene("room")
    integ = DC.integrator(mi, "prb", 64, 1000)
    params = mi.traverse(scene)
    gi = torch.from_numpy(_grad_in(scene.height, scene.width)).cuda()
    a = mi.render_backward(scene, params, gi, PRB_KEYS, integ, seed=SEED, deterministic=True)
    b = mi.render_backward(scene, params, gi, PRB_KEYS, integ, seed=SEED, deterministic=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    _assert_prb_grads(a, _ref_prb_grads("room", 64, 1000), 64, "deterministic (64, 1000)")


@pytest.mark.parametrize("max_depth,lds", [(32, "1"), (32, "0"), (33, "1")])
def test_prb_backward_room_bitmap(max_depth, lds, monkeypatch):
    """A 5 x 7 x 3 bitmap on the back wall, rr_depth 1000.  32: the last depth
    whose max_depth - 1 = 31 vertex records the fused wavefront keeps (the
    texel scatter in LDS and as global atomics, MH_PRB_LDS_TEX=0); 33: the
    replay kernel.  The bitmap criterion of test_prb_backward_bitmap_parity."""
    monkeypatch.setenv("MH_PRB_LDS_TEX", lds)
    mi = _mi()
    import torch
    from mitsuba_hip import _abi as A
    scene = _scene("room_bitmap")
    integ = DC.integrator(mi, "prb", max_depth, 1000)
    params = mi.traverse(scene)
    keys = [DC.BACK_KEY, "red.reflectance.value"]
    assert tuple(params[DC.BACK_KEY].shape) == (5, 7, 3)
    gi = _grad_in(scene.height, scene.width)
    st = A.Stats()
    g = mi.render_backward(scene, params, torch.from_numpy(gi).cuda(), keys, integ, seed=SEED, stats=st)
    assert st.mode == (1 if max_depth <= 32 else 0), st.mode
    ref = O.render_backward(scene, integ, SEED, scene.sample_count(), gi, [params.texture_of(k) for k in keys],
                            [tuple(params[k].shape) for k in keys])
    for k, a, b in zip(keys, g, ref):
        a = a.cpu().numpy()
        assert a.shape == b.shape and np.abs(b).min() > 0, k
        print(f"bitmap {max_depth} lds={lds} {k}: max rel {np.max(np.abs(a - b) / np.abs(b)):.2e}")
        np.testing.assert_allclose(a, b, rtol=2e-3, atol=1e-9 + 2e-4 * np.abs(b).max(), err_msg=k)


# ---------------------------------------------------------------------------
# render_forward of prb on the room
# ---------------------------------------------------------------------------
def _forward_close(img, ref):
    """test_gpu_forward.py's image criterion"""
    d = np.abs(img - ref)
    ok = d <= 1e-4 + 2e-3 * np.abs(ref)
    assert ok.mean() >= 0.995, f"{(~ok).sum()} of {ok.size} channels off, max {d.max():.3e}"
    assert d.mean() / max(np.abs(ref).mean(), 1e-12) < 1e-3


@pytest.mark.parametrize("max_depth,rr_depth", [(0, 5), (1, 5), (64, 1000), (65, 1000)])
def test_render_forward_room(max_depth, rr_depth):
    """The fused forward wavefront for 1 <= max_depth <= 64 (mode 2), else the
    per-sample kernel (test_plan_host.py's fwd_prb_depth_0 / _1 / _64 / _65).
    Reflectance tangents against the oracle's render_forward (zero images at
    max_depth <= 1); the light's tangent e_1 against the oracle's primal at
    radiance e_1 (test_gpu_emitter_grad.py's identity, its tolerances)."""
    mi = _mi()
    import torch
    from mitsuba_hip import _abi as A
    scene = _scene("room")
    integ = DC.integrator(mi, "prb", max_depth, rr_depth)
    params = mi.traverse(scene)
    spp = scene.sample_count()
    mode = 2 if _path_wavefront_ok(max_depth) else 0
    tans = {"white.reflectance.value": np.array([1.0, -0.5, 0.25], np.float32),
            "red.reflectance.value": np.array([0.3, 0.2, 0.1], np.float32)}
    st = A.Stats()
    img = mi.render_forward(scene, params, {k: torch.from_numpy(v).cuda() for k, v in tans.items()}, integ,
                            seed=SEED, spp=spp, stats=st).cpu().numpy()
    assert st.mode == mode, st.mode
    ref = O.develop(O.render_forward(scene, integ, SEED, spp, [params.param_id(k) for k in tans],
                                     list(tans.values())))
    if max_depth <= 1:
        assert not ref.any() and not img.any()
    else:
        assert np.abs(ref).mean() > 1e-3
        _forward_close(img, ref)
    st = A.Stats()
    t = torch.tensor([0.0, 1.0, 0.0], device="cuda")
    img = mi.render_forward(scene, params, {DC.LIGHT_KEY: t}, integ, seed=SEED, spp=spp, stats=st).cpu().numpy()
    assert st.mode == mode, st.mode
    e = scene.params[DC.LIGHT_KEY][1]
    keep = list(scene.emitter(e).radiance)
    scene.emitter(e).radiance[:] = [0.0, 1.0, 0.0]
    try:
        basis = O.develop(O.render(scene, integ, SEED, spp))
    finally:
        scene.emitter(e).radiance[:] = keep
    assert basis[..., 1].sum() > 0
    np.testing.assert_allclose(img, basis, rtol=1e-3, atol=1e-6)


@pytest.mark.parametrize("max_depth", [64, 65])
def test_render_forward_adjoint_identity_room(max_depth):
    """<J v, w> == <v, J^T w> at the last depth of the forward and backward
    wavefronts and the first of the per-sample kernels (rtol 2e-3,
    test_render_forward_adjoint_identity_config3's)."""
    mi = _mi()
    import torch
    scene = _scene("room")
    integ = DC.integrator(mi, "prb", max_depth, 1000)
    params = mi.traverse(scene)
    keys = ["white.reflectance.value", "green.reflectance.value", DC.LIGHT_KEY]
    v = [np.array([0.7, -0.3, 1.1], np.float32), np.array([0.2, 0.9, -0.1], np.float32),
         np.array([1.0, 2.0, -0.5], np.float32)]
    img = mi.render_forward(scene, params, {k: torch.from_numpy(t).cuda() for k, t in zip(keys, v)}, integ,
                            seed=SEED).cpu().numpy()
    w = _grad_in(scene.height, scene.width, seed=1)
    g = mi.render_backward(scene, params, torch.from_numpy(w).cuda(), keys, integ, seed=SEED)
    lhs = float((w.astype(np.float64) * img).sum())
    rhs = float(sum((a.cpu().numpy().astype(np.float64) * t).sum() for a, t in zip(g, v)))
    print(f"adjoint identity at {max_depth}: {lhs} against {rhs}")
    assert abs(lhs - rhs) <= 2e-3 * abs(rhs), (lhs, rhs)


# ---------------------------------------------------------------------------
# prbvolpath gradients
# ---------------------------------------------------------------------------
PVP_KEYS = ["medium1.sigma_t.value", "medium1.albedo.value"]


def _pvp_mode(mode, monkeypatch):
    if mode == "sched_off":
        monkeypatch.setenv("MH_PVP_SCHED", "0")
    elif mode == "replay":
        monkeypatch.setenv("MH_PVP_NEE_LOG", "0")


@functools.lru_cache(maxsize=None)
def _ref_pvp_grads(kind, max_depth, rr_depth):
    mi = _mi()
    scene = _scene(f"{kind}:prbvolpath")
    params = mi.traverse(scene)
    gi = _grad_in(scene.height, scene.width, seed=4)
    return _frozen(O.render_backward(scene, DC.integrator(mi, "prbvolpath", max_depth, rr_depth), SEED,
                                     scene.sample_count(), gi, [params.param_id(k) for k in PVP_KEYS],
                                     [tuple(params[k].shape) for k in PVP_KEYS]))


def _pvp_backward(kind, max_depth, rr_depth):
    mi = _mi()
    import torch
    scene = _scene(f"{kind}:prbvolpath")
    params = mi.traverse(scene)
    gi = torch.from_numpy(_grad_in(scene.height, scene.width, seed=4)).cuda()
    g = mi.render_backward(scene, params, gi, PVP_KEYS, DC.integrator(mi, "prbvolpath", max_depth, rr_depth),
                           seed=SEED)
    return [a.cpu().numpy() for a in g]


def _assert_pvp_grads(g, ref, max_depth, what):
    for k, a, b in zip(PVP_KEYS, g, ref):
        assert a.shape == b.shape, k
        if _depth(max_depth) <= 1:   # nothing is added before depth 1 (prbvolpath.py:216-234): no gradient
            assert not b.any() and not a.any(), k
            continue
        assert np.abs(b).max() > 0, k
        print(f"{what} {k}: got {a.ravel()} want {b.ravel()}, max rel {np.max(np.abs(a - b) / np.abs(b)):.2e}")
        np.testing.assert_allclose(a, b, rtol=2e-3, atol=1e-7 + 2e-4 * np.abs(b).max(), err_msg=f"{what} {k}")


@pytest.mark.parametrize("max_depth,rr_depth", [(0, 5), (1, 5), (2, 5), (6, 1), (64, 100000), (-1, 1)])
@pytest.mark.parametrize("mode", ["sched", "sched_off", "replay"])
def test_prbvolpath_backward_scale20(mode, max_depth, rr_depth, monkeypatch):
    """sigma_t and albedo of the scale-20 medium.  sched: k_vol_sched<PvBwdMachine>
    (max_depth <= 1024; (-1, 1) takes the per-sample kernel); sched_off:
    k_prbvol_backward; replay: two passes, the NEE walks replayed."""
    _pvp_mode(mode, monkeypatch)
    g = _pvp_backward("dense20", max_depth, rr_depth)
    _assert_pvp_grads(g, _ref_pvp_grads("dense20", max_depth, rr_depth), max_depth,
                      f"{mode} ({max_depth}, {rr_depth})")


@pytest.mark.parametrize("max_depth", [1024, 1025])
@pytest.mark.parametrize("mode", ["sched", "sched_off", "replay"])
def test_prbvolpath_backward_log_overflow(mode, max_depth, monkeypatch, capfd):
    """The dense cube (albedo 0.99) at 8 x 8 @ 4 with the default log caps of
    256 MainLog / NeeLog entries per thread: paths of up to max_depth scatters
    overflow them for real.  1024: the last depth of the scheduler; 1025: the
    per-sample kernel.  mh_stats does not count the overflow replays; the
    scheduler prints them under MH_VW_DEBUG, which this test reads for
    (sched, 1024).  That paths are long enough: on the oracle, samples still
    change between max_depth 300 and 1024."""
    _pvp_mode(mode, monkeypatch)
    sched = mode == "sched" and max_depth == 1024
    if sched:
        monkeypatch.setenv("MH_VW_DEBUG", "1")
    a = _ref_samples("dense_small:prbvolpath", None, "prbvolpath", 300, 100000)[0]
    b = _ref_samples("dense_small:prbvolpath", None, "prbvolpath", 1024, 100000)[0]
    assert np.any(a != b, axis=1).sum() >= 3
    g = _pvp_backward("dense_small", max_depth, 100000)
    if sched:
        m = re.search(r"pvb overflow replays: (\d+) paths, (\d+) walks, (\d+) lost", capfd.readouterr().err)
        assert m, "MH_VW_DEBUG: the scheduler's overflow counts"
        print(f"overflow replays: {m.group(1)} paths, {m.group(2)} walks, {m.group(3)} lost")
        assert int(m.group(1)) + int(m.group(2)) >= 1 and int(m.group(3)) == 0
    _assert_pvp_grads(g, _ref_pvp_grads("dense_small", max_depth, 100000), max_depth, f"{mode} ({max_depth})")
