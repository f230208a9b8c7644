"""GPU: every call path at launch shapes that are not round (ragged_cases.py;
DESIGN.md §4 "Launch geometry"), HIP through the C-ABI against the CPU oracle,
which test_ragged_oracle.py pins at the same shapes.

What the shapes reach that the round shapes of the other GPU tests do not:
lane_of's integer-division forms (S and spp each a power of two or not:
`slabs12` shift + division, `slab16` division + shift, the full cases
division + division), the splat kernels' 16-lane rounds with idle lanes and a
one-sample last round (Sn = 3, 5, 7, 12, 17, 33), path counts below a wave and
no multiple of 64 over the 64 queue segments, k_vol_sched's uneven column
bands (W = 13, 20, 27, 11) and its no-band path (W = 7), and chunks of 1,020
samples that start in the middle of a pixel row on alternating streams.

Criteria: the suite's own (tests/test_gpu_parity.py's docstring and the tests
named below); none is new.
  per sample  positions equal; >= 99.9 % of the samples bit-identical and every
              other one within 1e-4 max(1, |L|); below 1,000 samples at most
              one sample may differ in bits (ragged_cases.assert_per_sample)
  film        |d| <= 1e-4 max(1, |ref|) on >= 99.5 % of the pixels; W image
              rtol 1e-5 (test_prb_weights_parity)
  gradient    rgb rtol 1e-3, atol 1e-7; bitmap and prbvolpath rtol 2e-3 with
              atol 2e-4 max |ref| (test_prb_backward_bitmap_parity,
              test_prbvolpath_backward_parity); deterministic runs bit-equal
  forward     test_gpu_forward._close; adjoint identity within 2e-3

The oracle differentiates no phase function, so '<medium>.phase_function.g'
is held to the forward-mode image of the same seeded render (the adjoint
identity, as test_gpu_phase_g_grad.test_multiple_scattering_bookkeeping does)
and to the sum over slabs.

Deterministic films are bit-reproducible from 4 samples per pixel and pass on
(render_film's contract); `tiny` (3 spp) keeps the float atomics and is held
to the atomic film only.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_py as O
import ragged_cases as RC
from test_gpu_film_filters import _grad_in
from test_gpu_forward import _close

pytestmark = pytest.mark.gpu

SEED = 3
ENV = ("MH_WF_CHUNK", "MH_WF_STREAMS", "MH_TRAVERSAL", "MH_WF_FUSED", "MH_VOL_MODE", "MH_MODE", "MH_WF_BPC",
       "MH_PRB_LDS_TEX", "MH_PVP_SCHED", "MH_BVH4", "MH_BVH4Q", "MH_DETERMINISTIC")


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


_refs = {}


def _ref(name, fn):
    """Oracle results, computed once per case and shared (never modified)."""
    if name not in _refs:
        r = fn()
        for a in (r if isinstance(r, (list, tuple)) else [r]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _refs[name] = r
    return _refs[name]


def _shape(case):
    return (case.w, case.h, case.spp)


def _gpu_samples(scene, integ, case, b, e, flags=0):
    """mh_render_samples of slab [b, e): (n, 3) radiance and (n, 2) positions, pixel-major, e - b per pixel."""
    from mitsuba_hip import _abi as A
    n = RC.n_px(case) * (e - b)
    out = np.zeros(5 * n, np.float32)
    ic = integ.c()
    full = (b, e) == (0, case.spp)
    A.check(A.lib().mh_render_samples(scene.handle(0), C.byref(ic), SEED, case.spp, 0 if full else b, 0 if full else e,
                                      out.ctypes.data_as(C.c_void_p), flags))
    return out[:3 * n].reshape(3, n).T, out[3 * n:].reshape(2, n).T


def _oracle_samples(tag, scene, integ, case):
    return _ref(("samples", tag, _shape(case)),
                lambda: O.sample_range(scene, integ, SEED, case.spp, 0, RC.n_px(case) * case.spp)[:2])


def _check_samples(tag, scene, integ, case, b, e, flags):
    L, pos = _gpu_samples(scene, integ, case, b, e, flags)
    rL, rpos = _oracle_samples(tag, scene, integ, case)
    lanes = RC.slab_lanes(case, b, e)
    np.testing.assert_array_equal(pos, rpos[lanes])
    assert np.abs(rL[lanes]).max() > 0
    RC.assert_per_sample(L, rL[lanes])


# ---------------------------------------------------------------------------
# path, per sample
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["mega", "wavefront", "lane", "unfused"])
@pytest.mark.parametrize("case,b,e", RC.launches(RC.FULL + RC.SLABBED))
def test_path_per_sample(case, b, e, mode, monkeypatch):
    """mega: k_render<PATH>; wavefront: the fused bounce kernel on the packet
    engine; lane: MH_TRAVERSAL=lane; unfused: MH_WF_FUSED=0 (trace / shade /
    shadow kernels)."""
    if mode == "lane":
        monkeypatch.setenv("MH_TRAVERSAL", "lane")
    if mode == "unfused":
        monkeypatch.setenv("MH_WF_FUSED", "0")
    mi = _mi()
    from mitsuba_hip import _abi as A
    scene = RC.cbox(mi, case)
    integ = mi.load_dict({"type": "path", "max_depth": 6})
    _check_samples("cbox", scene, integ, case, b, e, 0 if mode == "mega" else A.FLAG_WAVEFRONT)


@pytest.mark.parametrize("bvh4", ["1", "0"])
@pytest.mark.parametrize("name", ["odd", "chunks"])
def test_path_per_sample_stream_engine(name, bvh4, monkeypatch):
    """The 6,000-triangle mesh scene: the per-lane stream engine on the
    collapsed 4-wide BVH and on the binary one (MH_BVH4=0).  `chunks` also as
    a film over its 7 chunks on the two streams (one splat per chunk)."""
    monkeypatch.setenv("MH_BVH4", bvh4)
    monkeypatch.setenv("MH_BVH4Q", "0")
    mi = _mi()
    from mitsuba_hip import _abi as A
    case = RC.CASES[name]
    scene = RC.blob(mi, case)
    integ = scene.integrator()
    _check_samples("blob", scene, integ, case, 0, case.spp, A.FLAG_WAVEFRONT)
    if name == "chunks":
        RC.apply_env(case, monkeypatch)
        st = A.Stats()
        film = mi.render_film(scene, integ, seed=SEED, spp=case.spp, stats=st).cpu().numpy()
        assert st.mode == 1 and st.n_aux_launches == RC.n_chunks(case) == 7
        ref = _ref(("film", "blob", _shape(case)), lambda: O.render(scene, integ, seed=SEED, spp=case.spp))
        ok, frac = RC.film_close(film, ref)
        assert ok, f"film parity {frac}"


@pytest.mark.parametrize("name", ["chunks", "chunks1s"])
def test_path_chunks_really_chunk(name, monkeypatch):
    """27 x 20 @ 12 under MH_WF_CHUNK=1024: 85 pixels per chunk, so
    ceil(540 / 85) = 7 chunks, each with its own bounce launches."""
    mi = _mi()
    from mitsuba_hip import _abi as A
    case = RC.CASES[name]
    RC.apply_env(case, monkeypatch)
    scene = RC.cbox(mi, case)
    integ = mi.load_dict({"type": "path", "max_depth": 6})
    st = A.Stats()
    mi.render_film(scene, integ, seed=SEED, spp=case.spp, stats=st)
    assert RC.n_chunks(case) == 7
    assert st.mode == 2 and st.n_aux_launches == 7 and st.n_trace_launches == 7 * 6
    assert st.samples == 27 * 20 * 12


# ---------------------------------------------------------------------------
# film and W image
# ---------------------------------------------------------------------------
FILM_LAUNCHES = RC.launches(RC.FULL + ["chunks1s"] + RC.SLABBED)


def _oracle_film(tag, scene, integ, case, b, e):
    return _ref(("film", tag, _shape(case), b, e),
                lambda: O.render(scene, integ, seed=SEED, spp=case.spp, **RC.slab_kw(case, b, e)))


@pytest.mark.parametrize("mode", ["auto", "mega", "deterministic"])
@pytest.mark.parametrize("case,b,e", FILM_LAUNCHES)
def test_film_parity(case, b, e, mode, monkeypatch):
    RC.apply_env(case, monkeypatch)
    mi = _mi()
    scene = RC.cbox(mi, case)
    integ = mi.load_dict({"type": "path", "max_depth": 6})
    kw = dict(seed=SEED, spp=case.spp, **RC.slab_kw(case, b, e))
    if mode == "deterministic":
        film = mi.render_film(scene, integ, deterministic=True, **kw)
        again = mi.render_film(scene, integ, deterministic=True, **kw).cpu().numpy()
        atomic = mi.render_film(scene, integ, **kw).cpu().numpy()
        if case.spp >= 4:   # below: the float atomics (render_film's contract)
            assert np.array_equal(film.cpu().numpy(), again)
        np.testing.assert_allclose(film.cpu().numpy(), atomic, rtol=1e-5, atol=1e-6)
    else:
        film = mi.render_film(scene, integ, mode=mode, **kw)
    ref = _oracle_film("cbox", scene, integ, case, b, e)
    assert ref[..., 3].min() > 0
    ok, frac = RC.film_close(film.cpu().numpy(), ref)
    assert ok, f"film parity {frac}"
    ok, frac = RC.film_close(mi.develop(scene, film).cpu().numpy(), O.develop(ref))
    assert ok, f"image parity {frac}"


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("case,b,e", RC.launches(RC.FULL + RC.SLABBED))
def test_weights_parity(case, b, e, deterministic):
    mi = _mi()
    scene = RC.cbox(mi, case)
    w = mi.prb_weights(scene, SEED, case.spp, b, e, deterministic=deterministic).cpu().numpy()
    ref = _ref(("w", _shape(case), b, e), lambda: O.prb_weights(scene, SEED, case.spp, b, e))
    assert ref.min() > 0
    np.testing.assert_allclose(w, ref, rtol=1e-5, atol=1e-6)
    if deterministic and case.spp >= 4:
        assert np.array_equal(w, mi.prb_weights(scene, SEED, case.spp, b, e, deterministic=True).cpu().numpy())


def _open_box_rgba(mi, case):
    d = RC._shape(mi.cornell_box(), case, "rgba")
    if case.h > 1:   # camera rays escape: alpha 0 there (every ray of `tiny`'s one row would: it keeps the wall)
        d.pop("back")
    return mi.load_dict(d)


@pytest.mark.parametrize("mode", ["auto", "mega", "deterministic"])
@pytest.mark.parametrize("name", ["odd", "over16", "tiny"])
def test_rgba_film_parity(name, mode):
    """An alpha film: the alpha splat (kSplatAlpha) and the W channel beside the rgb splat."""
    mi = _mi()
    case = RC.CASES[name]
    scene = _open_box_rgba(mi, case)
    integ = mi.load_dict({"type": "path", "max_depth": 6})
    kw = {"deterministic": True} if mode == "deterministic" else {"mode": mode}
    film = mi.render_film(scene, integ, seed=SEED, spp=case.spp, **kw).cpu().numpy()
    ref = _ref(("film", "rgba", _shape(case)), lambda: O.render(scene, integ, seed=SEED, spp=case.spp))
    assert film.shape == ref.shape == (case.h, case.w, 5)
    assert 0 < ref[..., 3].sum() < 0.9 * ref[..., 4].sum()   # alpha 1 for some samples, 0 for others
    ok, frac = RC.film_close(film, ref)
    assert ok, f"film parity {frac}"
    np.testing.assert_allclose(film[..., 4], O.prb_weights(scene, SEED, case.spp), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", RC.SLABBED)
def test_slab_films_sum_to_the_full_film(name):
    mi = _mi()
    case = RC.CASES[name]
    scene = RC.cbox(mi, case)
    integ = mi.load_dict({"type": "path", "max_depth": 6})
    cuts = sorted({0, case.spp} | {x for s in case.slabs for x in s})
    full = mi.render_film(scene, integ, seed=SEED, spp=case.spp).cpu().numpy()
    acc = np.zeros_like(full)
    for b, e in zip(cuts[:-1], cuts[1:]):
        acc += mi.render_film(scene, integ, seed=SEED, spp=case.spp, spp_begin=b, spp_end=e).cpu().numpy()
    ok, frac = RC.film_close(acc, full)
    assert ok, frac


@pytest.mark.parametrize("mode", ["auto", "mega"])
@pytest.mark.parametrize("name", ["odd", "over16"])
def test_invalid_sample_counter(name, mode):
    """mh_stats.invalid_samples against the count from the call's own samples
    (test_gpu_aux.test_invalid_sample_counter), under a light with a negative channel."""
    mi = _mi()
    from mitsuba_hip import _abi as A
    case = RC.CASES[name]
    d = RC._shape(mi.cornell_box(), case)
    d["light"]["emitter"]["radiance"]["value"] = [-1.0, 2.0, 3.0]
    scene = mi.load_dict(d)
    integ = mi.load_dict({"type": "path", "max_depth": 6})
    st = A.Stats()
    mi.render_film(scene, integ, seed=SEED, spp=case.spp, stats=st, mode=mode)
    L, _ = _gpu_samples(scene, integ, case, 0, case.spp, 0 if mode == "mega" else A.FLAG_WAVEFRONT)
    expect = int(np.sum(np.any(~(L >= -1e-5) | ~np.isfinite(L), axis=1)))
    assert expect > 0 and st.invalid_samples == expect


# ---------------------------------------------------------------------------
# prb backward, rgb keys
# ---------------------------------------------------------------------------
RGB_KEYS = ["white.reflectance.value", "red.reflectance.value", "green.reflectance.value"]
PRB_DEPTH = 6


def _prb(mi):
    return mi.load_dict({"type": "prb", "max_depth": PRB_DEPTH})


def _oracle_rgb_grad(scene, params, integ, case, b=0, e=0, weights=None):
    """All three keys at once; a call with fewer keys is held to its rows."""
    gi = _grad_in(case.w, case.h)
    return _ref(("grad", _shape(case), b, e),
                lambda: O.render_backward(scene, integ, SEED, case.spp, gi, [params.texture_of(k) for k in RGB_KEYS],
                                          [(3,)] * 3, weights=weights, spp_begin=b, spp_end=e))


PRB_MODES = ["auto", "replay", "mega", "deterministic", "unfused"]


def _prb_backward(mi, scene, params, keys, case, mode, **kw):
    import torch
    gi = torch.from_numpy(_grad_in(case.w, case.h)).cuda()
    mkw = {"deterministic": True} if mode == "deterministic" else {"mode": "auto" if mode == "unfused" else mode}
    g = mi.render_backward(scene, params, gi, keys, _prb(mi), seed=SEED, spp=case.spp, **mkw, **kw)
    return [x.cpu().numpy() for x in g]


@pytest.mark.parametrize("mode", PRB_MODES)
@pytest.mark.parametrize("n_keys", [1, 2, 3])
@pytest.mark.parametrize("name", ["odd", "over16", "over32", "chunks", "chunks1s", "tiny"])
def test_prb_backward_rgb(name, n_keys, mode, monkeypatch):
    """One key: the NEE-ring instance of the fused bounce kernel; two and
    three keys: the four-slot instance.  deterministic: summed per path and
    reduced in path-id order over a ragged path count -- three runs, the same bits."""
    case = RC.CASES[name]
    RC.apply_env(case, monkeypatch)
    if mode == "unfused":
        monkeypatch.setenv("MH_WF_FUSED", "0")
    mi = _mi()
    scene = RC.cbox(mi, case)
    params = mi.traverse(scene)
    keys = RGB_KEYS[:n_keys]
    g = _prb_backward(mi, scene, params, keys, case, mode)
    if mode == "deterministic":
        for _ in range(2):
            for a, b in zip(g, _prb_backward(mi, scene, params, keys, case, mode)):
                assert np.array_equal(a, b)
    ref = _oracle_rgb_grad(scene, params, _prb(mi), case)
    for k, a, r in zip(keys, g, ref):
        assert np.abs(r).max() > 0 or (name == "tiny" and k == RGB_KEYS[1]), k   # no path of `tiny` meets the red wall
        np.testing.assert_allclose(a, r, rtol=1e-3, atol=1e-7, err_msg=k)


@pytest.mark.parametrize("name", ["chunks", "chunks1s"])
def test_prb_backward_rgb_ring_several_iterations(name, monkeypatch):
    """MH_WF_BPC=1: 256 workgroups, so that the waves of a 1,020-path chunk
    run several iterations and the NEE ring is pushed to and drained."""
    case = RC.CASES[name]
    RC.apply_env(case, monkeypatch)
    monkeypatch.setenv("MH_WF_BPC", "1")
    mi = _mi()
    from mitsuba_hip import _abi as A
    scene = RC.cbox(mi, case)
    params = mi.traverse(scene)
    st = A.Stats()
    (g,) = _prb_backward(mi, scene, params, RGB_KEYS[:1], case, "auto", stats=st)
    assert st.n_trace_launches == 7 * PRB_DEPTH
    ref = _oracle_rgb_grad(scene, params, _prb(mi), case)
    np.testing.assert_allclose(g, ref[0], rtol=1e-3, atol=1e-7)


@pytest.mark.parametrize("mode", ["auto", "replay", "deterministic"])
@pytest.mark.parametrize("name", RC.SLABBED)
def test_prb_backward_rgb_slabs(name, mode):
    """Every slab with the full W image as `weights` against the oracle's
    gradient of that slab, and the slabs' sum against the full gradient."""
    mi = _mi()
    case = RC.CASES[name]
    scene = RC.cbox(mi, case)
    params = mi.traverse(scene)
    w = mi.prb_weights(scene, SEED, case.spp)
    rw = _ref(("w", _shape(case), 0, 0), lambda: O.prb_weights(scene, SEED, case.spp))
    np.testing.assert_allclose(w.cpu().numpy(), rw, rtol=1e-5, atol=1e-6)
    cuts = sorted({0, case.spp} | {x for s in case.slabs for x in s})
    acc = [np.zeros(3, np.float64) for _ in RGB_KEYS]
    for b, e in zip(cuts[:-1], cuts[1:]):
        g = _prb_backward(mi, scene, params, RGB_KEYS, case, mode, spp_begin=b, spp_end=e, weights=w)
        ref = _oracle_rgb_grad(scene, params, _prb(mi), case, b, e, weights=rw)
        for k, a, r, s in zip(RGB_KEYS, g, ref, acc):
            assert np.abs(r).max() > 0, k
            np.testing.assert_allclose(a, r, rtol=1e-3, atol=1e-7, err_msg=f"{k} [{b},{e})")
            s += a
    full = _oracle_rgb_grad(scene, params, _prb(mi), case)
    for k, s, r in zip(RGB_KEYS, acc, full):
        np.testing.assert_allclose(s, r, rtol=1e-3, atol=1e-7, err_msg=k)


# ---------------------------------------------------------------------------
# prb backward, bitmap key
# ---------------------------------------------------------------------------
BMP_KEYS = ["white.reflectance.data", "red.reflectance.value"]


@pytest.mark.parametrize("mode", ["auto", "auto-lds0", "replay", "deterministic"])
@pytest.mark.parametrize("name", ["odd", "over16", "chunks", "chunks1s"])
def test_prb_backward_bitmap(name, mode, monkeypatch):
    """auto: vertex records on the fused wavefront and the texel scatter, in
    LDS and (MH_PRB_LDS_TEX=0) as transposed global atomics; replay: the
    per-lane kernel; deterministic: two runs, the same bits."""
    case = RC.CASES[name]
    RC.apply_env(case, monkeypatch)
    if mode == "auto-lds0":
        monkeypatch.setenv("MH_PRB_LDS_TEX", "0")
    mi = _mi()
    import torch
    from mitsuba_hip import _abi as A
    scene = RC.cbox_bitmap(mi, case)
    integ = _prb(mi)
    params = mi.traverse(scene)
    gi = _grad_in(case.w, case.h)
    mkw = {"deterministic": True} if mode == "deterministic" else {"mode": mode.split("-")[0]}

    def run():
        st = A.Stats()
        g = mi.render_backward(scene, params, torch.from_numpy(gi).cuda(), BMP_KEYS, integ, seed=SEED, spp=case.spp,
                               stats=st, **mkw)
        return [x.cpu().numpy() for x in g], st

    g, st = run()
    assert st.mode == (0 if mode == "replay" else 1), st.mode
    if mode != "replay" and name.startswith("chunks"):
        assert st.n_aux_launches == 7   # one texel scatter per chunk
    if mode == "deterministic":
        for a, b in zip(g, run()[0]):
            assert np.array_equal(a, b)
    ref = _ref(("bmp", _shape(case)),
               lambda: O.render_backward(scene, integ, SEED, case.spp, gi, [params.texture_of(k) for k in BMP_KEYS],
                                         [tuple(params[k].shape) for k in BMP_KEYS]))
    for k, a, r in zip(BMP_KEYS, g, ref):
        assert a.shape == r.shape and np.abs(r).max() > 0, k
        np.testing.assert_allclose(a, r, rtol=2e-3, atol=1e-9 + 2e-4 * np.abs(r).max(), err_msg=k)


# ---------------------------------------------------------------------------
# render_forward
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("bitmap", [False, True])
@pytest.mark.parametrize("case,b,e", RC.launches(["odd", "over16", "chunks", "slabs12"]))
def test_render_forward(case, b, e, bitmap):
    """The fused forward-mode wavefront (k_wf_bounce_fwd) with rgb and with bitmap tangents."""
    mi = _mi()
    import torch
    from mitsuba_hip import _abi as A
    scene = RC.cbox_bitmap(mi, case) if bitmap else RC.cbox(mi, case)
    integ = _prb(mi)
    params = mi.traverse(scene)
    if bitmap:
        key = "white.reflectance.data"
        tans = {key: np.random.default_rng(3).standard_normal(tuple(params[key].shape)).astype(np.float32),
                "green.reflectance.value": np.array([0.2, 0.9, -0.1], np.float32)}
    else:
        tans = {"white.reflectance.value": np.array([1.0, -0.5, 0.25], np.float32),
                "red.reflectance.value": np.array([0.3, 0.2, 0.1], np.float32)}
    st = A.Stats()
    img = mi.render_forward(scene, params, {k: torch.from_numpy(v).cuda() for k, v in tans.items()}, integ, seed=SEED,
                            spp=case.spp, stats=st, **RC.slab_kw(case, b, e)).cpu().numpy()
    assert st.mode == 2
    film = O.render_forward(scene, integ, SEED, case.spp, [params.param_id(k) for k in tans], list(tans.values()),
                            **RC.slab_kw(case, b, e))
    ref = O.develop(film, scene.desc.sensor.pixel_format)
    assert img.shape == ref.shape and np.abs(ref).max() > 0
    _close(img, ref)


def test_render_forward_adjoint_identity():
    """<grad_in, forward image> = <gradient, tangent> at 13 x 7 @ 5 (test_gpu_film_filters.test_adjoint_identity)."""
    mi = _mi()
    import torch
    case = RC.CASES["odd"]
    scene = RC.cbox(mi, case)
    integ = _prb(mi)
    params = mi.traverse(scene)
    key = RGB_KEYS[0]
    tan = np.array([0.7, -0.3, 1.1], np.float32)
    img = mi.render_forward(scene, params, {key: torch.from_numpy(tan).cuda()}, integ, seed=SEED,
                            spp=case.spp).cpu().numpy()
    gi = _grad_in(case.w, case.h, seed=1)
    g = mi.render_backward(scene, params, torch.from_numpy(gi).cuda(), [key], integ, seed=SEED, spp=case.spp)[0]
    lhs = float((gi.astype(np.float64) * img).sum())
    rhs = float((g.cpu().numpy().astype(np.float64) * tan).sum())
    print(f"adjoint: lhs {lhs:.6e} rhs {rhs:.6e} rel {abs(lhs - rhs) / abs(rhs):.3e}")
    assert abs(lhs - rhs) <= 2e-3 * abs(rhs), (lhs, rhs)


# ---------------------------------------------------------------------------
# volpath, per sample
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sched", "rounds", "mega"])
@pytest.mark.parametrize("homogeneous", [False, True], ids=["grid", "homogeneous"])
@pytest.mark.parametrize("case,b,e", RC.launches(["tiny", "odd", "over16", "chunks"] + RC.SLABBED))
def test_volpath_per_sample(case, b, e, homogeneous, mode, monkeypatch):
    """sched: k_vol_sched (column bands q W / 8 of uneven width; W = 7: no
    bands); rounds: MH_VOL_MODE=rounds (k_vw_main / k_vw_walk, k_vw_finish);
    mega: k_render<VOLPATH>."""
    if mode == "rounds":
        monkeypatch.setenv("MH_VOL_MODE", "rounds")
    mi = _mi()
    from mitsuba_hip import _abi as A
    scene = RC.vol(mi, case, "volpath", homogeneous)
    integ = scene.integrator()
    assert integ.type == "volpath"
    _check_samples(("volpath", homogeneous), scene, integ, case, b, e, 0 if mode == "mega" else A.FLAG_WAVEFRONT)


def test_volpath_grid_lookups():
    """mh_stats.grid_lookups of k_vol_sched at 13 x 7 @ 5 equals the oracle's count (test_gpu_stats)."""
    mi = _mi()
    from mitsuba_hip import _abi as A
    case = RC.CASES["odd"]
    scene = RC.vol(mi, case)
    st = A.Stats()
    mi.render_film(scene, seed=SEED, spp=case.spp, stats=st)
    assert st.mode == 3
    O.grid_lookups(reset=True)
    O.render(scene, seed=SEED, spp=case.spp, threads=4)
    ref = O.grid_lookups(reset=True)
    assert ref > RC.n_px(case) * case.spp
    assert st.grid_lookups == ref, (st.grid_lookups, ref)


# ---------------------------------------------------------------------------
# prbvolpath
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sched", "mega"])
@pytest.mark.parametrize("case,b,e", RC.launches(["odd", "over16"] + RC.SLABBED))
def test_prbvolpath_per_sample(case, b, e, mode):
    mi = _mi()
    from mitsuba_hip import _abi as A
    scene = RC.vol(mi, case, "prbvolpath")
    integ = scene.integrator()
    assert integ.type == "prbvolpath"
    _check_samples("prbvolpath", scene, integ, case, b, e, 0 if mode == "mega" else A.FLAG_WAVEFRONT)


G_KEY = "medium1.phase_function.g"


def _pvp_backward(mi, scene, params, keys, gi, case, **kw):
    import torch
    g = mi.render_backward(scene, params, torch.from_numpy(gi).cuda(), keys, scene.integrator(), seed=SEED,
                           spp=case.spp, **kw)
    return [x.cpu().numpy() for x in g]


def _pvp_g_reference(mi, scene, params, gi, case):
    """<forward-mode image for dg = 1, grad_in>: the gradient's scalar (the adjoint identity)."""
    import torch
    img = mi.render_forward(scene, params, {G_KEY: torch.ones(1).cuda()}, scene.integrator(), seed=SEED,
                            spp=case.spp).cpu().numpy()
    return float((img.astype(np.float64) * gi).sum())


@pytest.mark.parametrize("mode", ["default", "sched_off", "deterministic"])
@pytest.mark.parametrize("name", ["odd", "over16"])
def test_prbvolpath_backward(name, mode, monkeypatch):
    """sigma_t grid, albedo and floor reflectance against the oracle on the
    phase scheduler with its per-thread logs (default), on the per-sample
    kernel (MH_PVP_SCHED=0) and in int64 fixed point (deterministic: two runs,
    the same bits); phase_function.g (a call of its own: the per-lane kernel's
    PhG instance) against the forward-mode image."""
    if mode == "sched_off":
        monkeypatch.setenv("MH_PVP_SCHED", "0")
    mi = _mi()
    case = RC.CASES[name]
    scene = RC.vol(mi, case, "prbvolpath")
    integ = scene.integrator()
    params = mi.traverse(scene)
    keys = RC.vol_keys()
    gi = np.random.default_rng(4).standard_normal((case.h, case.w, 3)).astype(np.float32)
    kw = {"deterministic": True} if mode == "deterministic" else {}
    g = _pvp_backward(mi, scene, params, keys, gi, case, **kw)
    (gg,) = _pvp_backward(mi, scene, params, [G_KEY], gi, case, **kw)
    if mode == "deterministic":
        for a, b in zip(g + [gg], _pvp_backward(mi, scene, params, keys, gi, case, **kw) +
                        _pvp_backward(mi, scene, params, [G_KEY], gi, case, **kw)):
            assert np.array_equal(a, b)
    ref = _ref(("pvp", _shape(case)),
               lambda: O.render_backward(scene, integ, SEED, case.spp, gi, [params.param_id(k) for k in keys],
                                         [tuple(params[k].shape) for k in keys]))
    for k, a, r in zip(keys, g, ref):
        assert a.shape == r.shape and np.abs(r).max() > 0, k
        np.testing.assert_allclose(a, r, rtol=2e-3, atol=1e-7 + 2e-4 * np.abs(r).max(), err_msg=k)
    rg = _pvp_g_reference(mi, scene, params, gi, case)
    print(f"{G_KEY}: backward {gg[0]} forward {rg}")
    assert rg != 0
    np.testing.assert_allclose(gg[0], rg, rtol=2e-3, atol=1e-7 + 2e-4 * abs(rg))


def test_prbvolpath_backward_slabs_sum():
    """slabs12: the gradients of [0,4), [4,7) and [7,12), each with the full
    W image as `weights`, sum to the full gradient (the oracle's; g: the call over all 12)."""
    mi = _mi()
    case = RC.CASES["slabs12"]
    scene = RC.vol(mi, case, "prbvolpath")
    integ = scene.integrator()
    params = mi.traverse(scene)
    keys = RC.vol_keys()
    gi = np.random.default_rng(4).standard_normal((case.h, case.w, 3)).astype(np.float32)
    w = mi.prb_weights(scene, SEED, case.spp)
    acc, acc_g = [np.zeros(params[k].shape, np.float64) for k in keys], 0.0
    for b, e in case.slabs:
        for s, a in zip(acc, _pvp_backward(mi, scene, params, keys, gi, case, spp_begin=b, spp_end=e, weights=w)):
            s += a
        acc_g += float(_pvp_backward(mi, scene, params, [G_KEY], gi, case, spp_begin=b, spp_end=e, weights=w)[0][0])
    ref = O.render_backward(scene, integ, SEED, case.spp, gi, [params.param_id(k) for k in keys],
                            [tuple(params[k].shape) for k in keys])
    for k, a, r in zip(keys, acc, ref):
        assert np.abs(r).max() > 0, k
        np.testing.assert_allclose(a, r, rtol=2e-3, atol=1e-7 + 2e-4 * np.abs(r).max(), err_msg=k)
    full_g = float(_pvp_backward(mi, scene, params, [G_KEY], gi, case)[0][0])
    print(f"{G_KEY}: slabs {acc_g} full {full_g}")
    assert full_g != 0
    np.testing.assert_allclose(acc_g, full_g, rtol=2e-3, atol=1e-7 + 2e-4 * abs(full_g))
