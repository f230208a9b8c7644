"""GPU: the Henyey-Greenstein asymmetry '<medium>.phase_function.g' as a
differentiable, updatable parameter of prbvolpath (backward, forward mode,
torch autograd), through the C ABI.

What the expected values are.  With max_depth = 2 and the directional sun as
the only emitter a sample is A * p_hg(cos theta_sun; g): the one scatter vertex
is placed before g is read, the sun's direction is fixed, mis = 1, and the
phase sample that follows leads to no further contribution.  The estimator's
derivative is then the derivative of the render itself, and central
differences of the CPU oracle's PRIMAL renders at g +- 0.01 are the reference
(steps 0.01 and 0.005 differ by 5.8e-5 of the largest pixel derivative).  For
multiple scattering the sampled directions depend on g while the adjoint
differentiates only the detached estimator, so the value is checked
statistically against central differences of forward renders, and the
bookkeeping (engines, overflow, slabs, determinism, forward against backward)
exactly.

"Gradient tolerance" is the project's own: rtol 1e-3 with
atol = 1e-7 + 2e-4 * max|ref|, as the existing prbvolpath tests use.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_py as O
from blend_cases import blend, tab

pytestmark = pytest.mark.gpu

KEY = "medium1.phase_function.g"
SIGMA, ALBEDO, SUN = "medium1.sigma_t.data", "medium1.albedo.value", "sun.irradiance.value"
RTOL = 1e-3
FD_STEP = 0.01
GS = [-0.95, -0.7, -0.3, 0.0, 1e-4, 0.5, 0.85, 0.95]
MESSAGE = "The asymmetry parameter must lie in the interval (-1, 1)!"


def _mi():
    import mitsuba_hip as mi
    if not mi.is_available():
        pytest.fail("no HIP device / native library: the GPU tests need an MI355X")
    mi.set_variant("hip_ad_rgb")
    return mi


def _atol(ref):
    return 1e-7 + 2e-4 * np.abs(ref).max()


def _engine(monkeypatch, engine):
    """sched: the default plan (which keeps a call with a `g` key off the scheduler); sample: MH_PVP_SCHED=0, the
    per-sample single pass; replay: MH_PVP_NEE_LOG=0, primal + adjoint replay with the NEE walks replayed."""
    if engine == "sample":
        monkeypatch.setenv("MH_PVP_SCHED", "0")
    elif engine == "replay":
        monkeypatch.setenv("MH_PVP_NEE_LOG", "0")


def _dict(mi, g=0.5, w=8, h=8, spp=64, max_depth=8, sky=True, hom=False):
    kw = {"medium_type": "homogeneous"} if hom else {}
    d = mi.volume_cube(w, h, spp, grid_res=8, scale=4.0, max_depth=max_depth, rr_depth=5, **kw)
    d["integrator"]["type"] = "prbvolpath"
    d["medium1"]["phase"] = {"type": "hg", "g": g}   # (also at g = 0: volume_cube would make it isotropic)
    if not sky:
        del d["sky"]
    return d


def _grad_in(h, w, seed=7):
    return (np.random.default_rng(seed).random((h, w, 3)) / (h * w * 3)).astype(np.float32)


def _backward(mi, scene, keys, gi, seed, spp, params=None, **kw):
    import torch
    params = params or mi.traverse(scene)
    g = mi.render_backward(scene, params, torch.from_numpy(gi).cuda(), keys, scene.integrator(), seed=seed, spp=spp, **kw)
    return [a.cpu().numpy() for a in g]


def _forward(mi, scene, seed, spp, key=KEY, **kw):
    import torch
    params = mi.traverse(scene)
    return mi.render_forward(scene, params, {key: torch.ones(1).cuda()}, scene.integrator(), seed=seed, spp=spp,
                             **kw).cpu().numpy()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------------------
# 1. function level: mh_phase_eval_grad against the float64 closed form
# ---------------------------------------------------------------------------
def _dirs():
    rng = np.random.default_rng(5)
    v = rng.normal(size=(3, 8190))
    v /= np.sqrt((v ** 2).sum(0))
    wo = np.concatenate([v, [[0.0, 0.0], [0.0, 0.0], [1.0, -1.0]]], axis=1).astype(np.float32)   # ... and +-z
    assert wo.shape == (3, 8192)
    return np.ascontiguousarray(wo)


def _closed_form(g, c, T):
    """d p / d g of eval_hg as the device forms it, in the arithmetic of T"""
    g, c, one = T(g), c.astype(T), T(1)
    temp = (one + g * g) + (T(2) * g) * c
    p = (T(1 / (4 * np.pi)) * (one - g * g)) / (temp * np.sqrt(temp))
    return p * ((T(-2) * g) / (one - g * g) - (T(3) * (g + c)) / temp)


def test_phase_eval_grad_is_the_closed_form():
    mi = _mi()
    from mitsuba_hip import _abi as A
    scene = mi.load_dict(_dict(mi, hom=True))
    params = mi.traverse(scene)
    wo = _dirs()
    for g in GS:
        params[KEY] = g
        params.update()
        out = np.zeros(wo.shape[1], np.float32)
        A.check(A.lib().mh_phase_eval_grad(scene.handle(0), 0, out.size, _p(wo), _p(out), 0))
        g32 = np.float32(g)
        ref = _closed_form(np.float64(g32), -wo[2], np.float64)
        f32 = _closed_form(g32, -wo[2], np.float32)
        err_dev, err_f32 = np.abs(out - ref).max(), np.abs(f32.astype(np.float64) - ref).max()
        print(f"g = {g}: d p / d g error device {err_dev:.3e}, float32 restatement {err_f32:.3e}, scale {np.abs(ref).max():.3e}")
        assert err_dev <= 4 * err_f32 + 2.0 ** -22 * np.abs(ref).max()
    # the last g, 0.95: the forward peak (wo = +z, cos = -1 in eval_hg's convention) grows with g, the back falls
    assert out[-2] > 0 > out[-1]


# ---------------------------------------------------------------------------
# 2. single scattering, exact: central differences of the oracle's renders
# ---------------------------------------------------------------------------
SS_SEED = 11


@functools.lru_cache(maxsize=None)
def _fd_single(g, hom, w=8, h=8, spp=64):
    """(O.develop(O.render(g + 0.01)) - O.develop(O.render(g - 0.01))) / 0.02 at SS_SEED, float64, shared"""
    mi = _mi()
    imgs = []
    for s in (+1, -1):
        sc = mi.load_dict(_dict(mi, g + s * FD_STEP, w, h, spp, max_depth=2, sky=False, hom=hom))
        imgs.append(O.develop(O.render(sc, sc.integrator(), SS_SEED, spp)).astype(np.float64))
    fd = (imgs[0] - imgs[1]) / (2 * FD_STEP)
    fd.setflags(write=False)
    return fd


@pytest.mark.parametrize("engine", ["sched", "sample", "replay"])
@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("g", [0.5, 0.0, -0.7])
@pytest.mark.parametrize("hom", [False, True])
def test_single_scattering_backward(hom, g, deterministic, engine, monkeypatch):
    _engine(monkeypatch, engine)
    mi = _mi()
    scene = mi.load_dict(_dict(mi, g, max_depth=2, sky=False, hom=hom))
    fd = _fd_single(g, hom)
    gi = _grad_in(8, 8)
    want = (gi.astype(np.float64) * fd).sum()
    (got,) = _backward(mi, scene, [KEY], gi, SS_SEED, 64, deterministic=deterministic)
    print(f"hom={hom} g={g} det={deterministic} {engine}: got {got} want {want}")
    assert got.shape == (1,) and np.abs(fd).max() > 0
    np.testing.assert_allclose(got[0], want, rtol=RTOL, atol=1e-7 + 2e-4 * abs(want))


@pytest.mark.parametrize("g", [0.5, 0.0, -0.7])
@pytest.mark.parametrize("hom", [False, True])
def test_single_scattering_forward(hom, g):
    mi = _mi()
    scene = mi.load_dict(_dict(mi, g, max_depth=2, sky=False, hom=hom))
    fd = _fd_single(g, hom)
    for det in (False, True):
        img = _forward(mi, scene, SS_SEED, 64, deterministic=det)
        print(f"hom={hom} g={g} det={det}: max |forward - FD| {np.abs(img - fd).max():.3e} of {np.abs(fd).max():.3e}")
        np.testing.assert_allclose(img, fd, rtol=RTOL, atol=2e-4 * np.abs(fd).max())


@pytest.mark.parametrize("engine", ["sched", "sample", "replay"])
def test_single_scattering_odd_film(engine, monkeypatch):
    """5 x 3 at 2 spp: a partial wave and the non-coalesced splat"""
    _engine(monkeypatch, engine)
    mi = _mi()
    scene = mi.load_dict(_dict(mi, 0.5, 5, 3, 2, max_depth=2, sky=False))
    fd = _fd_single(0.5, False, 5, 3, 2)
    gi = _grad_in(3, 5)
    want = (gi.astype(np.float64) * fd).sum()
    for det in (False, True):
        (got,) = _backward(mi, scene, [KEY], gi, SS_SEED, 2, deterministic=det)
        print(f"5x3 {engine} det={det}: got {got} want {want}")
        np.testing.assert_allclose(got[0], want, rtol=RTOL, atol=1e-7 + 2e-4 * abs(want))
    img = _forward(mi, scene, SS_SEED, 2)
    assert np.abs(fd).max() > 0
    np.testing.assert_allclose(img, fd, rtol=RTOL, atol=2e-4 * np.abs(fd).max())


# ---------------------------------------------------------------------------
# 3. several media: the slot of each key, beside the hot medium
# ---------------------------------------------------------------------------
MEDIA_G = {"medium1": 0.5, "medium2": -0.4, "medium3": 0.3, "medium4": 0.6}


def _media_dict(mi, **g_of):
    """vol_cases.three_media without its floor, `hg` in all three, the sun only, and a fourth `hg` medium in a cube
    behind the camera that neither a camera ray (towards -z) nor a shadow ray (towards +y, +z from |y| < 2) reaches"""
    import vol_cases
    g = dict(MEDIA_G, **g_of)
    d = vol_cases.three_media(mi, "prbvolpath", 24, 20, 8, with_floor=False, max_depth=2)
    del d["sky"]
    for m in ("medium1", "medium2", "medium3"):
        d[m]["phase"] = {"type": "hg", "g": g[m]}
    T = mi.Transform4f
    d["medium4"] = {"type": "homogeneous", "sigma_t": 1.0, "scale": 1.0, "albedo": 0.5,
                    "phase": {"type": "hg", "g": g["medium4"]}}
    d["cube4"] = {"type": "cube", "to_world": T.translate([0.0, -6.0, 12.0]) @ T.scale([0.3, 0.3, 0.3]),
                  "bsdf": {"type": "null"}, "interior": {"type": "ref", "id": "medium4"}}
    return d


def test_several_media():
    mi = _mi()
    scene = mi.load_dict(_media_dict(mi))
    keys = [m + ".phase_function.g" for m in ("medium3", "medium1", "medium4", "medium2")]   # not in medium order
    gi = _grad_in(20, 24)
    got = dict(zip(keys, _backward(mi, scene, keys, gi, SS_SEED, 8)))
    det = dict(zip(keys, _backward(mi, scene, keys, gi, SS_SEED, 8, deterministic=True)))
    for m in ("medium1", "medium2", "medium3"):
        imgs = []
        for s in (+1, -1):
            sc = mi.load_dict(_media_dict(mi, **{m: MEDIA_G[m] + s * FD_STEP}))
            imgs.append(O.develop(O.render(sc, sc.integrator(), SS_SEED, 8)).astype(np.float64))
        want = (gi.astype(np.float64) * (imgs[0] - imgs[1]) / (2 * FD_STEP)).sum()
        k = m + ".phase_function.g"
        print(f"{k}: got {got[k]} deterministic {det[k]} want {want}")
        assert want != 0
        for a in (got[k], det[k]):
            np.testing.assert_allclose(a[0], want, rtol=RTOL, atol=1e-7 + 2e-4 * abs(want))
    assert got["medium4.phase_function.g"][0] == 0.0 and det["medium4.phase_function.g"][0] == 0.0


# ---------------------------------------------------------------------------
# 4. + 5. multiple scattering: the bookkeeping
# ---------------------------------------------------------------------------
MS_SEED, MS_SPP = 3, 64


def test_multiple_scattering_bookkeeping(monkeypatch):
    mi = _mi()
    scene = mi.load_dict(_dict(mi, 0.5))   # max_depth 8, rr_depth 5, sky and sun
    gi = _grad_in(8, 8)

    def run(**kw):
        return _backward(mi, scene, [KEY], gi, MS_SEED, MS_SPP, **kw)[0][0]

    ref = run()
    assert ref != 0
    tol = dict(rtol=RTOL, atol=1e-7 + 2e-4 * abs(ref))
    d1, d2 = run(deterministic=True), run(deterministic=True)
    print(f"default {ref}, deterministic {d1} {d2}")
    assert d1 == d2
    np.testing.assert_allclose(d1, ref, **tol)
    for var, val in (("MH_PVP_SCHED", "0"), ("MH_PVP_NEE_LOG", "0"), ("MH_PVP_SINGLE", "0"), ("MH_PVP_MAIN_CAP", "2"),
                     ("MH_PVP_NEE_CAP", "1")):
        with monkeypatch.context() as m:
            m.setenv(var, val)
            a, b = run(), run(deterministic=True)
        print(f"{var}={val}: {a}, deterministic {b}")
        np.testing.assert_allclose(a, ref, err_msg=var, **tol)
        np.testing.assert_allclose(b, ref, err_msg=var, **tol)
    lo, hi = (_backward(mi, scene, [KEY], gi, MS_SEED, MS_SPP, spp_begin=a, spp_end=b)[0][0] for a, b in ((0, 32), (32, 64)))
    print(f"slabs {lo} + {hi} = {lo + hi}")
    np.testing.assert_allclose(lo + hi, ref, **tol)

    # 5. the adjoint identity: <render_forward's image, grad_in> is render_backward's scalar
    img = _forward(mi, scene, MS_SEED, MS_SPP)
    dot = (img.astype(np.float64) * gi).sum()
    print(f"<forward, grad_in> {dot}")
    np.testing.assert_allclose(dot, ref, **tol)


# ---------------------------------------------------------------------------
# 6. multiple scattering: the value, statistically
# ---------------------------------------------------------------------------
STAT_SPP = 16384


def test_multiple_scattering_value():
    """Sun only, max_depth 8, a 4 x 4 film, loss = the image mean, seeds 1..8.  G_s: the backward gradient; D_s(h):
    central differences of forward renders of freshly loaded scenes; R_s = (4 D_s(0.05) - D_s(0.10)) / 3.
    Required: |mean(G - R)| <= 4 stderr(G - R), paired, with stderr(R) and stderr(G) each <= 5 % of |mean R| (the
    reference's finite-difference threshold, test_ad_integrators.py).  On the CPU oracle R at 16,384 spp has mean
    -0.1267 and a relative standard error of 1.1 %.  Measured on the device at 16,384 spp (MI355X): mean R -0.12666
    with stderr 0.00135 (1.07 % of |mean R|), mean G -0.12609 with stderr 0.00041 (0.33 %), mean (G - R) 0.00057
    with stderr 0.00143; so 16,384 spp meets the condition for both, and G is the quieter of the two."""
    mi = _mi()
    gi = np.full((4, 4, 3), 1.0 / 48, np.float32)

    def mean_render(g, seed):
        sc = mi.load_dict(_dict(mi, g, 4, 4, STAT_SPP, sky=False))
        return float(mi.develop(sc, mi.render_film(sc, sc.integrator(), seed=seed, spp=STAT_SPP)).double().mean().cpu())

    scene = mi.load_dict(_dict(mi, 0.5, 4, 4, STAT_SPP, sky=False))
    G, R = [], []
    for s in range(1, 9):
        G.append(float(_backward(mi, scene, [KEY], gi, s, STAT_SPP)[0][0]))
        D = [(mean_render(0.5 + h, s) - mean_render(0.5 - h, s)) / (2 * h) for h in (0.05, 0.10)]
        R.append((4 * D[0] - D[1]) / 3)
    G, R = np.array(G), np.array(R)
    se = lambda x: x.std(ddof=1) / np.sqrt(x.size)
    print(f"G {G}\nR {R}\nmean G {G.mean():.5f} +- {se(G):.5f}, mean R {R.mean():.5f} +- {se(R):.5f}, "
          f"mean (G - R) {np.mean(G - R):.5f} +- {se(G - R):.5f}")
    assert se(R) <= 0.05 * abs(R.mean()) and se(G) <= 0.05 * abs(R.mean())
    assert abs(np.mean(G - R)) <= 4 * se(G - R)


# ---------------------------------------------------------------------------
# 7. the other keys are untouched
# ---------------------------------------------------------------------------
def test_other_keys_beside_g():
    mi = _mi()
    scene = mi.load_dict(_dict(mi, 0.5))
    gi = _grad_in(8, 8)
    keys = [SIGMA, ALBEDO, SUN, KEY]
    both = _backward(mi, scene, keys, gi, MS_SEED, MS_SPP)
    for k, a in zip(keys, both):
        (single,) = _backward(mi, scene, [k], gi, MS_SEED, MS_SPP)
        print(f"{k}: max |together - alone| {np.abs(a - single).max():.3e} of {np.abs(single).max():.3e}")
        assert np.abs(single).max() > 0
        np.testing.assert_allclose(a, single, rtol=RTOL, atol=_atol(single), err_msg=k)
    # a call without g: the kernels it ran before (profiles/phase_g_kres.txt), held to what the existing prbvolpath
    # tests hold them to -- the oracle's adjoint, test_prbvolpath_backward_parity's criterion -- and reproducible
    params = mi.traverse(scene)
    old = [SIGMA, ALBEDO]
    a = _backward(mi, scene, old, gi, MS_SEED, MS_SPP, deterministic=True)
    b = _backward(mi, scene, old, gi, MS_SEED, MS_SPP, deterministic=True)
    ref = O.render_backward(scene, scene.integrator(), MS_SEED, MS_SPP, gi, [params.param_id(k) for k in old],
                            [tuple(params[k].shape) for k in old])
    for k, x, y, r in zip(old, a, b, ref):
        assert np.array_equal(x, y), k
        np.testing.assert_allclose(x, r, rtol=2e-3, atol=_atol(r), err_msg=k)


# ---------------------------------------------------------------------------
# 8. update
# ---------------------------------------------------------------------------
def _det_render_and_backward(mi, scene, gi):
    film = mi.render_film(scene, scene.integrator(), seed=5, spp=16, deterministic=True).cpu().numpy()
    return film, _backward(mi, scene, [KEY, ALBEDO], gi, MS_SEED, 16, deterministic=True)


def test_update():
    mi = _mi()
    from mitsuba_hip import _abi as A
    gi = _grad_in(8, 8)
    scene = mi.load_dict(_dict(mi, 0.5))
    params = mi.traverse(scene)
    before = _det_render_and_backward(mi, scene, gi)     # (the device scene exists before the update)
    params[KEY] = 0.3
    params.update()
    film, grads = _det_render_and_backward(mi, scene, gi)
    fresh_film, fresh_grads = _det_render_and_backward(mi, mi.load_dict(_dict(mi, 0.3)), gi)
    assert np.array_equal(film, fresh_film) and not np.array_equal(film, before[0])
    for a, b in zip(grads, fresh_grads):
        assert np.array_equal(a, b)
    # a rejected value: an exception, and the host and device scene as they were
    params[KEY] = 1.0
    with pytest.raises(RuntimeError, match="asymmetry parameter must lie in the interval"):
        params.update()
    assert scene.medium(0).g == float(np.float32(0.3))
    assert np.array_equal(_det_render_and_backward(mi, scene, gi)[0], film)
    # the C entry point's own checks
    L, h = A.lib(), scene.handle(0)
    assert L.mh_scene_update_medium_phase(h, 1, 0.2) == A.MH_ERR_INVALID_ARGUMENT
    assert "medium index out of bounds" in L.mh_last_error().decode()
    for bad in (1.0, -1.0, float("nan")):
        assert L.mh_scene_update_medium_phase(h, 0, bad) == A.MH_ERR_INVALID_ARGUMENT
        assert MESSAGE in L.mh_last_error().decode()
    assert np.array_equal(_det_render_and_backward(mi, scene, gi)[0], film)
    for ph in ({"type": "isotropic"}, tab("b"), blend({"type": "hg", "g": 0.6}, {"type": "isotropic"}, 0.25)):
        d = _dict(mi, 0.5)
        d["medium1"]["phase"] = ph
        other = mi.load_dict(d)
        f0 = mi.render_film(other, other.integrator(), seed=5, spp=16, deterministic=True).cpu().numpy()
        assert L.mh_scene_update_medium_phase(other.handle(0), 0, 0.2) == A.MH_ERR_INVALID_ARGUMENT
        assert "not MH_PHASE_HG" in L.mh_last_error().decode()
        f1 = mi.render_film(other, other.integrator(), seed=5, spp=16, deterministic=True).cpu().numpy()
        assert np.array_equal(f0, f1) and np.abs(f1).max() > 0


# ---------------------------------------------------------------------------
# 9. torch autograd, the optimizers, forward_ad
# ---------------------------------------------------------------------------
def test_autograd_and_sgd_step(monkeypatch):
    """MH_DETERMINISTIC=1 makes both gradients fixed-point sums, so that "the same" can mean the same bits."""
    monkeypatch.setenv("MH_DETERMINISTIC", "1")
    mi = _mi()
    import torch
    from mitsuba_hip import _abi as A
    scene = mi.load_dict(_dict(mi, 0.5))
    integ = scene.integrator()
    params = mi.traverse(scene)
    lr = 0.5
    opt = mi.ad.SGD(lr=lr)
    opt[KEY] = params[KEY]
    params.update(opt)
    img = mi.render(scene, params, integrator=integ, seed=MS_SEED, spp=MS_SPP)
    img.mean().backward()
    assert opt[KEY].grad is not None and tuple(opt[KEY].grad.shape) == (1,)
    sg = mi.sample_tea_32(MS_SEED, 1)[0]
    gi = torch.full(tuple(img.shape), 1.0 / img.numel(), dtype=torch.float32, device="cuda")
    (ref,) = mi.render_backward(scene, mi.traverse(scene), gi, [KEY], integ, seed=sg, spp=MS_SPP)
    grad = opt[KEY].grad.cpu().numpy()
    print(f"autograd {grad} direct {ref.cpu().numpy()}")
    assert grad[0] != 0 and np.array_equal(grad, ref.cpu().numpy())
    # one SGD step moves the device scene's g by lr * grad
    old = opt[KEY].detach().cpu().numpy().copy()
    opt.step()
    new = opt[KEY].detach().cpu().numpy()
    np.testing.assert_allclose(new, old - lr * grad, rtol=1e-6)
    assert new[0] != old[0] and -1 < new[0] < 1
    params.update(opt)
    assert scene.medium(0).g == float(new[0])
    wo = np.ascontiguousarray(np.float32([[0.0, 0.6], [0.0, 0.0], [1.0, 0.8]]))
    fresh = mi.load_dict(_dict(mi, float(new[0])))
    vals = []
    for sc in (scene, fresh):
        v = np.zeros(2, np.float32)
        A.check(A.lib().mh_phase_eval(sc.handle(0), 0, 2, _p(wo), _p(v), 0))
        vals.append(v)
    assert np.array_equal(vals[0], vals[1])


def test_forward_ad():
    mi = _mi()
    import torch
    import torch.autograd.forward_ad as fwAD
    scene = mi.load_dict(_dict(mi, 0.5))
    integ = scene.integrator()
    params = mi.traverse(scene)
    tan = torch.ones(1)
    with fwAD.dual_level():
        params[KEY] = fwAD.make_dual(params[KEY].detach(), tan.to(params[KEY].device))
        img = mi.render(scene, params, integrator=integ, spp=MS_SPP, seed=2)
        _, jvp = fwAD.unpack_dual(img)
    assert jvp is not None
    sg = mi.sample_tea_32(2, 1)[0]
    ref = mi.render_forward(scene, mi.traverse(scene), {KEY: tan}, integ, seed=sg, spp=MS_SPP).cpu().numpy()
    assert np.abs(ref).max() > 0
    np.testing.assert_allclose(jvp.cpu().numpy(), ref, rtol=1e-6, atol=1e-7)


# ---------------------------------------------------------------------------
# 10. still refused
# ---------------------------------------------------------------------------
def _raw_backward(scene, ids, integ=None):
    from mitsuba_hip import _abi as A
    L = A.lib()
    gi = _grad_in(scene.height, scene.width)
    grads = [np.zeros(3, np.float32) for _ in ids]
    ptrs = (C.c_void_p * len(ids))(*[g.ctypes.data for g in grads])
    ic = (integ or scene.integrator()).c()
    rc = L.mh_render_backward(scene.handle(0), C.byref(ic), MS_SEED, 4, 0, 0, _p(gi), None, len(ids),
                              (C.c_uint32 * len(ids))(*ids), ptrs, 0, None)
    return rc, L.mh_last_error().decode(), grads


def test_still_refused():
    mi = _mi()
    from mitsuba_hip import _abi as A
    G = A.PARAM_MEDIUM_PHASE_G
    bl = blend({"type": "hg", "g": 0.6}, tab("b"), 0.25)
    for ph in ({"type": "isotropic"}, tab("b"), bl):
        d = _dict(mi, 0.5)
        d["medium1"]["phase"] = ph
        scene = mi.load_dict(d)
        params = mi.traverse(scene)
        assert KEY not in params
        for k in params.keys():
            if ".phase_function." in k:
                with pytest.raises(A.MitsubaHipError, match="not differentiable"):
                    params.param_id(k)
        rc, msg, _ = _raw_backward(scene, [G | 0])
        assert rc == A.MH_ERR_UNSUPPORTED and "MH_PHASE_HG" in msg, ph["type"]
        # ... and the scene stays usable
        rc, _, grads = _raw_backward(scene, [params.param_id(ALBEDO)])
        assert rc == A.MH_OK and np.abs(grads[0]).max() > 0
        out = np.zeros(2, np.float32)
        wo = np.ascontiguousarray(np.float32([[0.0, 0.6], [0.0, 0.0], [1.0, 0.8]]))
        assert A.lib().mh_phase_eval_grad(scene.handle(0), 0, 2, _p(wo), _p(out), 0) == A.MH_ERR_UNSUPPORTED
    # an `hg` medium: the index and the integrator are checked, and the scene stays usable
    scene = mi.load_dict(_dict(mi, 0.5))
    rc, msg, _ = _raw_backward(scene, [G | 1])
    assert rc == A.MH_ERR_INVALID_ARGUMENT and "medium index out of bounds" in msg
    rc, msg, _ = _raw_backward(scene, [G | 0, G | 0])
    assert rc == A.MH_ERR_INVALID_ARGUMENT and "duplicate parameter" in msg
    rc, msg, _ = _raw_backward(scene, [G | 0], mi.load_dict({"type": "prb", "max_depth": 4}))
    assert rc == A.MH_ERR_UNSUPPORTED and "prbvolpath" in msg
    rc, _, grads = _raw_backward(scene, [G | 0])
    assert rc == A.MH_OK and grads[0][0] != 0 and grads[0][1] == 0 and grads[0][2] == 0
