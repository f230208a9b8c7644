"""GPU: emitter radiance as a differentiable, updatable parameter (prb,
prbvolpath, forward mode) through the C-ABI, checked against the CPU oracle.

The identity the tests rest on.  At a fixed seed the emitter choice is uniform
(scene.cpp:227-250) and throughput, Russian roulette and every sampling
decision are independent of the emitters' radiance, so the film is exactly
linear in each emitter's radiance, with the same paths.  Let U(e, c) be the
scene with emitter e's radiance set to the unit vector of channel c and every
other emitter's radiance set to 0, and I(e, c) = develop(render(U(e, c))) the
oracle's PRIMAL render of it.  Then

    render_backward:  grad[e][c] = sum_px grad_in[px, c] * I(e, c)[px, c]
    render_forward with tangent e_c on emitter e:  the image I(e, c)

The expected values come from the oracle's primal, never from the code under
test.  Tolerances are the project's own for gradients (DESIGN.md section 4,
tests/test_gpu_parity.py): rtol 1e-3, atol 1e-7 for gradient vectors; per-pixel
forward images (values O(0.01 - 1)) rtol 1e-3, atol 1e-6.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_py as O

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 24, 20, 8, 13
LIGHT, SKY, SUN = "light.emitter.radiance.value", "sky.radiance.value", "sun.irradiance.value"
EMITTERS = [LIGHT, SKY, SUN]
RTOL, ATOL = 1e-3, 1e-7


def _mi():
    import mitsuba_hip as mi
    if not mi.is_available():
        pytest.fail("no HIP device / native library: the GPU tests need an MI355X")
    mi.set_variant("hip_ad_rgb")
    return mi


# ---------------------------------------------------------------------------
# scenes: the three-emitter box of test_gpu_parity._cbox_lights (area light,
# constant sky, directional sun) with the back wall removed, so that sky and
# sun contribute; variants of it
# ---------------------------------------------------------------------------
def _box(mi, kind="lights"):
    d = mi.cornell_box_bitmap(tex_res=8, width=W, height=H, spp=SPP) if kind == "bitmap" else mi.cornell_box()
    d["sensor"]["film"]["width"], d["sensor"]["film"]["height"] = W, H
    d["sensor"]["sampler"]["sample_count"] = SPP
    if kind in ("lights", "sky"):
        d.pop("back")   # open box: camera rays escape to the sky, the sun shines in
        d["sky"] = {"type": "constant", "radiance": {"type": "rgb", "value": [0.3, 0.4, 0.5]}}
    if kind == "lights":
        d["sun"] = {"type": "directional", "direction": [0.2, -0.5, -1.0], "irradiance": {"type": "rgb", "value": 2.0}}
    return d


def _vol(mi):
    d = mi.volume_cube(width=16, height=12, spp=4, grid=mi.fbm_grid(8))
    d["integrator"]["type"] = "prbvolpath"
    return d


def _integ(mi, name):
    return mi.load_dict({"prb": {"type": "prb", "max_depth": 6},
                         "prb_hide": {"type": "prb", "max_depth": 6, "hide_emitters": True},
                         "path": {"type": "path", "max_depth": 6}}[name])


def _emitter_keys(scene):
    return [k for k, (kind, _) in scene.params.items() if kind == "emitter_radiance"]


@functools.lru_cache(maxsize=None)
def _basis(kind, integ_name, seed, spp):
    """I(e, c) of every emitter of the scene, from the oracle's primal render:
    {key: (3, H, W, 3) float64}.  Computed once per scene and shared."""
    mi = _mi()
    scene = mi.load_dict(_vol(mi) if kind == "vol" else _box(mi, kind))
    integ = scene.integrator() if kind == "vol" else _integ(mi, integ_name)
    out = {}
    for k in _emitter_keys(scene):
        e = scene.params[k][1]
        imgs = []
        for c in range(3):
            for j in range(scene.desc.n_emitters):
                scene.emitter(j).radiance[:] = [0.0, 0.0, 0.0]
            scene.emitter(e).radiance[c] = 1.0
            imgs.append(O.develop(O.render(scene, integ, seed, spp)).astype(np.float64))
        out[k] = np.stack(imgs)
        out[k].setflags(write=False)
    return out


def _grad_in(h=H, w=W):
    """a fixed non-uniform upstream gradient"""
    return (np.random.default_rng(7).random((h, w, 3)) / (h * w * 3)).astype(np.float32)


def _expected(I, gi):
    return np.array([(gi[..., c].astype(np.float64) * I[c][..., c]).sum() for c in range(3)])


def _check_emitters(g, keys, basis, gi, msg=""):
    for k, a in zip(keys, g):
        if k not in basis:
            continue
        a = a.cpu().numpy()
        want = _expected(basis[k], gi)
        print(f"{msg} {k}: got {a} want {want}")
        assert a.shape == (3,)
        np.testing.assert_allclose(a, want, rtol=RTOL, atol=ATOL, err_msg=f"{msg} {k}")


def _backward(mi, scene, params, keys, integ, gi, seed=SEED, spp=SPP, **kw):
    import torch
    return mi.render_backward(scene, params, torch.from_numpy(gi).cuda(), keys, integ, seed=seed, spp=spp, **kw)


# ---------------------------------------------------------------------------
# 1. the scene: every basis image carries energy, so no check below is vacuous
# ---------------------------------------------------------------------------
def test_basis_images_are_not_empty():
    for kind, integ in (("lights", "prb"), ("sky", "prb_hide"), ("bitmap", "prb")):
        basis = _basis(kind, integ, SEED, SPP)
        assert set(basis) == {"lights": set(EMITTERS), "sky": {LIGHT, SKY}, "bitmap": {LIGHT}}[kind]
        for k, I in basis.items():
            for c in range(3):
                assert I[c][..., c].sum() > 0, (kind, k, c)
                # emitter e's channel c reaches the film's channel c only
                assert np.all(np.delete(I[c], c, axis=-1) == 0), (kind, k, c)
    vol = _basis("vol", "", 7, 4)
    assert set(vol) == {SKY, SUN}
    for k, I in vol.items():
        for c in range(3):
            assert I[c][..., c].sum() > 0, ("vol", k, c)


# ---------------------------------------------------------------------------
# 2. backward, every engine
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("mode", ["auto", "mega", "replay"])
def test_backward_three_emitters(mode, deterministic):
    """auto: the fused wavefront (k_wf_bounce_prb<4, ., ., Det, Em>); mega:
    prb_fused; replay: prb_sample<Grad, Em>."""
    mi = _mi()
    from mitsuba_hip import _abi as A
    scene = mi.load_dict(_box(mi))
    params = mi.traverse(scene)
    gi = _grad_in()
    st = A.Stats()
    g = _backward(mi, scene, params, EMITTERS, _integ(mi, "prb"), gi, mode=mode, deterministic=deterministic,
                  stats=st)
    assert st.mode == (1 if mode == "auto" else 0)
    _check_emitters(g, EMITTERS, _basis("lights", "prb", SEED, SPP), gi, f"{mode} det={deterministic}")
    if deterministic:
        g2 = _backward(mi, scene, params, EMITTERS, _integ(mi, "prb"), gi, mode=mode, deterministic=True)
        for a, b in zip(g, g2):
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())


@pytest.mark.parametrize("deterministic,unfused", [(False, False), (True, False), (False, True)])
def test_backward_light_alone(deterministic, unfused, monkeypatch):
    """One emitter parameter and nothing else: the NR == 1 instances (with the
    NEE ring when not deterministic); unfused: k_wf_shade_prb / k_wf_shadow_prb
    (the deterministic per-path sums exist on the fused wavefront only)."""
    if unfused:
        monkeypatch.setenv("MH_WF_FUSED", "0")
    mi = _mi()
    scene = mi.load_dict(_box(mi))
    params = mi.traverse(scene)
    gi = _grad_in()
    g = _backward(mi, scene, params, [LIGHT], _integ(mi, "prb"), gi, deterministic=deterministic)
    _check_emitters(g, [LIGHT], _basis("lights", "prb", SEED, SPP), gi, "alone")


@pytest.mark.parametrize("mode", ["auto", "mega", "replay"])
def test_backward_reflectance_and_light(mode):
    """A reflectance beside the light: its gradient is still the oracle's."""
    mi = _mi()
    scene = mi.load_dict(_box(mi))
    params = mi.traverse(scene)
    keys = ["white.reflectance.value", LIGHT]
    gi = _grad_in()
    integ = _integ(mi, "prb")
    g = _backward(mi, scene, params, keys, integ, gi, mode=mode)
    ref = O.render_backward(scene, integ, SEED, SPP, gi, [params.texture_of(keys[0])], [(3,)])[0]
    assert np.abs(ref).max() > 0
    np.testing.assert_allclose(g[0].cpu().numpy(), ref, rtol=RTOL, atol=ATOL)
    _check_emitters(g, keys, _basis("lights", "prb", SEED, SPP), gi, mode)


@pytest.mark.parametrize("mode", ["auto", "replay"])
def test_backward_bitmap_and_light(mode):
    """A bitmap reflectance and the light together (auto: the Bm instance and
    the texel scatter; replay: the per-lane kernel)."""
    mi = _mi()
    from mitsuba_hip import _abi as A
    scene = mi.load_dict(_box(mi, "bitmap"))
    params = mi.traverse(scene)
    keys = ["white.reflectance.data", LIGHT]
    gi = _grad_in()
    integ = _integ(mi, "prb")
    st = A.Stats()
    g = _backward(mi, scene, params, keys, integ, gi, mode=mode, stats=st)
    assert st.mode == (1 if mode == "auto" else 0)
    ref = O.render_backward(scene, integ, SEED, SPP, gi, [params.texture_of(keys[0])],
                            [tuple(params[keys[0]].shape)])[0]
    # the bitmap criterion of test_prb_backward_bitmap_parity
    np.testing.assert_allclose(g[0].cpu().numpy(), ref, rtol=2e-3, atol=1e-9 + 2e-4 * np.abs(ref).max())
    _check_emitters(g, keys, _basis("bitmap", "prb", SEED, SPP), gi, f"bitmap {mode}")


def test_backward_sharded_sums_the_slabs():
    """mh_render_backward_sharded sums slots generically: two scenes on one
    device, each differentiating half of the samples of every pixel."""
    mi = _mi()
    import torch
    from mitsuba_hip.comm import render_backward_sharded
    scenes = [mi.load_dict(_box(mi)) for _ in range(2)]
    params = mi.traverse(scenes[0])
    gi = _grad_in()
    outs = render_backward_sharded(scenes, params, torch.from_numpy(gi).cuda(), EMITTERS, _integ(mi, "prb"), SEED, SPP)
    torch.cuda.synchronize()
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)   # the sum is copied to every scene
    _check_emitters(outs[0], EMITTERS, _basis("lights", "prb", SEED, SPP), gi, "sharded")


# ---------------------------------------------------------------------------
# 3. zero radiance: the derivative must not divide by the radiance
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["auto", "mega", "replay"])
def test_backward_at_zero_radiance(mode):
    mi = _mi()
    scene = mi.load_dict(_box(mi))
    params = mi.traverse(scene)
    scene.handle(0)
    params[LIGHT] = [0.0, 0.5, 0.0]
    params.update()
    gi = _grad_in()
    g = _backward(mi, scene, params, EMITTERS, _integ(mi, "prb"), gi, mode=mode)
    for a in g:
        assert np.all(np.isfinite(a.cpu().numpy()))
    _check_emitters(g, EMITTERS, _basis("lights", "prb", SEED, SPP), gi, f"zero {mode}")


# ---------------------------------------------------------------------------
# 4. hide_emitters: the depth-0 gate of the direct hit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["auto", "mega", "replay"])
def test_backward_hide_emitters(mode):
    mi = _mi()
    scene = mi.load_dict(_box(mi, "sky"))
    params = mi.traverse(scene)
    keys = [SKY, LIGHT]
    gi = _grad_in()
    basis = _basis("sky", "prb_hide", SEED, SPP)
    # the gate matters: camera rays that escape see the sky unless it is hidden
    seen = _basis("sky", "prb", SEED, SPP)
    assert _expected(seen[SKY], gi)[0] > 1.05 * _expected(basis[SKY], gi)[0]
    g = _backward(mi, scene, params, keys, _integ(mi, "prb_hide"), gi, mode=mode)
    _check_emitters(g, keys, basis, gi, f"hide {mode}")


# ---------------------------------------------------------------------------
# 5. update parity: an already created handle renders the updated radiance
# ---------------------------------------------------------------------------
def _gpu_samples(scene, integrator, seed, spp, flags=0):
    from mitsuba_hip import _abi as A
    n = scene.width * scene.height * spp
    out = np.zeros(5 * n, np.float32)
    ic = integrator.c()
    A.check(A.lib().mh_render_samples(scene.handle(0), C.byref(ic), seed, spp, 0, 0,
                                      out.ctypes.data_as(C.c_void_p), flags))
    return out[:3 * n].reshape(3, n).T


@pytest.mark.parametrize("itype,mode", [("path", "wavefront"), ("path", "mega"), ("prb", "mega")])
def test_update_parity_per_sample(itype, mode):
    mi = _mi()
    from mitsuba_hip import _abi as A
    scene = mi.load_dict(_box(mi))
    integ = _integ(mi, itype)
    flags = A.FLAG_WAVEFRONT if mode == "wavefront" else 0
    before = _gpu_samples(scene, integ, 5, SPP, flags)   # creates the handle
    params = mi.traverse(scene)
    params[SKY] = [1.5, 0.25, 0.75]
    params[SUN] = [0.5, 3.0, 1.0]
    params[LIGHT] = [4.0, 5.0, 6.0]
    params.update()
    L = _gpu_samples(scene, integ, 5, SPP, flags)
    rL, _, _ = O.sample_range(scene, integ, 5, SPP, 0, L.shape[0])   # the oracle reads the updated desc
    exact = np.all(L == rL, axis=1)
    assert exact.mean() >= 0.999, f"bit-exact fraction {exact.mean()}"
    assert rL.mean() > 0 and not np.array_equal(before, L)
    # and the film of the same handle
    film = mi.render_film(scene, integ, seed=5, spp=SPP, mode=mode).cpu().numpy()
    ref = O.render(scene, integ, 5, SPP)
    ok = np.all(np.abs(film - ref) <= 1e-4 * np.maximum(1.0, np.abs(ref)), axis=-1)
    assert ok.mean() >= 0.995


# ---------------------------------------------------------------------------
# 6. forward mode
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["auto", "mega"])
@pytest.mark.parametrize("key", [LIGHT, SUN])
def test_forward_is_the_basis_image(key, mode, monkeypatch):
    """auto: k_wf_bounce_fwd<., Em>; mega: k_render_forward (prb_forward)."""
    if mode == "mega":
        monkeypatch.setenv("MH_MODE", "mega")
    mi = _mi()
    from mitsuba_hip import _abi as A
    import torch
    scene = mi.load_dict(_box(mi))
    params = mi.traverse(scene)
    integ = _integ(mi, "prb")
    basis = _basis("lights", "prb", SEED, SPP)[key]
    for c in range(3):
        t = np.zeros(3, np.float32)
        t[c] = 1.0
        st = A.Stats()
        img = mi.render_forward(scene, params, {key: torch.from_numpy(t).cuda()}, integ, seed=SEED, spp=SPP,
                                stats=st).cpu().numpy()
        assert st.mode == (2 if mode == "auto" else 0)
        print(f"forward {key} c={c}: max |d| {np.abs(img - basis[c]).max():.3e}, max ref {basis[c].max():.3e}")
        np.testing.assert_allclose(img, basis[c], rtol=1e-3, atol=1e-6)


def test_forward_ad_through_render():
    mi = _mi()
    import torch
    import torch.autograd.forward_ad as fwAD
    scene = mi.load_dict(_box(mi))
    params = mi.traverse(scene)
    integ = _integ(mi, "prb")
    tan = torch.tensor([0.0, 1.0, 0.0])
    with fwAD.dual_level():
        params[SUN] = fwAD.make_dual(params[SUN].detach(), tan.to(params[SUN].device))
        img = mi.render(scene, params, integrator=integ, spp=SPP, seed=2)
        _, jvp = fwAD.unpack_dual(img)
    assert jvp is not None
    sg = mi.sample_tea_32(2, 1)[0]
    ref = mi.render_forward(scene, params, {SUN: tan}, integ, seed=sg, spp=SPP)
    np.testing.assert_allclose(jvp.cpu().numpy(), ref.cpu().numpy(), rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(jvp.cpu().numpy(), _basis("lights", "prb", sg, SPP)[SUN][1], rtol=1e-3, atol=1e-6)


# ---------------------------------------------------------------------------
# 7. torch autograd and the optimizers
# ---------------------------------------------------------------------------
def test_autograd_and_sgd_step():
    """mi.render under autograd with an emitter and a reflectance key.  The
    differential seed is render's default sample_tea_32(seed, 1)[0]: render
    refuses seed_grad == seed, as the reference does (util.py:590-593)."""
    mi = _mi()
    import torch
    scene = mi.load_dict(_box(mi))
    params = mi.traverse(scene)
    integ = _integ(mi, "prb")
    g = torch.from_numpy(_grad_in()).cuda()
    keys = [LIGHT, "white.reflectance.value"]
    opt = mi.ad.SGD(lr=50.0)          # the emitter key through the optimizer, as in mi.ad's loop
    opt[LIGHT] = params[LIGHT]
    params.update(opt)
    params[keys[1]].requires_grad_()
    loss = (mi.render(scene, params, integrator=integ, seed=SEED, spp=SPP) * g).sum()
    loss.backward()
    sg = mi.sample_tea_32(SEED, 1)[0]
    ref = mi.render_backward(scene, mi.traverse(scene), g, keys, integ, seed=sg, spp=SPP)
    for k, r in zip(keys, ref):
        assert params[k].grad is not None, k
        np.testing.assert_allclose(params[k].grad.cpu().numpy(), r.cpu().numpy(), rtol=1e-6, atol=1e-9)
    _check_emitters([params[LIGHT].grad], [LIGHT], _basis("lights", "prb", sg, SPP), g.cpu().numpy(), "autograd")

    # one SGD step on the emitter key changes the next render like any update
    old, step = opt[LIGHT].detach().cpu().numpy().copy(), 50.0 * opt[LIGHT].grad.cpu().numpy()
    opt.step()
    new = opt[LIGHT].detach().cpu().numpy()
    np.testing.assert_allclose(new, old - step, rtol=1e-6)
    assert not np.allclose(new, old)
    params.update(opt)
    i = scene.params[LIGHT][1]
    assert list(scene.desc.emitters[i].radiance) == pytest.approx(new.tolist(), rel=1e-6)
    film = mi.render_film(scene, integ, seed=3, spp=SPP).cpu().numpy()
    refilm = O.render(scene, integ, 3, SPP)
    ok = np.all(np.abs(film - refilm) <= 1e-4 * np.maximum(1.0, np.abs(refilm)), axis=-1)
    assert ok.mean() >= 0.995


# ---------------------------------------------------------------------------
# 8. prbvolpath: the constant sky and the directional sun over a medium
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["sched", "sample", "replay"])
@pytest.mark.parametrize("deterministic", [False, True])
def test_prbvolpath_sky_and_sun(deterministic, engine, monkeypatch):
    """sched: k_vol_sched<PvBwdMachineEm>; sample: the per-sample single pass
    (k_prbvol_backward, MH_PVP_SCHED=0); replay: primal + adjoint replay with
    the NEE walks replayed (MH_PVP_NEE_LOG=0)."""
    if engine == "sample":
        monkeypatch.setenv("MH_PVP_SCHED", "0")
    elif engine == "replay":
        monkeypatch.setenv("MH_PVP_NEE_LOG", "0")
    mi = _mi()
    scene = mi.load_dict(_vol(mi))
    integ = scene.integrator()
    assert integ.type == "prbvolpath"
    params = mi.traverse(scene)
    keys = [SKY, SUN, "medium1.albedo.value"]
    gi = _grad_in(scene.height, scene.width)
    g = _backward(mi, scene, params, keys, integ, gi, seed=7, spp=4, deterministic=deterministic)
    _check_emitters(g, keys, _basis("vol", "", 7, 4), gi, f"vol {engine} det={deterministic}")
    ref = O.render_backward(scene, integ, 7, 4, gi, [params.param_id(keys[2])], [(3,)])[0]
    assert np.abs(ref).max() > 0
    # the albedo criterion of test_prbvolpath_backward_parity
    np.testing.assert_allclose(g[2].cpu().numpy(), ref, rtol=2e-3, atol=1e-7 + 2e-4 * np.abs(ref).max())
    if deterministic:
        g2 = _backward(mi, scene, params, keys, integ, gi, seed=7, spp=4, deterministic=True)
        for a, b in zip(g, g2):
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())


def test_prbvolpath_forward_is_the_basis_image():
    mi = _mi()
    import torch
    scene = mi.load_dict(_vol(mi))
    integ = scene.integrator()
    params = mi.traverse(scene)
    basis = _basis("vol", "", 7, 4)
    for key, c in ((SKY, 2), (SUN, 0)):
        t = np.zeros(3, np.float32)
        t[c] = 1.0
        img = mi.render_forward(scene, params, {key: torch.from_numpy(t).cuda()}, integ, seed=7, spp=4).cpu().numpy()
        np.testing.assert_allclose(img, basis[key][c], rtol=1e-3, atol=1e-6)


# ---------------------------------------------------------------------------
# 9. errors: each is reported and leaves the scene usable
# ---------------------------------------------------------------------------
def _raw_backward(scene, integ, ids):
    from mitsuba_hip import _abi as A
    L = A.lib()
    gi = _grad_in()
    grads = [np.zeros(3, np.float32) for _ in ids]
    ptrs = (C.c_void_p * len(ids))(*[g.ctypes.data for g in grads])
    ic = integ.c()
    rc = L.mh_render_backward(scene.handle(0), C.byref(ic), SEED, SPP, 0, 0, gi.ctypes.data_as(C.c_void_p), None,
                              len(ids), (C.c_uint32 * len(ids))(*ids), ptrs, 0, None)
    return rc, L.mh_last_error().decode(), grads


def test_errors_leave_the_scene_usable():
    mi = _mi()
    from mitsuba_hip import _abi as A
    scene = mi.load_dict(_box(mi))
    params = mi.traverse(scene)
    integ = _integ(mi, "prb")
    E = A.PARAM_EMITTER_RADIANCE
    light, sky = params.param_id(LIGHT), params.param_id(SKY)

    def usable():
        rc, _, grads = _raw_backward(scene, integ, [light])
        assert rc == A.MH_OK
        np.testing.assert_allclose(grads[0], _expected(_basis("lights", "prb", SEED, SPP)[LIGHT], _grad_in()),
                                   rtol=RTOL, atol=ATOL)

    rc, msg, _ = _raw_backward(scene, integ, [E | 3])
    assert rc == A.MH_ERR_INVALID_ARGUMENT and "emitter index out of bounds" in msg
    usable()
    rc, msg, _ = _raw_backward(scene, integ, [light, sky, light])
    assert rc == A.MH_ERR_INVALID_ARGUMENT and "duplicate parameter" in msg
    usable()
    five = [params.param_id(k) for k in ("white.reflectance.value", "red.reflectance.value",
                                         "green.reflectance.value", LIGHT, SKY)]
    rc, msg, _ = _raw_backward(scene, integ, five)
    assert rc == A.MH_ERR_UNSUPPORTED and "too many rgb parameters" in msg
    usable()
    L = A.lib()
    v = (C.c_float * 3)(1.0, 2.0, 3.0)
    assert L.mh_scene_update_emitter(scene.handle(0), 3, v) == A.MH_ERR_INVALID_ARGUMENT
    assert "emitter index out of bounds" in L.mh_last_error().decode()
    assert L.mh_scene_update_emitter(scene.handle(0), 0, None) == A.MH_ERR_INVALID_ARGUMENT
    assert "NULL argument" in L.mh_last_error().decode()
    usable()
