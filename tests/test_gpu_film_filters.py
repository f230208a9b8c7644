"""GPU parity of the film reconstruction filters other than the default
Gaussian (stddev 0.5, radius 2.0): the HIP path through the C-ABI vs the CPU
oracle, forward (the splat) and backward (gather_dL, the splat's adjoint).

  box              radius 0.5   box branch
  gaussian 0.3     radius 1.2   generic, 3 taps per axis
  gaussian 0.625   radius 2.5   upper edge of the 5-tap fast kernels
  gaussian 0.75    radius 3.0   generic, 7 taps
  gaussian 1.0     radius 4.0   generic, 9 taps

spp 2 takes the non-coalesced footprint (imageblock.cpp:264-409), spp 8 the
coalesced one (imageblock.cpp:418-531); 20 x 12 films, and 5 x 3 where the
wide footprints overhang every border at once.

Criteria are the suite's own: film |d| <= 1e-4 max(1, |ref|) on >= 99.5 % of
the pixels, W image rtol 1e-5, gradients rtol 1e-3 (bitmaps and prbvolpath
2e-3 with their atol), forward images by test_gpu_forward._close, and the
adjoint identity <grad_in, render_forward(t)> = <render_backward(grad_in), t>
within 2e-3 -- the last needs no oracle.
"""
import numpy as np
import pytest

import oracle_py as O
from test_gpu_forward import _close

pytestmark = pytest.mark.gpu

FILTERS = {"box": {"type": "box"},
           "g0.3": {"type": "gaussian", "stddev": 0.3},
           "g0.625": {"type": "gaussian", "stddev": 0.625},
           "g0.75": {"type": "gaussian", "stddev": 0.75},
           "g1.0": {"type": "gaussian", "stddev": 1.0}}
RADIUS = {"box": 0.5, "g0.3": 1.2, "g0.625": 2.5, "g0.75": 3.0, "g1.0": 4.0}
SIZES = [(20, 12), (5, 3)]
KEY = "white.reflectance.value"
MAX_DEPTH = 5


def _mi():
    import mitsuba_hip as mi
    if not mi.is_available():
        pytest.fail("no HIP device / native library: the GPU tests need an MI355X")
    mi.set_variant("hip_ad_rgb")
    return mi


def _cbox(mi, rf, w, h, spp, bitmap=False):
    d = mi.cornell_box_bitmap(tex_res=8, width=w, height=h, spp=spp) if bitmap else mi.cornell_box()
    d["sensor"]["film"].update(width=w, height=h, rfilter=dict(FILTERS[rf]))
    d["sensor"]["sampler"]["sample_count"] = spp
    scene = mi.load_dict(d)
    assert abs(scene.desc.sensor.rfilter_radius - RADIUS[rf]) < 1e-6
    return scene


def _grad_in(w, h, seed=2):
    return np.random.default_rng(seed).random((h, w, 3)).astype(np.float32) / (h * w * 3)


_refs = {}


def _ref(name, fn):
    """Oracle results, computed once per case and shared (never modified)."""
    if name not in _refs:
        r = fn()
        for a in (r if isinstance(r, list) else [r]):
            a.setflags(write=False)
        _refs[name] = r
    return _refs[name]


def _film_close(a, b, frac=0.995):
    ok = np.all(np.abs(a - b) <= 1e-4 * np.maximum(1.0, np.abs(b)), axis=-1)
    return ok.mean() >= frac, ok.mean()


CASES = [(rf, spp, size) for rf in FILTERS for spp in (2, 8) for size in SIZES]
_ids = lambda c: f"{c[0]}-spp{c[1]}-{c[2][0]}x{c[2][1]}"


# the megakernel at 20 x 12 only
FILM_CASES = [(c, m) for c in CASES for m in ("auto", "mega") if m == "auto" or c[2] == SIZES[0]]


@pytest.mark.parametrize("case,mode", FILM_CASES, ids=lambda v: v if isinstance(v, str) else _ids(v))
def test_film_parity(case, mode):
    rf, spp, (w, h) = case
    mi = _mi()
    scene = _cbox(mi, rf, w, h, spp)
    integ = mi.load_dict({"type": "path", "max_depth": MAX_DEPTH})
    film = mi.render_film(scene, integ, seed=5, spp=spp, mode=mode).cpu().numpy()
    ref = _ref(("film", case), lambda: O.render(scene, integ, seed=5, spp=spp))
    assert ref[..., 3].min() > 0
    ok, frac = _film_close(film, ref)
    d = np.abs(film - ref) / np.maximum(1.0, np.abs(ref))
    print(f"film {rf} spp {spp} {w}x{h} {mode}: close {frac:.4f}, max rel {d.max():.3e}")
    assert ok, f"film parity {frac}"


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_weights_parity(case):
    rf, spp, (w, h) = case
    mi = _mi()
    scene = _cbox(mi, rf, w, h, spp)
    wt = mi.prb_weights(scene, seed=7, spp=spp).cpu().numpy()
    ref = _ref(("w", case), lambda: O.prb_weights(scene, 7, spp))
    assert ref.min() > 0
    np.testing.assert_allclose(wt, ref, rtol=1e-5, atol=1e-6)


def _prb(mi):
    return mi.load_dict({"type": "prb", "max_depth": MAX_DEPTH})


@pytest.mark.parametrize("mode", ["auto", "mega", "replay", "unfused"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_prb_gradient_parity(case, mode, monkeypatch):
    """auto: the fused wavefront (k_wf_bounce_prb); unfused: auto with
    MH_WF_FUSED=0; mega / replay: the per-sample kernels.  All reach
    gather_dL; at spp 8 with its coalesced footprint."""
    rf, spp, (w, h) = case
    if mode == "unfused":
        monkeypatch.setenv("MH_WF_FUSED", "0")
        mode = "auto"
    mi = _mi()
    import torch
    scene = _cbox(mi, rf, w, h, spp)
    integ = _prb(mi)
    params = mi.traverse(scene)
    gi = _grad_in(w, h)
    g = mi.render_backward(scene, params, torch.from_numpy(gi).cuda(), [KEY], integ, seed=11, spp=spp,
                           mode=mode)[0].cpu().numpy()
    ref = _ref(("grad", case), lambda: O.render_backward(scene, integ, 11, spp, gi, [params.texture_of(KEY)],
                                                         [(3,)]))[0]
    assert np.abs(ref).min() > 0
    print(f"grad {rf} spp {spp} {w}x{h}: max rel err {np.abs(g / ref - 1).max():.3e}")
    np.testing.assert_allclose(g, ref, rtol=1e-3, atol=1e-7)


@pytest.mark.parametrize("rf", ["g1.0", "box"])
def test_prb_bitmap_gradient_parity(rf):
    mi = _mi()
    import torch
    w, h, spp = SIZES[0] + (8,)
    scene = _cbox(mi, rf, w, h, spp, bitmap=True)
    integ = _prb(mi)
    params = mi.traverse(scene)
    key = "white.reflectance.data"
    gi = _grad_in(w, h)
    g = mi.render_backward(scene, params, torch.from_numpy(gi).cuda(), [key], integ, seed=13,
                           spp=spp)[0].cpu().numpy()
    ref = O.render_backward(scene, integ, 13, spp, gi, [params.texture_of(key)], [tuple(params[key].shape)])[0]
    assert g.shape == ref.shape and np.abs(ref).max() > 0
    print(f"bitmap grad {rf}: max |d| / max |ref| {np.abs(g - ref).max() / np.abs(ref).max():.3e}")
    np.testing.assert_allclose(g, ref, rtol=2e-3, atol=1e-9 + 2e-4 * np.abs(ref).max())


def test_prbvolpath_gradient_parity_wide_filter():
    """prbvolpath's backward (bw.coalesce, gather_dL_wave) under the 9-tap
    Gaussian: sigma_t grid, albedo and floor reflectance vs the oracle."""
    mi = _mi()
    import torch
    d = mi.volume_cube(24, 20, 8, grid=mi.fbm_grid(16), scale=4.0)
    d["sensor"]["film"]["rfilter"] = dict(FILTERS["g1.0"])
    d["integrator"] = {"type": "prbvolpath", "max_depth": 6, "rr_depth": 5}
    T = mi.Transform4f
    d["floor"] = {"type": "rectangle",
                  "to_world": T.translate([0, -1.2, 0]) @ T.rotate([1, 0, 0], -90) @ T.scale([3, 3, 3]),
                  "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.6, 0.5, 0.4]}}}
    scene = mi.load_dict(d)
    assert abs(scene.desc.sensor.rfilter_radius - 4.0) < 1e-6
    integ = scene.integrator()
    params = mi.traverse(scene)
    keys = ["medium1.sigma_t.data", "medium1.albedo.value", "floor.bsdf.reflectance.value"]
    gi = np.random.default_rng(4).standard_normal((20, 24, 3)).astype(np.float32)
    g = mi.render_backward(scene, params, torch.from_numpy(gi).cuda(), keys, integ, seed=7, spp=8)
    ref = O.render_backward(scene, integ, 7, 8, gi, [params.param_id(k) for k in keys],
                            [tuple(params[k].shape) for k in keys])
    for k, a, b in zip(keys, g, ref):
        a = a.cpu().numpy()
        assert a.shape == b.shape and np.abs(b).max() > 0, k
        print(f"prbvolpath {k}: max |d| / max |ref| {np.abs(a - b).max() / np.abs(b).max():.3e}")
        np.testing.assert_allclose(a, b, rtol=2e-3, atol=1e-7 + 2e-4 * np.abs(b).max(), err_msg=k)


@pytest.mark.parametrize("rf", list(FILTERS))
def test_adjoint_identity(rf):
    """The forward image dotted with grad_in equals the backward gradient
    dotted with the tangent: the splat (forward) and gather_dL (backward)
    are adjoint for every filter."""
    mi = _mi()
    import torch
    w, h, spp = SIZES[0] + (8,)
    scene = _cbox(mi, rf, w, h, spp)
    integ = _prb(mi)
    params = mi.traverse(scene)
    tan = np.array([0.7, -0.3, 1.1], np.float32)
    img = mi.render_forward(scene, params, {KEY: torch.from_numpy(tan).cuda()}, integ, seed=3, spp=spp).cpu().numpy()
    gi = _grad_in(w, h, seed=1)
    g = mi.render_backward(scene, params, torch.from_numpy(gi).cuda(), [KEY], integ, seed=3, spp=spp)[0]
    lhs = float((gi.astype(np.float64) * img).sum())
    rhs = float((g.cpu().numpy().astype(np.float64) * tan).sum())
    print(f"adjoint {rf}: lhs {lhs:.6e} rhs {rhs:.6e} rel {abs(lhs - rhs) / abs(rhs):.3e}")
    assert abs(lhs - rhs) <= 2e-3 * abs(rhs), (lhs, rhs)


@pytest.mark.parametrize("rf", ["box", "g1.0"])
def test_render_forward_parity(rf):
    mi = _mi()
    import torch
    w, h, spp = SIZES[0] + (8,)
    scene = _cbox(mi, rf, w, h, spp)
    integ = _prb(mi)
    params = mi.traverse(scene)
    tans = {KEY: np.array([1.0, -0.5, 0.25], np.float32), "red.reflectance.value": np.array([0.3, 0.2, 0.1], np.float32)}
    img = mi.render_forward(scene, params, {k: torch.from_numpy(v).cuda() for k, v in tans.items()}, integ,
                            seed=11, spp=spp).cpu().numpy()
    film = O.render_forward(scene, integ, 11, spp, [params.param_id(k) for k in tans], list(tans.values()))
    ref = O.develop(film, scene.desc.sensor.pixel_format)
    assert img.shape == ref.shape and np.abs(ref).max() > 0
    _close(img, ref)
