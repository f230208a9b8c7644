"""GPU parity of the bitmap texture's filter and wrap modes and its to_uv
transform: `nearest` / `bilinear` x `repeat` / `mirror` / `clamp` under
translate(-0.9, -0.6) @ rotate_z(30 deg) @ scale(2.7, 2.3), which takes the
walls' uv to about [-2, 3.4]: negative texel indices and second periods.

The oracle these tests compare against is pinned independently of the shared
bitmap_taps text by tests/test_bitmap_oracle.py.

  per sample   `pos` equal, >= 99.9 % of the samples bit-exact, the rest 1e-4
  gradient     rtol 2e-3, atol 1e-9 + 2e-4 max |ref| (under clamp some texels
               are never sampled and have a zero gradient: the atol term)
  forward      test_gpu_forward._close, and the adjoint identity at 2e-3
"""
import ctypes as C

import numpy as np
import pytest

import oracle_py as O
from test_bitmap_oracle import to_uv_transform
from test_gpu_forward import _close

pytestmark = pytest.mark.gpu

KEY = "white.reflectance.data"
# (3, 1, 1): a one-texel-wide bitmap, where mirror and clamp fold every index
COMBOS = [(f, w, s) for f in ("nearest", "bilinear") for w in ("repeat", "mirror", "clamp")
          for s in ((5, 7, 3), (1, 4, 1)) + (((3, 1, 1),) if w != "repeat" else ())]
_ids = lambda c: f"{c[0]}-{c[1]}-{'x'.join(map(str, c[2]))}"


def _mi():
    import mitsuba_hip as mi
    if not mi.is_available():
        pytest.fail("no HIP device / native library: the GPU tests need an MI355X")
    mi.set_variant("hip_ad_rgb")
    return mi


def _scene(mi, combo, w=24, h=24, spp=8):
    filt, wrap, shape = combo
    d = mi.cornell_box_bitmap(tex_res=8, width=w, height=h, spp=spp)
    data = np.random.default_rng(sum(shape) + len(wrap)).uniform(0.2, 0.9, shape).astype(np.float32)
    d["white"]["reflectance"] = {"type": "bitmap", "data": data, "filter_type": filt, "wrap_mode": wrap, "raw": True,
                                 "to_uv": to_uv_transform(mi)}
    return mi.load_dict(d)


def _grad_in(w, h, seed):
    return np.random.default_rng(seed).random((h, w, 3)).astype(np.float32) / (h * w * 3)


_refs = {}


def _ref(name, fn):
    """Oracle results, computed once per case and shared (never modified)."""
    if name not in _refs:
        r = fn()
        for a in (r if isinstance(r, (list, tuple)) else [r]):
            a.setflags(write=False)
        _refs[name] = r
    return _refs[name]


@pytest.mark.parametrize("itype,mode", [("path", "wavefront"), ("path", "mega"), ("prb", "mega")])
@pytest.mark.parametrize("combo", COMBOS, ids=_ids)
def test_per_sample_parity(combo, itype, mode):
    mi = _mi()
    from mitsuba_hip import _abi as A
    scene = _scene(mi, combo)
    integ = mi.load_dict({"type": itype, "max_depth": 6})
    n = scene.width * scene.height * 8
    out = np.zeros(5 * n, np.float32)
    ic = integ.c()
    A.check(A.lib().mh_render_samples(scene.handle(0), C.byref(ic), 3, 8, 0, 0, out.ctypes.data_as(C.c_void_p),
                                      A.FLAG_WAVEFRONT if mode == "wavefront" else 0))
    L, pos = out[:3 * n].reshape(3, n).T, out[3 * n:].reshape(2, n).T
    rL, rpos, _ = _ref(("samples", combo, itype), lambda: O.sample_range(scene, integ, 3, 8, 0, n))
    np.testing.assert_array_equal(pos, rpos)
    exact = np.all(L == rL, axis=1)
    print(f"samples {_ids(combo)} {itype} {mode}: bit-exact {exact.mean():.5f}")
    assert exact.mean() >= 0.999, f"bit-exact fraction {exact.mean()}"
    close = np.all(np.abs(L - rL) <= 1e-4 * np.maximum(1, np.abs(rL)), axis=1)
    assert close.mean() >= 0.999


def _check_grad(g, ref, what):
    g = g.cpu().numpy()
    assert g.shape == ref.shape and np.abs(ref).max() > 0
    scale = np.abs(ref).max()
    print(f"grad {what}: max |d| / max |ref| {np.abs(g - ref).max() / scale:.3e}, "
          f"non-zero texels {np.mean(ref != 0):.2f}")
    np.testing.assert_allclose(g, ref, rtol=2e-3, atol=1e-9 + 2e-4 * scale)


def _oracle_grad(scene, integ, params, seed, spp, gi):
    return O.render_backward(scene, integ, seed, spp, gi, [params.texture_of(KEY)], [tuple(params[KEY].shape)])[0]


@pytest.mark.parametrize("mode", ["lds", "global", "replay", "chunks"])
@pytest.mark.parametrize("combo", COMBOS, ids=_ids)
def test_bitmap_gradient_parity(combo, mode, monkeypatch):
    """lds / global: the fused wavefront's texel scatter in LDS
    (MH_PRB_LDS_TEX=1) and as global atomics (=0); replay: the per-sample
    primal + adjoint kernel (tex_backward); chunks: five 4096-path chunks of
    a 40 x 32 film at 16 spp."""
    w, h, spp = (40, 32, 16) if mode == "chunks" else (24, 24, 8)
    if mode == "chunks":
        monkeypatch.setenv("MH_WF_CHUNK", "4096")
    elif mode != "replay":
        monkeypatch.setenv("MH_PRB_LDS_TEX", "1" if mode == "lds" else "0")
    mi = _mi()
    import torch
    from mitsuba_hip import _abi as A
    scene = _scene(mi, combo, w, h, spp)
    integ = mi.load_dict({"type": "prb", "max_depth": 6})
    params = mi.traverse(scene)
    gi = _grad_in(w, h, 2)
    st = A.Stats()
    g = mi.render_backward(scene, params, torch.from_numpy(gi).cuda(), [KEY], integ, seed=13, spp=spp,
                           mode="replay" if mode == "replay" else "auto", stats=st)[0]
    assert st.mode == (0 if mode == "replay" else 1), st.mode
    ref = _ref(("grad", combo, w), lambda: _oracle_grad(scene, integ, params, 13, spp, gi))
    if combo[1] != "clamp":
        assert np.all(ref != 0)  # repeat / mirror: every texel is reached
    _check_grad(g, ref, f"{_ids(combo)} {mode}")


@pytest.mark.parametrize("combo", [("nearest", "clamp", (5, 7, 3)), ("bilinear", "mirror", (5, 7, 3))], ids=_ids)
def test_bitmap_gradient_deterministic(combo):
    mi = _mi()
    import torch
    scene = _scene(mi, combo)
    integ = mi.load_dict({"type": "prb", "max_depth": 6})
    params = mi.traverse(scene)
    gi = _grad_in(24, 24, 2)
    runs = [mi.render_backward(scene, params, torch.from_numpy(gi).cuda(), [KEY], integ, seed=13, spp=8,
                               deterministic=True)[0] for _ in range(2)]
    assert torch.equal(runs[0], runs[1])
    ref = _ref(("grad", combo, 24), lambda: _oracle_grad(scene, integ, params, 13, 8, gi))
    _check_grad(runs[0], ref, f"{_ids(combo)} deterministic")


@pytest.mark.parametrize("mode", ["auto", "mega"])
@pytest.mark.parametrize("combo", [("nearest", "repeat", (5, 7, 3)), ("bilinear", "mirror", (5, 7, 3))], ids=_ids)
def test_render_forward_parity_and_adjoint(combo, mode, monkeypatch):
    """Random tangent texels: the forward image vs the oracle's, and against
    the backward gradient of the same seeded render (the gather through
    bitmap_taps and the scatter through it are adjoint)."""
    if mode == "mega":
        monkeypatch.setenv("MH_MODE", "mega")
    mi = _mi()
    import torch
    scene = _scene(mi, combo, 24, 24, 8)
    integ = mi.load_dict({"type": "prb", "max_depth": 6})
    params = mi.traverse(scene)
    rng = np.random.default_rng(3)
    tans = {KEY: rng.standard_normal(tuple(params[KEY].shape)).astype(np.float32),
            "green.reflectance.value": np.array([0.2, 0.9, -0.1], np.float32)}
    img = mi.render_forward(scene, params, {k: torch.from_numpy(v).cuda() for k, v in tans.items()}, integ,
                            seed=5, spp=8).cpu().numpy()
    film = _ref(("fwd", combo), lambda: O.render_forward(scene, integ, 5, 8, [params.param_id(k) for k in tans],
                                                         list(tans.values())))
    _close(img, O.develop(film, scene.desc.sensor.pixel_format))
    gi = _grad_in(24, 24, 6)
    g = mi.render_backward(scene, params, torch.from_numpy(gi).cuda(), list(tans), integ, seed=5, spp=8)
    lhs = float((gi.astype(np.float64) * img).sum())
    rhs = float(sum((a.cpu().numpy().astype(np.float64) * t).sum() for a, t in zip(g, tans.values())))
    print(f"adjoint {_ids(combo)} {mode}: lhs {lhs:.6e} rhs {rhs:.6e}")
    assert abs(lhs - rhs) <= 2e-3 * max(abs(rhs), 1e-12), (lhs, rhs)
