"""The oracle's bitmap lookup (tex_eval / bitmap_taps / wrap_index) against a
float64 numpy restatement written here from the definition, not from the C
text: the HIP bitmap_taps is the same text as the oracle's, so HIP == oracle
cannot catch a shared misreading of Texture2f (textures/bitmap.cpp:696-710).

  index wrap  floor-division arithmetic (repeat: i - floor(i / res) res;
              mirror: odd periods run backwards; clamp: clip)
  nearest     the texel at floor(u res)
  bilinear    four taps around u res - 0.5

Bounds: bilinear |d| <= 2e-5 -- the oracle forms fx = u' res - 0.5 in float32
with |fx| < 128, so an axis weight is off by up to one ulp(64..128) = 7.6e-6,
times texel differences <= 0.7, two axes.  nearest is exact except where the
float32 floor lands on the other side of a texel boundary: <= 0.1 % of the
points may differ, every other point is bit-equal.

The wrap-mode properties of the reference's own bitmap test
(tests/golden/known_answers.json "bitmap_wrap") are asserted on the oracle too.
"""
import json
import math
import os

import numpy as np
import pytest

import oracle_py as O

HERE = os.path.dirname(os.path.abspath(__file__))
KA = json.load(open(os.path.join(HERE, "golden", "known_answers.json")))["bitmap_wrap"]

SHAPES = [(8, 8, 3), (5, 7, 3), (1, 4, 1), (3, 1, 1)]
N_UV = 4000


def to_uv_transform(mi):
    T = mi.Transform4f
    return T.translate([-0.9, -0.6, 0.0]) @ T.rotate([0, 0, 1], 30.0) @ T.scale([2.7, 2.3, 1.0])


def _to_uv_rows():
    """translate(-0.9, -0.6) @ rotate_z(30 deg) @ scale(2.7, 2.3) as the 2 x 3
    affine map of (u, v, 1), entries rounded to float32 as the texture stores
    them."""
    c, s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    m = np.array([[2.7 * c, -2.3 * s, -0.9], [2.7 * s, 2.3 * c, -0.6]])
    return m.astype(np.float32).astype(np.float64)


def _scene(data, filt, wrap, to_uv):
    import mitsuba_hip as mi
    d = mi.cornell_box_bitmap(tex_res=8, width=8, height=8, spp=1)
    spec = {"type": "bitmap", "data": data, "filter_type": filt, "wrap_mode": wrap, "raw": True}
    if to_uv:
        spec["to_uv"] = to_uv_transform(mi)
    d["white"]["reflectance"] = spec
    scene = mi.load_dict(d)
    return scene, scene.params["white.reflectance.data"][1]


def _wrap(i, res, mode):
    if mode == "clamp":
        return np.clip(i, 0, res - 1)
    period = np.floor_divide(i, res)
    r = i - period * res
    if mode == "mirror":
        return np.where(period & 1, res - 1 - r, r)
    return r


def _reference(data, filt, wrap, uv, to_uv):
    data = data.astype(np.float64)
    H, W, _ = data.shape
    u, v = uv[:, 0].astype(np.float64), uv[:, 1].astype(np.float64)
    if to_uv:
        m = _to_uv_rows()
        u, v = m[0, 0] * u + m[0, 1] * v + m[0, 2], m[1, 0] * u + m[1, 1] * v + m[1, 2]
    if filt == "nearest":
        ix = _wrap(np.floor(u * W).astype(np.int64), W, wrap)
        iy = _wrap(np.floor(v * H).astype(np.int64), H, wrap)
        out = data[iy, ix]
    else:
        fx, fy = u * W - 0.5, v * H - 0.5
        x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
        wx, wy = (fx - x0)[:, None], (fy - y0)[:, None]
        xa, xb, ya, yb = _wrap(x0, W, wrap), _wrap(x0 + 1, W, wrap), _wrap(y0, H, wrap), _wrap(y0 + 1, H, wrap)
        out = (1 - wy) * ((1 - wx) * data[ya, xa] + wx * data[ya, xb]) + \
            wy * ((1 - wx) * data[yb, xa] + wx * data[yb, xb])
    return np.broadcast_to(out, (len(u), 3))  # one channel: r = g = b


@pytest.mark.parametrize("to_uv", [False, True], ids=["identity", "to_uv"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("wrap", ["repeat", "mirror", "clamp"])
@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
def test_tex_eval_vs_float64_reference(filt, wrap, shape, to_uv):
    rng = np.random.default_rng(sum(shape) * 7 + len(wrap))
    data = rng.uniform(0.2, 0.9, shape).astype(np.float32)
    uv = rng.uniform(-3.0, 4.0, (N_UV, 2)).astype(np.float32)
    scene, tex = _scene(data, filt, wrap, to_uv)
    got = O.tex_eval(scene, tex, uv)
    ref = _reference(data, filt, wrap, uv, to_uv)
    d = np.abs(got - ref).max(axis=1)
    if filt == "nearest":
        differ = got != ref.astype(np.float32)
        n_off = int(differ.any(axis=1).sum())
        print(f"nearest {wrap} {shape} to_uv={to_uv}: {n_off} of {N_UV} points differ")
        assert n_off <= N_UV // 1000, f"{n_off} of {N_UV} points pick another texel"
    else:
        print(f"bilinear {wrap} {shape} to_uv={to_uv}: max |d| {d.max():.3e}")
        assert d.max() <= 2e-5, f"max |d| {d.max():.3e} at uv {uv[d.argmax()]}"


def _grid(xr, yr, reverse):
    n = KA["axis_res"]
    x = np.linspace(xr[0], xr[1], n, dtype=np.float32)
    y = np.linspace(yr[0], yr[1], n, dtype=np.float32)
    if reverse:
        x, y = x[::-1], y[::-1]
    xv, yv = np.meshgrid(x, y)  # x runs fastest, as dr.meshgrid
    return np.stack([xv.ravel(), yv.ravel()], axis=1)


@pytest.mark.parametrize("wrap", ["repeat", "clamp", "mirror"])
def test_wrap_mode_properties(wrap):
    """repeat: f(uv - 1) = f(uv) = f(uv + 1); clamp: outside [0, 1] the edge
    row / column; mirror: f(-uv) = f(uv) = f(2 - uv).  Ranges, grid size and
    atol from the reference's test (provenance in known_answers.json)."""
    n = KA["axis_res"]
    data = np.random.default_rng(11).uniform(0.2, 0.9, (8, 8, 3)).astype(np.float32)
    scene, tex = _scene(data, "bilinear", wrap, False)
    ref = O.tex_eval(scene, tex, _grid(KA["ref"]["x"], KA["ref"]["y"], False)).reshape(n, n, 3)
    assert ref.std() > 0.05
    assert len(KA[wrap]) >= 2
    for case in KA[wrap]:
        got = O.tex_eval(scene, tex, _grid(case["x"], case["y"], case["reversed"])).reshape(n, n, 3)
        want = ref
        if "equals" in case:
            i = case["equals"]["index"]
            want = ref[i:i + 1 or None] if case["equals"]["axis"] == "row" else ref[:, i:i + 1 or None]
            want = np.broadcast_to(want, ref.shape)
        d = np.abs(got - want).max()
        print(f"{wrap} {case['name']}: max |d| {d:.3e}")
        assert d <= case["atol"], (case["name"], case["source"], d)
