"""Blend phase function cases shared by the blendphase tests
(test_blend_phase_host.py, test_gpu_blend_phase.py): the child pairs, the
weight grids -- each with a to_world of its own, different from the medium's
box, and with values below 0 and above 1 so that the clamp works -- and the
numpy restatement of the weight lookup (grid.cpp: trilinear, clamp; then
blendphase.cpp:196-200's clamp to [0, 1]).  A plain helper module."""
import numpy as np

from phase_cases import TABLES


def tab(key):
    c, v = TABLES[key]
    return {"type": "tabphase", "cost": c, "values": v}


# the child pairs of the function-level tests
CHILD_PAIRS = {
    "iso_hg": ({"type": "isotropic"}, {"type": "hg", "g": 0.6}),
    "rayleigh_d": ({"type": "rayleigh"}, tab("d")),
    "b_e": (tab("b"), tab("e")),
}


def blend(child0, child1, weight):
    """The dictionary form: the children's names do not matter, their order does."""
    return {"type": "blendphase", "weight_0": weight, "first": dict(child0), "second": dict(child1)}


def _grid_to_world(mi, res):
    """Not the medium's box [-1, 1]^3: rotated, anisotropically scaled, shifted."""
    T = mi.Transform4f
    if res == (2, 3, 4):
        return T.translate([-1.3, -0.9, -1.2]) @ T.rotate([0, 1, 0], 20.0) @ T.scale([2.5, 2.0, 2.3])
    return T.translate([-0.8, -1.4, -1.0]) @ T.rotate([1, 0, 0], -15.0) @ T.scale([1.7, 2.6, 2.1])


def weight_grid(mi, res, seed=3):
    """A gridvolume of res = (x, y, z) texels, uniform in [-0.5, 1.5] (a quarter
    of the values below 0, a quarter above 1).  2x3x4 is non-cubic (an axis swap
    shows); 5x6x7 crosses 4^3 brick edges and has partial bricks."""
    x, y, z = res
    data = np.random.default_rng(seed).uniform(-0.5, 1.5, (z, y, x)).astype(np.float32)
    return {"type": "gridvolume", "data": data, "to_world": _grid_to_world(mi, res)}


def const_grid(mi, res, value):
    x, y, z = res
    return {"type": "gridvolume", "data": np.full((z, y, x), value, np.float32), "to_world": _grid_to_world(mi, res)}


def falling_grid(mi, n=8):
    """The weight of child 0 falling with height (y) from 0.9 to 0.1 over the cube, as an aerosol fraction does."""
    T = mi.Transform4f
    w = np.linspace(0.9, 0.1, n, dtype=np.float32)
    data = np.broadcast_to(w[None, :, None], (n, n, n)).astype(np.float32).copy()
    data += np.random.default_rng(1).uniform(-0.05, 0.05, data.shape).astype(np.float32)
    return {"type": "gridvolume", "data": data, "to_world": T.translate([-1.0, -1.0, -1.0]) @ T.scale([2.0, 2.0, 2.0])}


def weight_lookup(data, to_local, p, dt):
    """clamp(eval_1(p), 0, 1) of a one-channel grid `data` (z, y, x) with the
    3x4 world -> [0, 1]^3 transform `to_local` at the points p (3, n), in the
    arithmetic of `dt`: Texture3f's linear filter with clamped taps
    (grid.cpp:545-558)."""
    data = np.asarray(data, np.float32).astype(dt)
    M = np.asarray(to_local, np.float32).astype(dt).reshape(3, 4)
    p = np.asarray(p, np.float32).astype(dt)
    q = [(M[r, 0] * p[0] + M[r, 1] * p[1]) + (M[r, 2] * p[2] + M[r, 3]) for r in range(3)]
    rz, ry, rx = data.shape
    idx, w1 = [], []
    for qa, r in zip(q, (rx, ry, rz)):
        pa = np.clip(qa * dt(r) - dt(0.5), dt(-1), dt(r))   # beyond [-1, r] both taps are the edge texel
        ia = np.floor(pa)
        w1.append((pa - ia).astype(dt))
        ia = ia.astype(np.int64)
        idx.append((np.clip(ia, 0, r - 1), np.clip(ia + 1, 0, r - 1)))
    w0 = [dt(1) - w for w in w1]
    tap = lambda bx, by, bz: data[idx[2][bz], idx[1][by], idx[0][bx]]
    f = lambda by, bz: w0[0] * tap(0, by, bz) + w1[0] * tap(1, by, bz)
    f0 = w0[1] * f(0, 0) + w1[1] * f(1, 0)
    f1 = w0[1] * f(0, 1) + w1[1] * f(1, 1)
    return np.clip(w0[2] * f0 + w1[2] * f1, dt(0), dt(1)).astype(dt)
