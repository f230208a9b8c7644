"""CPU: the oracle's prbvolpath sigma_t gradients against float64 single-scatter
quadratures (analytic_cases.py), by z-tests.

PRB's detached estimator is unbiased for the derivative of the render, so over
independent seeds  |mean - quadrature| <= 3 SE  with  SE = std(ddof=1) / sqrt(n)
-- provided SE itself is small enough for the test to bite: it must stay within
1 % of |quadrature| (a condition on the case; a mask that misses it is replaced
or given more samples, never a wider cap).  The primal render is held to L in
the same way, with seeds disjoint from the backward pass'.

The cases, sizes and seeds are those of the device's test
(test_gpu_sigma_t_analytic.py): 8 x 8 at 16384 spp, 16 seeds, grad_in =
1 / (W H C), so a gradient is the derivative of the image mean.

Multiple scattering has no closed form and stays with the two common-random-
number tests of test_prbvolpath_oracle.py.
"""
import numpy as np
import pytest

import analytic_cases as AC
import oracle_py as O


def _mi():
    import mitsuba_hip as mi
    mi.set_variant("hip_ad_rgb")
    return mi


GI = np.full((AC.H, AC.W, 3), 1.0 / (AC.H * AC.W * 3), np.float32)


def _backward_samples(mi, name, quantities=None, update=None):
    """{label: [value per seed]} of the case's quantities; update: {key: value} for params.update() before"""
    scene = mi.load_dict(AC.scene_dict(name))
    params = mi.traverse(scene)
    if update:
        params.update(update)
    quantities = quantities or AC.quantities(name)
    keys = list(dict.fromkeys(q[1] for q in quantities))
    ids = [params.param_id(k) for k in keys]
    shapes = [tuple(params[k].shape) for k in keys]
    out = {q[0]: [] for q in quantities}
    for seed in AC.BACKWARD_SEEDS:
        grads = dict(zip(keys, O.render_backward(scene, scene.integrator(), seed, AC.SPP, GI, ids, shapes)))
        for label, key, mask, _, _ in quantities:
            g = grads[key].astype(np.float64)
            assert np.isfinite(g).all(), (name, key, seed)
            out[label].append(float(g.sum()) if mask is None else float((g.reshape(mask.shape) * mask).sum()))
    return out


def _check(rows):
    """rows: (case, label, coarse, fine, samples); prints the table, then asserts"""
    table = [(c, l, lo, hi) + AC.z_row(c, l, hi, s) for c, l, lo, hi, s in rows]
    for t in table:
        print(t[-1])
    for case, label, lo, hi, mean, se, z, row in table:
        assert abs(lo - hi) <= AC.QUAD_RTOL * abs(hi), f"quadrature not converged: {case} {label} {lo} {hi}"
        assert se <= AC.SE_CAP * abs(hi), row
        assert abs(z) <= 3.0, row


@pytest.mark.parametrize("name", AC.ALL_CASES)
def test_backward_meets_the_quadrature(name):
    mi = _mi()
    samples = _backward_samples(mi, name)
    _check([(name, label, lo, hi, samples[label]) for label, _, _, lo, hi in AC.quantities(name)])


@pytest.mark.parametrize("name", AC.ALL_CASES)
def test_primal_meets_the_quadrature(name):
    mi = _mi()
    scene = mi.load_dict(AC.scene_dict(name))
    lo, hi = AC.case_references(name)
    means = [float(O.develop(O.render(scene, scene.integrator(), seed=s, spp=AC.SPP)).astype(np.float64).mean())
             for s in AC.PRIMAL_SEEDS]
    assert np.isfinite(means).all()
    _check([(name, "primal", lo.L, hi.L, means)])


@pytest.mark.slow
def test_backward_after_update():
    """the cases of the device's update tests, on the host scene: that the oracle with these seeds is within 3 SE
    of the updated parameters' quadrature is what lets the device's test allow 4"""
    mi = _mi()
    before, after = AC.UPDATED_VALUE
    q = AC.quantities(after)
    s = _backward_samples(mi, before, q, {"medium1.sigma_t.value": AC.HOM_CASES[after]["sigma_t"]})
    rows = [(f"{before}->{after}", label, lo, hi, s[label]) for label, _, _, lo, hi in q]
    q = AC.updated_grid_quantities()
    g = AC.updated_grid()
    s = _backward_samples(mi, AC.UPDATED_GRID, q, {"medium1.sigma_t.data": g.reshape(g.shape + (1,))})
    _check(rows + [(f"{AC.UPDATED_GRID}->new", label, lo, hi, s[label]) for label, _, _, lo, hi in q])


# ---------------------------------------------------------------------------
# the helper itself
# ---------------------------------------------------------------------------
def test_trilinear_rule():
    rng = np.random.default_rng(2)
    g = rng.random((3, 5, 4))
    rz, ry, rx = g.shape
    # texel centres return the texel
    z, y, x = np.meshgrid(np.arange(rz), np.arange(ry), np.arange(rx), indexing="ij")
    q = np.stack([(x + 0.5) / rx, (y + 0.5) / ry, (z + 0.5) / rz], -1).reshape(-1, 3)
    np.testing.assert_allclose(AC.tri(g, q), g.reshape(-1), rtol=0, atol=1e-15)
    # a field linear in the texel index is reproduced between the outer centres and clamped outside them
    lin = 1.0 + 2.0 * x + 3.0 * y - 0.5 * z
    q = rng.random((4096, 3))
    p = np.clip(q * [rx, ry, rz] - 0.5, 0.0, [rx - 1, ry - 1, rz - 1])
    np.testing.assert_allclose(AC.tri(lin, q), 1.0 + 2.0 * p[:, 0] + 3.0 * p[:, 1] - 0.5 * p[:, 2], rtol=0, atol=1e-12)
    # the weights of a lookup sum to one, border included
    _, w = AC.taps(g.shape, np.concatenate([q, [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]]]))
    np.testing.assert_allclose(w.sum(-1), 1.0, rtol=0, atol=1e-15)


def test_generic_quadrature_reproduces_the_homogeneous_form():
    """a 1 x 1 x 1 grid of value sigma_t is the homogeneous medium: the per-texel field's one entry is
    d L / d sigma_t, by the two-dimensional quadrature instead of the one-dimensional form"""
    for name in ("hom_thin", "hom_scaled"):
        c = AC.HOM_CASES[name]
        want = AC.case_references(name)[1]
        d = AC._cube(grid=np.full((1, 1, 1), c["sigma_t"], np.float32), scale=c["scale"], g=c["g"])
        got = AC.Reference(AC.Geometry(d), AC.RES_COARSE)
        assert abs(got.L - want.L) <= 1e-5 * want.L
        assert abs(got.d_mask() - want.d_mask()) <= 1e-5 * abs(want.d_mask())


def test_field_is_the_derivative_of_L():
    """central differences of the quadrature's own L along a mask reproduce <field, mask>: the field's algebra
    (swapped sums, scatter weights) against the plain formula"""
    g0 = AC.random_grid()
    m = AC.masks(g0.shape)["random0"].astype(np.float64)
    res, h = (501, 201), 1e-4
    for name in ("het_random_6x8x7", "wall_het"):
        ref = AC.Reference(AC.Geometry(AC.scene_dict(name)), res)
        Lp, Lm = (AC.Reference(AC.Geometry(AC.scene_dict(name, grid=g0.astype(np.float64) + s * h * m)), res).L
                  for s in (+1, -1))
        fd = (Lp - Lm) / (2 * h)
        assert abs(ref.d_mask(m) - fd) <= 1e-6 * abs(fd), (name, ref.d_mask(m), fd)


def test_sun_only_mask_has_no_weight_on_the_axis():
    for name in AC.HET_CASES:
        geo = AC.case_references(name)[1].geo
        m = AC.sun_only_mask(geo.grid.shape)
        u = np.linspace(0.0, geo.length, 257)
        assert m.sum() > 0 and np.all(AC.tri(m, geo.local(geo.cam(u))) == 0.0)
        # ... with a texel of margin on either side of the near-zero field of view
        off = geo.cam(u) + np.array([0.0, 2.0 / geo.grid.shape[1], 0.0])
        assert np.all(AC.tri(m, geo.local(off)) == 0.0)
