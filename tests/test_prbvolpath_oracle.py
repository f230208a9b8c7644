"""CPU: the prbvolpath restatement (oracle, SURVEY.md §8(f) rank 1,
src/python/python/ad/integrators/prbvolpath.py).

The reference ships no prbvolpath gradient fixtures, so the restatement is
"parity unpinned" against llvm_ad_rgb and is checked by properties of the
estimator instead:
  * with Russian roulette off, the albedo and surface-reflectance gradients
    are exact derivatives of the same-seed primal (the sampling decisions do
    not depend on them): central finite differences agree to ~1e-4;
  * the sigma_t gradients (grid texels, homogeneous value) are unbiased:
    common-random-number finite differences over many samples agree within
    the Monte Carlo error;
  * the primal matches a quadrature of single scattering under the sun.
Single scattering's sigma_t gradients are held to closed forms, far tighter, in
test_sigma_t_analytic_oracle.py; the two 12 % tests here cover multiple
scattering, which has none.
"""
import numpy as np
import pytest

import oracle_py as O


def _mi():
    import mitsuba_hip as mi
    mi.set_variant("hip_ad_rgb")
    return mi


def _scene(mi, W, spp, albedo=0.8, grid=None, floor=None, medium_type="heterogeneous", sigma_t=1.0,
           sky=0.2, sun=5.0, integrator="prbvolpath", max_depth=6, rr_depth=100):
    T = mi.Transform4f
    g = grid if grid is not None else mi.fbm_grid(8)
    d = mi.volume_cube(W, W, spp, grid=g, scale=4.0, albedo=albedo, g=0.5, max_depth=max_depth,
                       rr_depth=rr_depth, medium_type=medium_type, sigma_t=sigma_t, sky=sky, sun=sun)
    if sky is None:
        del d["sky"]
    d["integrator"] = {"type": integrator, "max_depth": max_depth, "rr_depth": rr_depth}
    if floor is not None:
        d["floor"] = {"type": "rectangle",
                      "to_world": T.translate([0, -1.2, 0]) @ T.rotate([1, 0, 0], -90) @ T.scale([3, 3, 3]),
                      "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": list(floor)}}}
    return mi.load_dict(d)


def _loss(sc, seed, spp, gi):
    img = O.develop(O.render(sc, sc.integrator(), seed=seed, spp=spp))
    return float((img.astype(np.float64) * gi).sum())


def test_albedo_gradient_is_the_same_seed_derivative():
    mi = _mi()
    W, spp, seed, h = 24, 8, 3, 1e-2
    gi = np.random.default_rng(0).standard_normal((W, W, 3)).astype(np.float32)
    sc = _scene(mi, W, spp)
    p = mi.traverse(sc)
    g = O.render_backward(sc, sc.integrator(), seed, spp, gi, [p.param_id("medium1.albedo.value")], [(3,)])[0]
    fd = []
    for c in range(3):
        a, b = np.full(3, 0.8), np.full(3, 0.8)
        a[c] += h
        b[c] -= h
        fd.append((_loss(_scene(mi, W, spp, albedo=a.tolist()), seed, spp, gi) -
                   _loss(_scene(mi, W, spp, albedo=b.tolist()), seed, spp, gi)) / (2 * h))
    assert np.allclose(g, fd, rtol=1e-3, atol=1e-3), (g, fd)


def test_surface_reflectance_gradient_is_the_same_seed_derivative():
    mi = _mi()
    W, spp, seed, h = 20, 8, 9, 1e-2
    rho = np.array([0.6, 0.5, 0.4])
    gi = np.random.default_rng(1).standard_normal((W, W, 3)).astype(np.float32)
    sc = _scene(mi, W, spp, floor=rho)
    p = mi.traverse(sc)
    keys = ["floor.bsdf.reflectance.value", "medium1.albedo.value"]
    g = O.render_backward(sc, sc.integrator(), seed, spp, gi, [p.param_id(k) for k in keys], [(3,), (3,)])
    fd = []
    for c in range(3):
        a, b = rho.copy(), rho.copy()
        a[c] += h
        b[c] -= h
        fd.append((_loss(_scene(mi, W, spp, floor=a), seed, spp, gi) -
                   _loss(_scene(mi, W, spp, floor=b), seed, spp, gi)) / (2 * h))
    assert np.abs(g[0]).max() > 1e-2
    assert np.allclose(g[0], fd, rtol=1e-3, atol=1e-3), (g[0], fd)


def test_grid_gradient_unbiased_against_finite_differences():
    mi = _mi()
    W, spp, h = 16, 8192, 0.05
    g0 = mi.fbm_grid(8).astype(np.float32)
    g0[0, 0, 0] = g0.max() + 0.2            # the majorant stays outside the perturbed block
    mask = np.zeros_like(g0)
    mask[2:6, 2:6, 2:6] = 1.0
    gi = np.ones((W, W, 3), np.float32)     # d mean-radiance / d density of the core
    sc = _scene(mi, W, spp, grid=g0)
    p = mi.traverse(sc)
    key = "medium1.sigma_t.data"
    assert tuple(p[key].shape) == (8, 8, 8, 1)
    adj = np.mean([float((O.render_backward(sc, sc.integrator(), s, spp, gi, [p.param_id(key)],
                                            [g0.shape])[0] * mask).sum()) for s in (5, 6)])
    fd = np.mean([(_loss(_scene(mi, W, spp, grid=g0 + h * mask), s, spp, gi) -
                   _loss(_scene(mi, W, spp, grid=g0 - h * mask), s, spp, gi)) / (2 * h) for s in (5, 6, 7, 8)])
    assert abs(adj - fd) <= 0.12 * abs(fd), (adj, fd)


def test_homogeneous_sigma_t_gradient_unbiased_against_finite_differences():
    mi = _mi()
    W, spp, h, st = 16, 4096, 0.02, 0.5
    gi = np.ones((W, W, 3), np.float32)
    sc = _scene(mi, W, spp, medium_type="homogeneous", sigma_t=st)
    p = mi.traverse(sc)
    key = "medium1.sigma_t.value"
    assert key in p and tuple(p[key].shape) == (1,)
    adj = np.mean([O.render_backward(sc, sc.integrator(), s, spp, gi, [p.param_id(key)], [(1,)])[0][0]
                   for s in (1, 2)])
    fd = np.mean([(_loss(_scene(mi, W, spp, medium_type="homogeneous", sigma_t=st + h), s, spp, gi) -
                   _loss(_scene(mi, W, spp, medium_type="homogeneous", sigma_t=st - h), s, spp, gi)) / (2 * h)
                  for s in (1, 2, 3, 4)])
    assert abs(adj - fd) <= 0.12 * abs(fd), (adj, fd)


def test_primal_single_scattering_matches_quadrature():
    """Homogeneous cube under the sun, max_depth 2 (single scattering only),
    near-zero field of view: every camera ray is the cube's axis, and the
    radiance is  E * integral_0^2 a s exp(-s u) f_HG exp(-s l(u)) du  with l
    the sun-ward distance to the cube boundary (the fork's prbvolpath
    attenuates the sun, prbvolpath.py:357-359, unlike volpath's spawn_ray_to)."""
    mi = _mi()
    W, spp, s, a, g, E = 4, 4096, 0.8, 0.7, 0.5, 5.0
    d = mi.volume_cube(W, W, spp, medium_type="homogeneous", sigma_t=s, scale=1.0, albedo=a, g=g,
                       sky=0.0, sun=E, max_depth=2, rr_depth=100, fov=0.01)
    del d["sky"]
    d["integrator"] = {"type": "prbvolpath", "max_depth": 2, "rr_depth": 100}
    img = O.develop(O.render(mi.load_dict(d), seed=4, spp=spp))
    # quadrature (float64)
    sun = np.array([0.0, -1.0, -0.3]) / np.linalg.norm([0.0, -1.0, -0.3])
    w = -sun                                   # towards the sun
    cos = -np.dot(w, [0.0, 0.0, -1.0])         # eval_hg(g, dot(wo, wi)), wi = -ray.d
    f = (1 - g * g) / (4 * np.pi * (1 + g * g + 2 * g * cos) ** 1.5)
    u = np.linspace(0.0, 2.0, 200001)
    l = np.minimum(1.0 / w[1], u / w[2])       # exits through y = 1 or z = 1
    L = np.trapezoid(a * s * np.exp(-s * u) * f * E * np.exp(-s * l), u)
    assert abs(img.mean() - L) <= 0.02 * L, (img.mean(), L)


def test_gradient_is_linear_in_grad_in():
    mi = _mi()
    W, spp = 12, 4
    sc = _scene(mi, W, spp, floor=(0.5, 0.5, 0.5))
    p = mi.traverse(sc)
    keys = ["medium1.sigma_t.data", "medium1.albedo.value", "floor.bsdf.reflectance.value"]
    shapes = [tuple(p[k].shape) for k in keys]
    ids = [p.param_id(k) for k in keys]
    r = np.random.default_rng(3)
    g1, g2 = (r.standard_normal((W, W, 3)).astype(np.float32) for _ in range(2))
    a = O.render_backward(sc, sc.integrator(), 2, spp, g1, ids, shapes)
    b = O.render_backward(sc, sc.integrator(), 2, spp, g2, ids, shapes)
    c = O.render_backward(sc, sc.integrator(), 2, spp, g1 + 2 * g2, ids, shapes)
    for x, y, z in zip(a, b, c):
        assert np.allclose(z, x + 2 * y, rtol=1e-4, atol=1e-5 * max(1.0, np.abs(z).max()))


def test_medium_parameters_need_prbvolpath():
    mi = _mi()
    sc = _scene(mi, 8, 4)
    p = mi.traverse(sc)
    prb = mi.Integrator("prb", {})
    with pytest.raises(RuntimeError, match="prbvolpath"):
        O.render_backward(sc, prb, 0, 4, np.ones((8, 8, 3), np.float32),
                          [p.param_id("medium1.albedo.value")], [(3,)])
