"""CPU: the volpath / prbvolpath restatements (oracle) on the medium
topologies of vol_cases.py -- several media, mixed medium types, a camera
inside a medium, grids that are not their boundary's box.

test_gpu_vol_topologies.py holds the device to the oracle on these layouts, so
the oracle is pinned here first, by properties that do not depend on its own
conventions: known transmittances, invariance of the expectation under a rigid
motion of the whole scene, the white furnace, and gradients against finite
differences of the oracle's own primal.
"""
import math

import numpy as np
import pytest

import oracle_py as O
import vol_cases as VC


def _mi():
    import mitsuba_hip as mi
    mi.set_variant("hip_ad_rgb")
    return mi


# ---------------------------------------------------------------------------
# absorbers in series
# ---------------------------------------------------------------------------
def _absorbers(mi, inside):
    """A homogeneous cube (sigma_t 0.5) around the origin in front of a
    heterogeneous one at z = -3 (the constant 0.25 on a 3 x 4 x 5 grid, scale
    2): albedo 0, unit sky, a near-zero field of view."""
    T = mi.Transform4f
    d = mi.volume_cube(9, 9, 4096, medium_type="homogeneous", sigma_t=0.5, scale=1.0, albedo=0.0, g=0.0,
                       sky=1.0, sun=None, max_depth=-1, fov=1.0)
    back = T.translate([0.0, 0.0, -3.0])
    d["medium2"] = {"type": "heterogeneous",
                    "sigma_t": {"type": "gridvolume", "data": np.full((5, 4, 3), 0.25, np.float32),
                                "to_world": back @ VC.unit_grid_to_world(mi)},
                    "scale": 2.0, "albedo": 0.0, "phase": {"type": "isotropic"}}
    d["cube2"] = {"type": "cube", "to_world": back, "bsdf": {"type": "null"},
                  "interior": {"type": "ref", "id": "medium2"}}
    if inside:
        d["sensor"]["to_world"] = T.look_at(origin=[0, 0, 0.5], target=[0, 0, -1], up=[0, 1, 0])
        d["sensor"]["medium"] = {"type": "ref", "id": "medium1"}
    return mi.load_dict(d)


@pytest.mark.parametrize("inside", [False, True])
def test_absorbers_in_series(inside):
    """The centre pixel sees exp(-(0.5 * 2 + 0.5 * 2)) = 0.13534 through both
    cubes, and exp(-(0.5 * 1.5 + 0.5 * 2)) = 0.17377 from z = 0.5 inside the
    first one (sensor.medium): a homogeneous and a heterogeneous medium on one
    ray.  Measured 0.13588 and 0.17407; the bound is
    test_homogeneous_absorber_transmittance's."""
    mi = _mi()
    s = _absorbers(mi, inside)
    assert s.desc.n_media == 2 and s.medium(0).type != s.medium(1).type
    img = O.develop(O.render(s, seed=0, spp=4096))
    ref = math.exp(-(0.5 * (1.5 if inside else 2.0) + 0.5 * 2.0))
    print(f"absorbers in series (camera inside: {inside}): {img[4, 4, 0]:.5f} against {ref:.5f}")
    assert abs(img[4, 4, 0] - ref) < 0.02


def test_nested_absorbers():
    """A heterogeneous cube of half-size 0.4 (the constant 0.5 at scale 2:
    sigma_t 1) inside the homogeneous one (sigma_t 0.5), interior = medium2 and
    exterior = medium1 on its boundary: the centre pixel sees
    exp(-(0.5 * 1.2 + 1 * 0.8)) = 0.24660 -- not exp(-1) = 0.368 (the boundary
    ignored) nor exp(-0.6) = 0.549 (the path leaving into vacuum at the inner
    cube).  Measured 0.23725 (one pixel at 4096 spp: a standard deviation of
    about 0.007); the bound is test_homogeneous_absorber_transmittance's."""
    mi = _mi()
    T = mi.Transform4f
    d = mi.volume_cube(9, 9, 4096, medium_type="homogeneous", sigma_t=0.5, scale=1.0, albedo=0.0, g=0.0,
                       sky=1.0, sun=None, max_depth=-1, fov=1.0)
    inner = T.scale([0.4, 0.4, 0.4])
    d["medium2"] = {"type": "heterogeneous",
                    "sigma_t": {"type": "gridvolume", "data": np.full((5, 4, 3), 0.5, np.float32),
                                "to_world": inner @ VC.unit_grid_to_world(mi)},
                    "scale": 2.0, "albedo": 0.0, "phase": {"type": "isotropic"}}
    d["core"] = {"type": "cube", "to_world": inner, "bsdf": {"type": "null"},
                 "interior": {"type": "ref", "id": "medium2"}, "exterior": {"type": "ref", "id": "medium1"}}
    img = O.develop(O.render(mi.load_dict(d), seed=0, spp=4096))
    ref = math.exp(-(0.5 * 1.2 + 1.0 * 0.8))
    print(f"nested absorbers: {img[4, 4, 0]:.5f} against {ref:.5f}")
    assert abs(img[4, 4, 0] - ref) < 0.02


# ---------------------------------------------------------------------------
# rigid-motion invariance of the expectation
# ---------------------------------------------------------------------------
def _moved(mi, integrator, M, sun):
    """The parity tests' scene (cube, grid, floor, sensor, sun) moved by M."""
    d = VC.base(mi, integrator, 16, 16, 1024, sun=5.0 if sun else None)
    d["sensor"]["to_world"] = M @ d["sensor"]["to_world"]
    d["cube"]["to_world"] = M
    d["medium1"]["sigma_t"]["to_world"] = M @ d["medium1"]["sigma_t"]["to_world"]
    d["floor"]["to_world"] = M @ d["floor"]["to_world"]
    if sun:
        d["sun"]["direction"] = M.transform_vector(d["sun"]["direction"]).tolist()
    return mi.load_dict(d)


@pytest.mark.parametrize("integrator", ["volpath", "prbvolpath"])
def test_rigid_motion_leaves_the_expectation(integrator):
    """Sensor, cube, grid, floor and sun moved together by
    M = translate(.3, -.2, .5) @ rotate((1, 2, 3), 37 deg): the image mean stays
    within Monte Carlo error.  Only means are compared: per-sample results are
    not invariant (coordinate_system is not equivariant, so the sampled
    directions differ).

    volpath runs without the sun.  It reproduces the reference's unattenuated
    sun (test_sun_contributes_unattenuated_like_the_reference): the shadow ray
    towards p - d * inf ends the transmittance loop through NaN components,
    and which components are NaN depends on which components of the direction
    are zero -- so with the sun the mean changes by about 26 % under M.  That
    is the reproduced quirk, not a defect of the restatement.  prbvolpath
    attenuates the sun and keeps it.

    8 fixed seeds per placement at 16 x 16 @ 1024 spp; s is the identity
    placement's seed-to-seed standard deviation, the means over the seeds may
    differ by 4 s sqrt(2 / 8).  Measured:
      volpath     identity 0.152748, moved 0.152749: difference 7.2e-7, standard error 3.4e-5
      prbvolpath  identity 0.205255, moved 0.205067: difference 1.9e-4, standard error 6.6e-4
      volpath with the sun (4 seeds, not asserted): 0.5001 against 0.3713"""
    mi = _mi()
    T = mi.Transform4f
    M = T.translate([0.3, -0.2, 0.5]) @ T.rotate([1, 2, 3], 37)
    sun = integrator == "prbvolpath"
    seeds = range(8)
    means = []
    for m in (T(), M):
        s = _moved(mi, integrator, m, sun)
        means.append([float(O.develop(O.render(s, seed=k, spp=1024)).astype(np.float64).mean()) for k in seeds])
    se = np.std(means[0], ddof=1) * math.sqrt(2.0 / len(seeds))
    diff = abs(np.mean(means[0]) - np.mean(means[1]))
    print(f"{integrator}: identity {np.mean(means[0]):.6f}, moved {np.mean(means[1]):.6f}: "
          f"difference {diff:.2e}, standard error {se:.2e}")
    assert np.mean(means[0]) > 0.05
    assert diff <= 4 * se


# ---------------------------------------------------------------------------
# white furnace
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("inside", [False, True])
def test_white_furnace_three_media(inside):
    """three_media without the floor, every albedo 1, under a unit sky: every
    pixel's expectation is 1, also from inside medium1 (looking along +x
    through cube 1 towards cube 2).  test_white_furnace's bound and budget."""
    mi = _mi()
    d = VC.three_media(mi, "volpath", 16, 16, 64, with_floor=False, albedo=1.0, sky=1.0, sun=None, max_depth=-1)
    d["medium2"]["albedo"] = d["medium3"]["albedo"] = 1.0
    if inside:
        d["sensor"]["to_world"] = mi.Transform4f.look_at(origin=[-0.9, 0.0, 0.0], target=[0.9, 0.1, 0.0], up=[0, 1, 0])
        d["sensor"]["medium"] = {"type": "ref", "id": "medium1"}
    s = mi.load_dict(d)
    assert s.desc.n_media == 3 and s.desc.n_shapes == 3
    img = O.develop(O.render(s, seed=0, spp=256))
    print(f"white furnace, three media (camera inside: {inside}): mean {img.mean():.5f}, std {img.std():.4f}")
    assert abs(img.mean() - 1.0) < 0.01


def test_white_furnace_nested_media():
    """nested_media (a homogeneous medium inside the heterogeneous one) without
    the floor, both albedos 1, under a unit sky."""
    mi = _mi()
    d = VC.nested_media(mi, "volpath", 16, 16, 64, with_floor=False, albedo=1.0, sky=1.0, sun=None, max_depth=-1)
    d["medium2"]["albedo"] = 1.0
    img = O.develop(O.render(mi.load_dict(d), seed=0, spp=256))
    print(f"white furnace, nested media: mean {img.mean():.5f}, std {img.std():.4f}")
    assert abs(img.mean() - 1.0) < 0.01


# ---------------------------------------------------------------------------
# gradients
# ---------------------------------------------------------------------------
def _loss(sc, seed, spp, gi):
    img = O.develop(O.render(sc, sc.integrator(), seed=seed, spp=spp))
    return float((img.astype(np.float64) * gi).sum())


def _same_seed_fd(mi, make, key, value, W, H, spp, seed, gi_seed):
    """test_albedo_gradient_is_the_same_seed_derivative's method: with Russian
    roulette off no sampling decision depends on an albedo or a reflectance,
    so the adjoint is the derivative of the same-seed primal."""
    h = 1e-2
    gi = np.random.default_rng(gi_seed).standard_normal((H, W, 3)).astype(np.float32)
    sc = make(value)
    p = mi.traverse(sc)
    g = O.render_backward(sc, sc.integrator(), seed, spp, gi, [p.param_id(key)], [(3,)])[0]
    fd = []
    for c in range(3):
        a, b = np.array(value, np.float64), np.array(value, np.float64)
        a[c] += h
        b[c] -= h
        fd.append((_loss(make(a.tolist()), seed, spp, gi) - _loss(make(b.tolist()), seed, spp, gi)) / (2 * h))
    return g, np.asarray(fd)


def test_second_medium_albedo_gradient_is_the_same_seed_derivative():
    """medium2.albedo.value on three_media (albedo_slot indexed by medium).
    Measured: adjoint (-7.15355, 0.04838, 1.59387), central differences
    (-7.15390, 0.04845, 1.59399)."""
    mi = _mi()

    def make(alb):
        d = VC.three_media(mi, "prbvolpath", 24, 20, 8, rr_depth=100)
        d["medium2"]["albedo"] = alb
        return mi.load_dict(d)
    g, fd = _same_seed_fd(mi, make, "medium2.albedo.value", [0.9, 0.6, 0.3], 24, 20, 8, 3, 0)
    print(f"medium2.albedo.value: adjoint {g}, central differences {fd}")
    assert np.abs(g).max() > 1e-2
    assert np.allclose(g, fd, rtol=1e-3, atol=1e-3), (g, fd)


def test_inner_object_reflectance_gradient_is_the_same_seed_derivative():
    """The reflectance of the diffuse cube inside the medium (object_inside).
    Measured: adjoint (-0.94894, -1.16922, -1.74306), central differences
    (-0.94892, -1.16922, -1.74305)."""
    mi = _mi()

    def make(rho):
        d = VC.object_inside(mi, "prbvolpath", 24, 20, 8, rr_depth=100)
        d["inner"]["bsdf"]["reflectance"]["value"] = rho
        return mi.load_dict(d)
    g, fd = _same_seed_fd(mi, make, VC.INNER_KEY, [0.7, 0.4, 0.3], 24, 20, 8, 9, 1)
    print(f"{VC.INNER_KEY}: adjoint {g}, central differences {fd}")
    assert np.abs(g).max() > 1e-2
    assert np.allclose(g, fd, rtol=1e-3, atol=1e-3), (g, fd)


def _unbiased(make, key, shape, mask, h, W, H, spp):
    """test_grid_gradient_unbiased_against_finite_differences's method: the
    adjoint over two seeds against common-random-number central differences
    over four."""
    import mitsuba_hip as mi
    gi = np.ones((H, W, 3), np.float32)
    sc = make(0.0)
    p = mi.traverse(sc)
    assert tuple(p[key].shape) == shape
    adj = np.mean([float((O.render_backward(sc, sc.integrator(), s, spp, gi, [p.param_id(key)], [shape])[0]
                          * mask).sum()) for s in (5, 6)])
    fd = np.mean([(_loss(make(+h), s, spp, gi) - _loss(make(-h), s, spp, gi)) / (2 * h) for s in (5, 6, 7, 8)])
    return adj, fd


def test_second_grid_gradient_unbiased_against_finite_differences():
    """medium2.sigma_t.data on three_media: the second grid of the packed
    buffer.  The majorant texel stays outside the perturbed block.
    Measured: adjoint -1.08060, finite differences -1.03091 (ratio 1.048)."""
    mi = _mi()
    g0 = VC.crop_795(mi).astype(np.float32)
    g0[0, 0, 0] = g0.max() + 0.2
    mask = np.zeros_like(g0)
    mask[2:5, 2:7, 1:4] = 1.0

    def make(h):
        d = VC.three_media(mi, "prbvolpath", 16, 16, 8192, rr_depth=100)
        d["medium2"]["sigma_t"]["data"] = g0 + h * mask
        return mi.load_dict(d)
    adj, fd = _unbiased(make, "medium2.sigma_t.data", (7, 9, 5, 1), mask[..., None], 0.05, 16, 16, 8192)
    print(f"medium2.sigma_t.data: adjoint {adj:.5f}, finite differences {fd:.5f} (ratio {adj / fd:.4f})")
    assert abs(adj - fd) <= 0.12 * abs(fd), (adj, fd)


def test_third_medium_sigma_t_gradient_unbiased_against_finite_differences():
    """medium3.sigma_t.value on three_media: the homogeneous medium next to
    two heterogeneous ones.  Measured: adjoint 0.59977, finite differences
    0.63481 (ratio 0.945)."""
    mi = _mi()

    def make(h):
        d = VC.three_media(mi, "prbvolpath", 16, 16, 4096, rr_depth=100)
        d["medium3"]["sigma_t"] = 0.8 + h
        return mi.load_dict(d)
    adj, fd = _unbiased(make, "medium3.sigma_t.value", (1,), np.ones(1), 0.02, 16, 16, 4096)
    print(f"medium3.sigma_t.value: adjoint {adj:.5f}, finite differences {fd:.5f} (ratio {adj / fd:.4f})")
    assert abs(adj - fd) <= 0.12 * abs(fd), (adj, fd)


def test_grid_gradient_unbiased_without_spectral_extinction():
    """has_spectral_extinction = False with a chromatic albedo: its grid
    gradient is an order of magnitude larger than the other cases' (max-abs
    25 against about 2 at 24 x 20 @ 8; the base scene's, whose grid is the
    cube's box as well, is 30), so it is shown unbiased, not assumed.
    Measured: adjoint -10.54383, finite differences -10.76329 (ratio 0.980)."""
    mi = _mi()
    g0 = mi.fbm_grid(16).astype(np.float32)
    g0[0, 0, 0] = g0.max() + 0.2
    mask = np.zeros_like(g0)
    mask[4:12, 4:12, 4:12] = 1.0

    def make(h):
        return mi.load_dict(VC.no_spectral_extinction(mi, "prbvolpath", 16, 16, 8192, rr_depth=100,
                                                      grid=g0 + h * mask))
    adj, fd = _unbiased(make, "medium1.sigma_t.data", (16, 16, 16, 1), mask[..., None], 0.05, 16, 16, 8192)
    print(f"no_spectral_extinction medium1.sigma_t.data: adjoint {adj:.5f}, finite differences {fd:.5f} "
          f"(ratio {adj / fd:.4f})")
    assert abs(adj - fd) <= 0.12 * abs(fd), (adj, fd)
