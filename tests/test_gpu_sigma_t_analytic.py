"""GPU: prbvolpath's sigma_t gradients ('<medium>.sigma_t.value', '.data')
against float64 single-scatter quadratures (analytic_cases.py) -- the first
check of these gradients that does not go through the CPU oracle.

Same cases, film, spp and seeds as test_sigma_t_analytic_oracle.py, one
backward call per seed (a texel's float atomics then sum fewer than 1e6
addends).  Over the seeds,

    |mean - quadrature| <= 4 SE,   SE = std(ddof=1) / sqrt(n) <= 1 % of |quadrature|.

4 SE is one more than the CPU test allows: the device's samples are those of
the oracle for >= 99.9 % of the samples, and the CPU test shows the oracle with
these very seeds within 3 SE.  The cap on SE is a condition on the case, as
there.

Every prbvolpath backward engine is held to it (the default plan, the
per-sample pass, the replay without the NEE log, and the deterministic
fixed-point sums), then forward mode, the primal render, and a backward pass
after params.update() of the homogeneous value and of the grid -- the recomputed
majorant and the uploaded grid against an absolute answer.
"""
import numpy as np
import pytest

import analytic_cases as AC
from test_gpu_phase_g_grad import _engine

pytestmark = pytest.mark.gpu

ENGINES = ["sched", "sample", "replay", "deterministic"]


def _mi():
    import mitsuba_hip as mi
    if not mi.is_available():
        pytest.fail("no HIP device / native library: the GPU tests need an MI355X")
    mi.set_variant("hip_ad_rgb")
    return mi


def _grad_in():
    import torch
    return torch.full((AC.H, AC.W, 3), 1.0 / (AC.H * AC.W * 3), dtype=torch.float32, device="cuda")


def _check(rows):
    """rows: (case, label, coarse, fine, samples); prints the table, then asserts"""
    table = [(c, l, lo, hi) + AC.z_row(c, l, hi, s) for c, l, lo, hi, s in rows]
    for t in table:
        print(t[-1])
    for case, label, lo, hi, mean, se, z, row in table:
        assert abs(lo - hi) <= AC.QUAD_RTOL * abs(hi), f"quadrature not converged: {case} {label} {lo} {hi}"
        assert se <= AC.SE_CAP * abs(hi), row
        assert abs(z) <= 4.0, row


def _backward_samples(mi, scene, params, quantities, **kw):
    """{label: [value per seed]}: one render_backward per seed, all keys of the case at once"""
    keys = list(dict.fromkeys(q[1] for q in quantities))
    gi = _grad_in()
    out = {q[0]: [] for q in quantities}
    for seed in AC.BACKWARD_SEEDS:
        grads = mi.render_backward(scene, params, gi, keys, scene.integrator(), seed=seed, spp=AC.SPP, **kw)
        grads = {k: g.double().cpu().numpy() for k, g in zip(keys, grads)}
        for label, key, mask, _, _ in quantities:
            g = grads[key]
            assert np.isfinite(g).all(), (key, seed)
            out[label].append(float(g.sum()) if mask is None else float((g.reshape(mask.shape) * mask).sum()))
    return out


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("name", AC.ALL_CASES)
def test_backward_meets_the_quadrature(name, engine, monkeypatch):
    _engine(monkeypatch, engine)
    mi = _mi()
    scene = mi.load_dict(AC.scene_dict(name))
    quantities = AC.quantities(name)
    samples = _backward_samples(mi, scene, mi.traverse(scene), quantities, deterministic=engine == "deterministic")
    _check([(f"{name}/{engine}", label, lo, hi, samples[label]) for label, _, _, lo, hi in quantities])


FORWARD = [("hom_thin", "sigma_t"), ("het_random_6x8x7", "ones"), ("het_random_6x8x7", "sun_only")]


@pytest.mark.parametrize("name,label", FORWARD)
def test_forward_mode_meets_the_quadrature(name, label):
    """the tangent set to the mask (to 1 for the value): the forward image's mean is the same derivative"""
    mi = _mi()
    import torch
    scene = mi.load_dict(AC.scene_dict(name))
    params = mi.traverse(scene)
    (_, key, mask, lo, hi), = [q for q in AC.quantities(name) if q[0] == label]
    tan = torch.ones(1) if mask is None else torch.from_numpy(mask.reshape(tuple(params[key].shape)).copy())
    tan = tan.cuda()
    means = []
    for seed in AC.BACKWARD_SEEDS:
        img = mi.render_forward(scene, params, {key: tan}, scene.integrator(), seed=seed, spp=AC.SPP)
        means.append(float(img.double().mean().cpu()))
    assert np.isfinite(means).all()
    _check([(f"{name}/forward", label, lo, hi, means)])


@pytest.mark.parametrize("name", AC.ALL_CASES)
def test_primal_meets_the_quadrature(name):
    """prbvolpath's own primal render (no volpath involved) against L"""
    mi = _mi()
    scene = mi.load_dict(AC.scene_dict(name))
    lo, hi = AC.case_references(name)
    means = [float(mi.develop(scene, mi.render_film(scene, scene.integrator(), seed=s, spp=AC.SPP)).double().mean().cpu())
             for s in AC.PRIMAL_SEEDS]
    assert np.isfinite(means).all()
    _check([(f"{name}/primal", "primal", lo.L, hi.L, means)])


def test_backward_after_update_of_the_value():
    """hom_thin's scene, rendered once, then sigma_t 0.3 -> 2.0: hom_thick's quadrature"""
    mi = _mi()
    before, after = AC.UPDATED_VALUE
    scene = mi.load_dict(AC.scene_dict(before))
    params = mi.traverse(scene)
    mi.render_film(scene, scene.integrator(), seed=1, spp=4)            # the device scene exists before the update
    params["medium1.sigma_t.value"] = AC.HOM_CASES[after]["sigma_t"]
    params.update()
    quantities = AC.quantities(after)
    samples = _backward_samples(mi, scene, params, quantities)
    _check([(f"{before}->{after}", label, lo, hi, samples[label]) for label, _, _, lo, hi in quantities])


def test_backward_after_update_of_the_grid():
    """het_random_6x8x7's scene, rendered once, then another random grid with another majorant"""
    mi = _mi()
    scene = mi.load_dict(AC.scene_dict(AC.UPDATED_GRID))
    params = mi.traverse(scene)
    mi.render_film(scene, scene.integrator(), seed=1, spp=4)
    key = "medium1.sigma_t.data"
    params[key] = AC.updated_grid().reshape(tuple(params[key].shape))
    params.update()
    quantities = AC.updated_grid_quantities()
    samples = _backward_samples(mi, scene, params, quantities)
    _check([(f"{AC.UPDATED_GRID}->new", label, lo, hi, samples[label]) for label, _, _, lo, hi in quantities])
