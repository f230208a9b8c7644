"""GPU: the tabulated (phase/tabphase.cpp over core/distr_1d.h's
IrregularContinuousDistribution) and Rayleigh (phase/rayleigh.cpp, no
depolarization) phase functions.

Function level: mh_phase_sample / mh_phase_eval run the device functions the
volumetric integrators call; they are checked against a numpy restatement of
the distribution (phase_cases.py), evaluated in float64 (the reference) and in
float32 (whose own error against float64 sets the bound: the device may be 4 x
worse, for FMA contraction and division / sqrt rounding, plus 2^-22 where the
float32 restatement happens to be exact).

Integrator level: the execution engines agree bit for bit, a tabulated HG
matches the CPU oracle's analytic HG (and the reversed table its mirror image),
the white furnace stays white, the prbvolpath gradients agree between the
backward's execution paths and with finite differences, and an updated table
renders like a freshly loaded one.  The oracle never sees a tabphase or
rayleigh medium (it would treat it as isotropic)."""
import ctypes as C

import numpy as np
import pytest

import oracle_py as O
from phase_cases import TABLES, Distr, hg

pytestmark = pytest.mark.gpu


def _mi():
    import mitsuba_hip as mi
    if not mi.is_available():
        pytest.fail("no HIP device / native library: the GPU tests need an MI355X")
    return mi


def _tab(key):
    c, v = TABLES[key]
    return {"type": "tabphase", "cost": c, "values": v}


def _phase_scene(mi, phase):
    """A small homogeneous cube whose medium 0 carries `phase` (function-level queries)."""
    d = mi.volume_cube(8, 8, 1, medium_type="homogeneous", sigma_t=1.0, scale=1.0)
    d["medium1"]["phase"] = phase
    return mi.load_dict(d)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def gpu_sample(scene, u1, u2, medium=0):
    from mitsuba_hip import _abi as A
    n = u1.size
    u = np.ascontiguousarray(np.concatenate([u1, u2]).astype(np.float32))
    wo, pdf = np.zeros(3 * n, np.float32), np.zeros(n, np.float32)
    A.check(A.lib().mh_phase_sample(scene.handle(0), medium, n, _p(u), _p(wo), _p(pdf), 0))
    return wo.reshape(3, n), pdf


def gpu_eval(scene, wo, medium=0):
    from mitsuba_hip import _abi as A
    wo = np.ascontiguousarray(wo, np.float32)
    n = wo.shape[1]
    val = np.zeros(n, np.float32)
    A.check(A.lib().mh_phase_eval(scene.handle(0), medium, n, _p(wo), _p(val), 0))
    return val


def _uniforms():
    rng = np.random.default_rng(11)
    u1 = np.concatenate([rng.random(65536, np.float32), np.float32([0.0, 0.5, 1 - 2.0 ** -24])])
    return u1, rng.random(u1.size, np.float32)


ULP1 = 2.0 ** -23


# ---------------------------------------------------------------------------
# function level
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["a", "b", "c", "d", "e", "f"])
def test_tabulated_sampling(key):
    """The float64 CDF at the sampled cosine returns u1; the bound is the
    float32 restatement's own residual on the same inputs, x 4, + 2^-22."""
    mi = _mi()
    c, v = TABLES[key]
    scene = _phase_scene(mi, _tab(key))
    u1, u2 = _uniforms()
    wo, pdf = gpu_sample(scene, u1, u2)
    d64, d32 = Distr(c, v, np.float64), Distr(c, v, np.float32)
    res_dev = np.abs(d64.eval_cdf_normalized(wo[2]) - u1.astype(np.float64)).max()
    res_f32 = np.abs(d64.eval_cdf_normalized(d32.sample(u1)) - u1.astype(np.float64)).max()
    print(f"table ({key}): CDF residual device {res_dev:.3e}, float32 restatement {res_f32:.3e}")
    assert res_dev <= 4 * res_f32 + 2.0 ** -22
    norm = np.sqrt((wo.astype(np.float64) ** 2).sum(0))
    assert np.abs(norm - 1).max() <= 4 * ULP1
    np.testing.assert_array_equal(pdf, gpu_eval(scene, wo))
    assert (pdf > 0).mean() > 0.99
    if key == "c":   # never inside an interval without mass
        assert wo[2].min() >= np.float32(-0.8) and wo[2].max() <= np.float32(0.85)


def _eval_points(c):
    """Every node, +-1 and random cosines: at least 4096 values (more where
    the table itself has more nodes)."""
    rng = np.random.default_rng(5)
    z = np.concatenate([c, np.float32([-1, 1]), rng.uniform(-1, 1, max(4096 - c.size - 2, 1024)).astype(np.float32)])
    phi = rng.uniform(0, 2 * np.pi, z.size)
    s = np.sqrt(np.maximum(1 - z.astype(np.float64) ** 2, 0))
    return np.stack([(s * np.cos(phi)).astype(np.float32), (s * np.sin(phi)).astype(np.float32), z])


@pytest.mark.parametrize("key", ["a", "b", "c", "d", "e", "f"])
def test_tabulated_eval(key):
    mi = _mi()
    c, v = TABLES[key]
    scene = _phase_scene(mi, _tab(key))
    wo = _eval_points(c)
    assert wo.shape[1] >= 4096
    val = gpu_eval(scene, wo)
    ref = Distr(c, v, np.float64).eval_pdf_normalized(wo[2]) / (2 * np.pi)
    f32 = Distr(c, v, np.float32).eval_pdf_normalized(wo[2]) * np.float32(1 / (2 * np.pi))
    pos = ref > 0
    np.testing.assert_array_equal(val[~pos], 0.0)
    err_dev = (np.abs(val[pos] - ref[pos]) / ref[pos]).max()
    err_f32 = (np.abs(f32[pos] - ref[pos]) / ref[pos]).max()
    print(f"table ({key}): eval relative error device {err_dev:.3e}, float32 restatement {err_f32:.3e}")
    assert err_dev <= 4 * err_f32 + 2.0 ** -22


def test_tabulated_eval_is_zero_outside_the_table():
    mi = _mi()
    c = np.linspace(-0.5, 0.5, 5).astype(np.float32)
    v = np.float32([1, 2, 0.5, 3, 1])
    scene = _phase_scene(mi, {"type": "tabphase", "cost": c, "values": v})
    z = np.float32([-1, -0.75, np.nextafter(np.float32(-0.5), np.float32(-1)), -0.5, 0.0, 0.5,
                    np.nextafter(np.float32(0.5), np.float32(1)), 0.75, 1])
    wo = np.stack([np.sqrt(1 - z * z), np.zeros_like(z), z]).astype(np.float32)
    val = gpu_eval(scene, wo)
    inside = (z >= -0.5) & (z <= 0.5)
    np.testing.assert_array_equal(val[~inside], 0.0)
    ref = Distr(c, v, np.float64).eval_pdf_normalized(z[inside]) / (2 * np.pi)
    np.testing.assert_allclose(val[inside], ref, rtol=1e-6)
    # samples stay inside, with a positive pdf
    u1, u2 = _uniforms()
    wo, pdf = gpu_sample(scene, u1, u2)
    assert wo[2].min() >= -0.5 and wo[2].max() <= 0.5 and (pdf > 0).all()


def test_rayleigh():
    """F(c) = (c^3 + 3c + 4) / 8 is the CDF of 3/8 (1 + c^2) on [-1, 1]: F' <= 3/4
    and the two cube roots are below 1.62, so float32 keeps |F(c) - u1| <= 2^-20."""
    mi = _mi()
    scene = _phase_scene(mi, {"type": "rayleigh", "depolarization": 0})
    u1, u2 = _uniforms()
    wo, pdf = gpu_sample(scene, u1, u2)
    c = wo[2].astype(np.float64)
    res = np.abs((c ** 3 + 3 * c + 4) / 8 - u1.astype(np.float64)).max()
    print(f"rayleigh: CDF residual device {res:.3e}")
    assert res <= 2.0 ** -20
    ref = 3 / (16 * np.pi) * (1 + c * c)
    assert (np.abs(pdf - ref) / ref).max() <= 4 * ULP1
    np.testing.assert_array_equal(pdf, gpu_eval(scene, wo))
    norm = np.sqrt((wo.astype(np.float64) ** 2).sum(0))
    assert np.abs(norm - 1).max() <= 4 * ULP1


@pytest.mark.parametrize("phase", [{"type": "isotropic"}, {"type": "hg", "g": 0.6}])
def test_queries_cover_the_analytic_phase_functions(phase):
    mi = _mi()
    scene = _phase_scene(mi, phase)
    u1, u2 = _uniforms()
    wo, pdf = gpu_sample(scene, u1, u2)
    np.testing.assert_array_equal(pdf, gpu_eval(scene, wo))
    g = phase.get("g", 0.0)
    np.testing.assert_allclose(pdf, hg(g, wo[2].astype(np.float64)), rtol=2e-6)


def test_render_without_a_table_is_refused():
    """A tabulated medium without its table: every entry point that would
    launch returns MH_ERR_INVALID_ARGUMENT first."""
    mi = _mi()
    from mitsuba_hip import _abi as A
    scene = _phase_scene(mi, _tab("b"))
    tables, scene.phase_tables = scene.phase_tables, {}     # handle() then uploads none
    h = scene.handle(0)
    L = A.lib()
    ic = scene.integrator().c()
    n = scene.width * scene.height
    buf = np.zeros(8 * n, np.float32)
    assert L.mh_render(h, C.byref(ic), 0, 1, 0, 0, _p(buf), 0, None) == A.MH_ERR_INVALID_ARGUMENT
    assert b"no table" in L.mh_last_error()
    assert L.mh_render_samples(h, C.byref(ic), 0, 1, 0, 0, _p(buf), 0) == A.MH_ERR_INVALID_ARGUMENT
    assert L.mh_phase_eval(h, 0, 1, _p(buf), _p(buf[4:]), 0) == A.MH_ERR_INVALID_ARGUMENT
    assert b"mh_phase_eval" in L.mh_last_error() and b"no table" in L.mh_last_error()
    assert L.mh_phase_sample(h, 0, 1, _p(buf), _p(buf[4:]), _p(buf[8:]), 0) == A.MH_ERR_INVALID_ARGUMENT
    assert b"mh_phase_sample" in L.mh_last_error() and b"no table" in L.mh_last_error()
    pv = mi.load_dict({"type": "prbvolpath", "max_depth": 4}).c()
    assert L.mh_render_backward(h, C.byref(pv), 0, 1, 0, 0, _p(buf), None, 0, None, None, 0, None) == A.MH_ERR_INVALID_ARGUMENT
    assert b"mh_render_backward" in L.mh_last_error() and b"no table" in L.mh_last_error()
    assert L.mh_render_forward(h, C.byref(pv), 0, 1, 0, 0, 0, None, None, _p(buf), 0, None) == A.MH_ERR_INVALID_ARGUMENT
    assert b"mh_render_forward" in L.mh_last_error() and b"no table" in L.mh_last_error()
    c, v = tables[0]
    bad = v.copy()
    bad[1] = -1
    assert L.mh_scene_set_phase_table(h, 0, c.size, c.ctypes.data_as(A.PF), bad.ctypes.data_as(A.PF)) == A.MH_ERR_INVALID_ARGUMENT
    assert b"mh_scene_set_phase_table" in L.mh_last_error() and b"non-negative" in L.mh_last_error()
    assert L.mh_scene_set_phase_table(h, 0, 1, c.ctypes.data_as(A.PF), v.ctypes.data_as(A.PF)) == A.MH_ERR_INVALID_ARGUMENT
    scene.phase_tables = tables
    scene.upload_phase_table(h, 0)
    assert L.mh_render(h, C.byref(ic), 0, 1, 0, 0, _p(buf), 0, None) == A.MH_OK


# ---------------------------------------------------------------------------
# integrator level
# ---------------------------------------------------------------------------
HET = {"grid_res": 16, "scale": 4.0}
HOM = {"medium_type": "homogeneous", "sigma_t": 0.8, "scale": 1.0}
PHASES = {"d": lambda: _tab("d"), "e": lambda: _tab("e"), "f": lambda: _tab("f"),
          "rayleigh": lambda: {"type": "rayleigh"}}


def _scene(mi, phase, integrator="volpath", w=24, h=20, spp=8, floor=True, max_depth=6, rr_depth=5, **kw):
    """volume_cube (+ the diffuse floor of the parity tests' scenes) with the medium's phase replaced."""
    if "grid_res" in kw:
        kw["grid"] = mi.fbm_grid(kw.pop("grid_res"))
    d = mi.volume_cube(w, h, spp, **kw)
    d["medium1"]["phase"] = phase
    d["integrator"] = {"type": integrator, "max_depth": max_depth, "rr_depth": rr_depth}
    if floor:
        T = mi.Transform4f
        d["floor"] = {"type": "rectangle",
                      "to_world": T.translate([0, -1.2, 0]) @ T.rotate([1, 0, 0], -90) @ T.scale([3, 3, 3]),
                      "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.6, 0.5, 0.4]}}}
    return mi.load_dict(d)


def _gpu_samples(scene, seed, spp, flags):
    from mitsuba_hip import _abi as A
    n = scene.width * scene.height * spp
    out = np.zeros(5 * n, np.float32)
    ic = scene.integrator().c()
    A.check(A.lib().mh_render_samples(scene.handle(0), C.byref(ic), seed, spp, 0, 0, _p(out), flags))
    return out


@pytest.mark.parametrize("integrator", ["volpath", "prbvolpath"])
@pytest.mark.parametrize("shape", [HET, HOM], ids=["heterogeneous", "homogeneous"])
@pytest.mark.parametrize("phase", ["d", "e", "f", "rayleigh"])
def test_engines_agree(phase, shape, integrator):
    """The per-lane megakernel and the phase scheduler (MH_FLAG_WAVEFRONT) call
    the same device functions: bit-identical per sample.  (e) is the size of a
    Mie table (1,801 nodes, 29 KB)."""
    mi = _mi()
    from mitsuba_hip import _abi as A
    scene = _scene(mi, PHASES[phase](), integrator, **shape)
    mega = _gpu_samples(scene, 3, 8, 0)
    wave = _gpu_samples(scene, 3, 8, A.FLAG_WAVEFRONT)
    assert np.isfinite(mega).all() and np.abs(mega[:3 * scene.width * scene.height * 8]).max() > 0
    np.testing.assert_array_equal(mega, wave)


HG_KW = dict(medium_type="homogeneous", sigma_t=1.0, scale=2.0, albedo=0.9, max_depth=8)


@pytest.fixture(scope="module")
def oracle_hg():
    """Image mean of the oracle's analytic HG at g = +0.6 and -0.6 over seeds
    0-7 (mean, seed-to-seed standard deviation)."""
    import mitsuba_hip as mi
    out = {}
    for g in (0.6, -0.6):
        scene = mi.load_dict(mi.volume_cube(16, 16, 256, g=g, **HG_KW))
        means = [float(O.develop(O.render(scene, seed=s, spp=256)).astype(np.float64).mean()) for s in range(8)]
        out[g] = (float(np.mean(means)), float(np.std(means, ddof=1)))
    return out


def _tabulated_hg_mean(mi, reverse):
    c = np.linspace(-1.0, 1.0, 2049)
    v = hg(0.6, c)
    d = mi.volume_cube(16, 16, 256, g=0.6, **HG_KW)
    d["medium1"]["phase"] = {"type": "tabphase", "cost": c, "values": v[::-1] if reverse else v}
    scene = mi.load_dict(d)
    img = mi.develop(scene, mi.render_film(scene, seed=100, spp=256)).cpu().numpy()
    return float(img.astype(np.float64).mean())


def test_tabulated_hg_matches_the_oracle(oracle_hg):
    """HG(0.6) tabulated on 2,049 nodes uniform in cos (interpolation bias about
    3e-5 relative) against the oracle's analytic HG: the image mean within 4
    sigma of the difference of one render and the 8-seed mean.  The reversed
    table must match g = -0.6 instead and miss g = +0.6 by more than 8 sigma,
    so a flipped cosine convention cannot pass."""
    mi = _mi()
    (mu, sigma), (mu_r, sigma_r) = oracle_hg[0.6], oracle_hg[-0.6]
    fwd, rev = _tabulated_hg_mean(mi, False), _tabulated_hg_mean(mi, True)
    print(f"oracle hg +0.6: {mu:.4f} +- {sigma:.4f}, -0.6: {mu_r:.4f} +- {sigma_r:.4f}; tabulated {fwd:.4f}, reversed {rev:.4f}")
    assert abs(fwd - mu) <= 4 * sigma * np.sqrt(1 + 1 / 8)
    assert abs(rev - mu_r) <= 4 * sigma * np.sqrt(1 + 1 / 8)
    assert abs(rev - mu) > 8 * sigma


@pytest.mark.parametrize("phase", ["d", "rayleigh"])
def test_white_furnace(phase):
    """test_volpath_white_furnace_gpu's scene and bound."""
    mi = _mi()
    d = mi.volume_cube(32, 32, 256, grid=mi.fbm_grid(32), albedo=1.0, sky=1.0, sun=None, scale=5.0, max_depth=-1)
    d["medium1"]["phase"] = PHASES[phase]()
    scene = mi.load_dict(d)
    img = mi.develop(scene, mi.render_film(scene, seed=0, spp=256)).cpu().numpy()
    assert abs(img.mean() - 1.0) < 0.01


@pytest.mark.parametrize("table", ["d", "e"])
def test_backward_paths_agree(monkeypatch, table):
    """sigma_t grid, albedo and floor reflectance gradients with a tabulated
    phase function: the default scheduler, the per-sample kernel
    (MH_PVP_SCHED=0) and the NEE-replaying kernel (MH_PVP_NEE_LOG=0), at
    test_prbvolpath_backward_parity's tolerance.  (e) is the size of a Mie
    table."""
    mi = _mi()
    import torch
    keys = ["medium1.sigma_t.data", "medium1.albedo.value", "floor.bsdf.reflectance.value"]
    gi = np.random.default_rng(4).standard_normal((20, 24, 3)).astype(np.float32)
    out = {}
    for mode, env in (("sched", None), ("sched_off", "MH_PVP_SCHED"), ("replay", "MH_PVP_NEE_LOG")):
        if env:
            monkeypatch.setenv(env, "0")
        scene = _scene(mi, _tab(table), "prbvolpath", **HET)
        params = mi.traverse(scene)
        g = mi.render_backward(scene, params, torch.from_numpy(gi).cuda(), keys, scene.integrator(), seed=7, spp=8)
        out[mode] = [a.cpu().numpy() for a in g]
        if env:
            monkeypatch.delenv(env)
    for mode in ("sched_off", "replay"):
        for k, a, b in zip(keys, out[mode], out["sched"]):
            assert a.shape == b.shape and np.abs(b).max() > 0, (mode, k)
            np.testing.assert_allclose(a, b, rtol=2e-3, atol=1e-7 + 2e-4 * np.abs(b).max(), err_msg=f"{mode} {k}")


def test_albedo_gradient_vs_finite_differences():
    """rr_depth > max_depth = 3: no path depends on the albedo, so the
    backward at the render's own seed is the derivative of that render."""
    mi = _mi()
    import torch
    scene = _scene(mi, _tab("d"), "prbvolpath", max_depth=3, rr_depth=8, **HET)
    integ = scene.integrator()
    params = mi.traverse(scene)
    key = "medium1.albedo.value"
    H, W = scene.height, scene.width
    gi = torch.full((H, W, 3), 1.0 / (H * W * 3), dtype=torch.float32, device="cuda")
    seed, spp, eps = 5, 8, 1e-3
    g = mi.render_backward(scene, params, gi, [key], integ, seed=seed, spp=spp)[0].cpu().numpy()
    base = params[key].detach().clone()
    for c in range(3):
        vals = []
        for s in (+1, -1):
            v = base.clone()
            v[c] += s * eps
            params[key] = v
            params.update()
            vals.append(mi.develop(scene, mi.render_film(scene, integ, seed=seed, spp=spp)).double().mean().item())
        fd = (vals[0] - vals[1]) / (2 * eps)
        print(f"albedo[{c}]: backward {g[c]:.6e}, central differences {fd:.6e}")
        assert np.isclose(g[c], fd, rtol=2e-2), (c, g[c], fd)
        params[key] = base
        params.update()


def test_autograd_through_render():
    """mi.render with autograd on a tabphase scene: sigma_t grid and albedo
    receive gradients as with HG; the table's values refuse."""
    mi = _mi()
    from mitsuba_hip import _abi as A
    scene = _scene(mi, _tab("d"), "prbvolpath", **HET)
    params = mi.traverse(scene)
    for k in ("medium1.sigma_t.data", "medium1.albedo.value"):
        params[k].requires_grad_()
    img = mi.render(scene, params, spp=8, seed=3)
    img.mean().backward()
    for k in ("medium1.sigma_t.data", "medium1.albedo.value"):
        g = params[k].grad
        assert g is not None and g.shape == params[k].shape and bool(g.abs().max() > 0) and bool(g.isfinite().all())
    with pytest.raises(A.MitsubaHipError, match="not differentiable"):
        params.param_id("medium1.phase_function.values")


def test_update_equals_a_fresh_scene():
    mi = _mi()
    scene = _scene(mi, _tab("d"), **HET)
    before = mi.render_film(scene, seed=2, spp=8, deterministic=True).cpu().numpy()
    params = mi.traverse(scene)
    c, _ = TABLES["d"]
    new = hg(0.3, c.astype(np.float64)).astype(np.float32)
    params["medium1.phase_function.values"] = new
    params.update()
    after = mi.render_film(scene, seed=2, spp=8, deterministic=True).cpu().numpy()
    fresh = _scene(mi, {"type": "tabphase", "cost": c, "values": new}, **HET)
    ref = mi.render_film(fresh, seed=2, spp=8, deterministic=True).cpu().numpy()
    assert not np.array_equal(before, after)
    np.testing.assert_array_equal(after, ref)
