"""GPU: volpath / prbvolpath against the CPU oracle on the medium topologies
of vol_cases.py -- several media in one scene (grid_offset, per-medium slots),
mixed medium types (both vol_flags at once), sensor.medium, the medium flags,
grids that are not their boundary's box, a mesh boundary, an object inside a
medium, an area light through a medium and two tabulated phase tables.

The criteria are test_gpu_parity.py's (per sample, film, gradient), the
oracle on these layouts is pinned by test_vol_topologies_oracle.py.  Every
test runs at 24 x 20 @ 8 spp; the oracle's results are computed once per
(case, integrator) and shared.

Which test runs which code:
  grid_offset != 0 in grid_eval, sigma_slot / albedo_slot by medium,
  a second grid's bitmap slot and corner block    three_media, camera_in_third: per_sample, backward,
                                                  grid_corner_scatter, deterministic_gradient, render_forward
  mh_scene_update_medium at grid_offset != 0      test_update_second_grid_equals_a_fresh_scene
  both vol_flags (handle_null, nee_hom) at once   three_media, camera_in_third, nested_media
  sensor.medium (S.camera_medium)                 camera_inside (heterogeneous), camera_in_third (homogeneous)
  sample_emitters / has_spectral_extinction       no_emitter_sampling, no_spectral_extinction(_s37)
  general affine grid_to_local, bbox != shape     three_media, grid_inside_cube, use_grid_bbox, mesh_boundary
  mesh boundary, object in a medium, area light   mesh_boundary, object_inside, area_light
  a boundary between two media                    nested_media
  two phase tables, tab_offset != 0, LDS staging  test_two_tables_*"""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_py as O
import vol_cases as VC
from phase_cases import TABLES, Distr, hg
from test_gpu_parity import _film_close
from test_gpu_phase_functions import _eval_points, _uniforms, gpu_eval, gpu_sample

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 24, 20, 8, 3
PRIMAL = [c for c in VC.CASES if c != "two_tables"]


def _mi():
    import mitsuba_hip as mi
    if not mi.is_available():
        pytest.fail("no HIP device / native library: the GPU tests need an MI355X")
    return mi


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _gpu_samples(scene, seed=SEED, spp=SPP, flags=0):
    from mitsuba_hip import _abi as A
    n = scene.width * scene.height * spp
    out = np.zeros(5 * n, np.float32)
    ic = scene.integrator().c()
    A.check(A.lib().mh_render_samples(scene.handle(0), C.byref(ic), seed, spp, 0, 0, _p(out), flags))
    return out[:3 * n].reshape(3, n).T, out[3 * n:].reshape(2, n).T


def _scene(case, integrator, **kw):
    import mitsuba_hip as mi
    return mi.load_dict(VC.CASES[case](mi, integrator, W, H, SPP, **kw))


@functools.lru_cache(maxsize=None)
def _oracle_samples(case, integrator):
    scene = _scene(case, integrator)
    L, pos, _ = O.sample_range(scene, scene.integrator(), SEED, SPP, 0, W * H * SPP)
    L.setflags(write=False)
    pos.setflags(write=False)
    return L, pos


# the measured share of non-zero samples (volpath, prbvolpath) on the oracle;
# a case must reach half of it.  None: not measured, any non-zero sample will do
SHARE = {"three_media": (1.00, 0.51), "camera_inside": (1.00, 0.066), "no_emitter_sampling": (0.98, 0.22),
         "object_inside": (1.00, 0.26), "area_light": (0.34, None), "grid_inside_cube": (1.00, 0.25),
         "mesh_boundary": (1.00, 0.37)}
SHARE.update({c: (None, None) for c in VC.CASES if c not in SHARE})


def _coverage(case, integrator, scene, rL):
    """The case runs the code it is there for (on the oracle's samples)."""
    import mitsuba_hip as mi
    from mitsuba_hip import _abi as A
    share = (np.abs(rL).max(1) > 0).mean()
    want = SHARE[case][integrator == "prbvolpath"]
    assert share >= (0.5 * want if want else 1.0 / rL.shape[0]), f"non-zero share {share}"
    d = scene.desc
    if case == "three_media":
        assert d.n_media == 3 and d.n_shapes == 4
        assert [scene.medium(i).type for i in range(3)] == [A.MEDIUM_HETEROGENEOUS, A.MEDIUM_HETEROGENEOUS,
                                                            A.MEDIUM_HOMOGENEOUS]
        assert scene.medium(0).grid_offset == 0 and scene.medium(1).grid_offset == 16 ** 3
        assert tuple(scene.medium(1).grid_res) == (5, 9, 7)
    elif case == "camera_inside":
        assert d.sensor.medium == 0
    elif case == "camera_in_third":
        assert d.sensor.medium == 2 and d.n_media == 3 and scene.medium(2).type == A.MEDIUM_HOMOGENEOUS
    elif case in ("no_emitter_sampling", "no_spectral_extinction", "no_spectral_extinction_s37"):
        flag = A.MEDIUM_NO_EMITTER_SAMPLING if case == "no_emitter_sampling" else A.MEDIUM_NO_SPECTRAL_EXTINCTION
        assert scene.medium(0).flags == flag and list(scene.medium(0).albedo) != [scene.medium(0).albedo[0]] * 3
        # the flag changes the result: the same scene with the flag at its default.  Not so for
        # has_spectral_extinction at scale 4 (a power-of-two majorant: both branches round
        # alike) and in prbvolpath, which does not read it; volpath at scale 3.7 tells
        if case == "no_emitter_sampling" or (case == "no_spectral_extinction_s37" and integrator == "volpath"):
            other = mi.load_dict(VC.base(mi, integrator, W, H, SPP, albedo=[0.9, 0.5, 0.2],
                                         scale=scene.medium(0).scale))
            oL, _, _ = O.sample_range(other, other.integrator(), SEED, SPP, 0, rL.shape[0])
            assert (np.abs(oL - rL).max(1) > 0).mean() > 0.1
    elif case == "grid_inside_cube":
        m = scene.medium(0)
        assert np.allclose(m.bbox_min, [-0.5, -0.7, -0.2]) and np.allclose(m.bbox_max, [0.5, 0.5, 0.7])
    elif case == "use_grid_bbox":
        bL, _ = _oracle_samples_base(integrator)
        np.testing.assert_array_equal(rL, bL)
    elif case == "mesh_boundary":
        assert d.shapes[0].type == A.SHAPE_MESH and d.shapes[0].face_count == 8 and d.shapes[0].interior_medium == 0
    elif case == "object_inside":
        assert d.n_shapes == 2 and d.shapes[1].exterior_medium == 0 and d.shapes[1].interior_medium == A.INVALID
    elif case == "nested_media":
        core = d.shapes[scene.shape_names.index("core")]
        assert d.n_media == 2 and (core.interior_medium, core.exterior_medium) == (1, 0)
    elif case == "area_light":
        assert d.n_emitters == 1 and d.emitters[0].type == A.EMITTER_AREA and d.environment == A.INVALID


@functools.lru_cache(maxsize=None)
def _oracle_samples_base(integrator):
    import mitsuba_hip as mi
    scene = mi.load_dict(VC.base(mi, integrator, W, H, SPP))
    L, pos, _ = O.sample_range(scene, scene.integrator(), SEED, SPP, 0, W * H * SPP)
    return L, pos


def _assert_per_sample(L, pos, rL, rpos):
    np.testing.assert_array_equal(pos, rpos)
    exact = np.all(L == rL, axis=1)
    assert exact.mean() >= 0.999, f"bit-exact fraction {exact.mean()}"
    close = np.all(np.abs(L - rL) <= 1e-4 * np.maximum(1, np.abs(rL)), axis=1)
    assert close.mean() >= 0.999, f"close fraction {close.mean()}"


# ---------------------------------------------------------------------------
# primal, per sample
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["mega", "wavefront", "wavefront-rounds", "wavefront-finish1"])
@pytest.mark.parametrize("case", PRIMAL)
def test_volpath_per_sample(case, mode, monkeypatch):
    """The modes of test_volpath_per_sample_parity, set the same way."""
    _mi()
    from mitsuba_hip import _abi as A
    if mode != "wavefront" and mode != "mega":
        monkeypatch.setenv("MH_VOL_MODE", "rounds")
    if mode == "wavefront-finish1":
        monkeypatch.setenv("MH_VW_ROUNDS", "1")
    mode = mode.split("-")[0]
    scene = _scene(case, "volpath")
    rL, rpos = _oracle_samples(case, "volpath")
    _coverage(case, "volpath", scene, rL)
    L, pos = _gpu_samples(scene, flags=A.FLAG_WAVEFRONT if mode == "wavefront" else 0)
    _assert_per_sample(L, pos, rL, rpos)
    if case == "use_grid_bbox":
        bL, _ = _gpu_samples(_scene_base("volpath"), flags=A.FLAG_WAVEFRONT if mode == "wavefront" else 0)
        np.testing.assert_array_equal(L, bL)


def _scene_base(integrator):
    import mitsuba_hip as mi
    return mi.load_dict(VC.base(mi, integrator, W, H, SPP))


@pytest.mark.parametrize("mode", ["mega", "wavefront"])
@pytest.mark.parametrize("case", PRIMAL)
def test_prbvolpath_per_sample(case, mode):
    _mi()
    from mitsuba_hip import _abi as A
    scene = _scene(case, "prbvolpath")
    assert scene.integrator().type == "prbvolpath"
    rL, rpos = _oracle_samples(case, "prbvolpath")
    _coverage(case, "prbvolpath", scene, rL)
    flags = A.FLAG_WAVEFRONT if mode == "wavefront" else 0
    L, pos = _gpu_samples(scene, flags=flags)
    _assert_per_sample(L, pos, rL, rpos)
    if case == "use_grid_bbox":
        bL, _ = _gpu_samples(_scene_base("prbvolpath"), flags=flags)
        np.testing.assert_array_equal(L, bL)


# ---------------------------------------------------------------------------
# film
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", ["volpath", "prbvolpath"])
@pytest.mark.parametrize("case", ["three_media", "camera_inside"])
def test_film(case, integrator):
    """render_film in both execution modes against the oracle's film; the two
    modes trace the same rays (test_volpath_wavefront_matches_megakernel_stats)."""
    mi = _mi()
    from mitsuba_hip import _abi as A
    scene = _scene(case, integrator)
    ref = O.render(scene, seed=5, spp=SPP)
    assert np.abs(ref[..., :3]).max() > 0
    st = {}
    for mode in ("mega", "wavefront"):
        st[mode] = A.Stats()
        film = mi.render_film(scene, seed=5, spp=SPP, mode=mode, stats=st[mode]).cpu().numpy()
        ok, frac = _film_close(film, ref)
        assert ok, f"{mode}: film parity {frac}"
    assert st["wavefront"].mode == 3 and st["mega"].mode == 0
    assert (st["wavefront"].rays_closest, st["wavefront"].rays_shadow) == \
        (st["mega"].rays_closest, st["mega"].rays_shadow)
    assert st["mega"].rays_closest > 0


# ---------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------
def _grad_in(seed=4):
    return np.random.default_rng(seed).standard_normal((H, W, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _oracle_backward(case, seed=7, gi_seed=4):
    """{key: gradient} of every key of the case."""
    import mitsuba_hip as mi
    scene = _scene(case, "prbvolpath")
    params = mi.traverse(scene)
    keys = VC.KEYS[case]
    ref = O.render_backward(scene, scene.integrator(), seed, SPP, _grad_in(gi_seed),
                            [params.param_id(k) for k in keys], [tuple(params[k].shape) for k in keys])
    for r in ref:
        r.setflags(write=False)
    return dict(zip(keys, ref))


ENGINE_ENV = {"single": {}, "main4": {"MH_PVP_MAIN_CAP": "4"}, "sched_nee2": {"MH_PVP_NEE_CAP": "2"},
              "sched_off": {"MH_PVP_SCHED": "0"}, "twopass": {"MH_PVP_SINGLE": "0"},
              "cap2": {"MH_PVP_NEE_CAP": "2", "MH_PVP_SINGLE": "0"}, "replay": {"MH_PVP_NEE_LOG": "0"}}
BACKWARD = [(c, e) for c in PRIMAL for e in ("single", "sched_off", "replay")] + \
           [("three_media", e) for e in ("main4", "sched_nee2", "cap2", "twopass")]


def _gpu_backward(mi, scene, params, keys, gi, seed=7, **kw):
    import torch
    g = mi.render_backward(scene, params, torch.from_numpy(gi).cuda(), keys, scene.integrator(), seed=seed,
                           spp=SPP, **kw)
    return [x.cpu().numpy() for x in g]


@pytest.mark.parametrize("case,engine", BACKWARD)
def test_prbvolpath_backward(case, engine, monkeypatch):
    """Every key of the case against the oracle, on the engines of
    test_prbvolpath_backward_parity and at its tolerance.  three_media's first
    call holds two grid parameters (two bitmap slots, two corner blocks) and
    the homogeneous sigma_t next to an albedo (small slots); no call holds
    more than four small parameters."""
    for k, v in ENGINE_ENV[engine].items():
        monkeypatch.setenv(k, v)
    mi = _mi()
    scene = _scene(case, "prbvolpath")
    params = mi.traverse(scene)
    ref = _oracle_backward(case)
    assert set(ref) == set(VC.KEYS[case])
    for keys in VC.key_calls(case):
        for k, a in zip(keys, _gpu_backward(mi, scene, params, keys, _grad_in())):
            b = ref[k]
            assert a.shape == b.shape, k
            assert np.abs(b).max() > 0, k
            np.testing.assert_allclose(a, b, rtol=2e-3, atol=1e-7 + 2e-4 * np.abs(b).max(), err_msg=k)


GRID_CASES = ["three_media", "grid_inside_cube", "mesh_boundary"]


@pytest.mark.parametrize("case", GRID_CASES)
def test_prbvolpath_grid_corner_scatter(case, monkeypatch):
    """As test_prbvolpath_grid_corner_scatter: the corner blocks (default)
    against float atomics straight into the grid gradient (MH_GRID_CORNER=0)."""
    mi = _mi()
    scene = _scene(case, "prbvolpath")
    params = mi.traverse(scene)
    keys = VC.key_calls(case)[0]
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MH_GRID_CORNER", mode)
        out[mode] = _gpu_backward(mi, scene, params, keys, _grad_in())
    ref = _oracle_backward(case)
    for k, a, b in zip(keys, out["1"], out["0"]):
        scale = np.abs(ref[k]).max()
        assert a.shape == ref[k].shape and scale > 0, k
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-6 * scale, err_msg=k)
        np.testing.assert_allclose(a, ref[k], rtol=2e-3, atol=1e-7 + 2e-4 * scale, err_msg=k)


@pytest.mark.parametrize("mode", ["sched", "sched_off", "replay"])
@pytest.mark.parametrize("case", GRID_CASES)
def test_prbvolpath_deterministic_gradient(case, mode, monkeypatch):
    """As test_prbvolpath_deterministic_grid_gradient, on its three engines:
    bit-identical over three runs, equal to the float run up to the order of
    the adds."""
    if mode == "sched_off":
        monkeypatch.setenv("MH_PVP_SCHED", "0")
    elif mode == "replay":
        monkeypatch.setenv("MH_PVP_NEE_LOG", "0")
    mi = _mi()
    import torch
    scene = _scene(case, "prbvolpath")
    params = mi.traverse(scene)
    keys = VC.key_calls(case)[0]
    gi = torch.from_numpy(_grad_in()).cuda()
    runs = [mi.render_backward(scene, params, gi, keys, scene.integrator(), seed=7, spp=SPP, deterministic=True)
            for _ in range(3)]
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b)
    flt = mi.render_backward(scene, params, gi, keys, scene.integrator(), seed=7, spp=SPP)
    ref = _oracle_backward(case)
    for k, a, b in zip(keys, runs[0], flt):
        a, b = a.cpu().numpy(), b.cpu().numpy()
        scale = np.abs(ref[k]).max()
        assert scale > 0, k
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-6 * scale, err_msg=k)
        np.testing.assert_allclose(a, ref[k], rtol=2e-3, atol=1e-7 + 2e-4 * scale, err_msg=k)


# ---------------------------------------------------------------------------
# forward mode
# ---------------------------------------------------------------------------
def _tangents(params):
    rng = np.random.default_rng(9)
    return {"medium2.sigma_t.data": rng.random(tuple(params["medium2.sigma_t.data"].shape)).astype(np.float32),
            "medium3.sigma_t.value": np.array([0.7], np.float32),
            "medium2.albedo.value": np.array([0.1, -0.2, 0.3], np.float32)}


def _gpu_forward(mi, scene, params, tans, seed=7):
    import torch
    t = {k: torch.as_tensor(v).cuda() for k, v in tans.items()}
    return mi.render_forward(scene, params, t, scene.integrator(), seed=seed, spp=SPP).cpu().numpy()


@pytest.mark.parametrize("which", ["medium2.sigma_t.data", "medium3.sigma_t.value", "medium2.albedo.value", "all"])
def test_render_forward_three_media(which):
    """test_render_forward_prbvolpath_parity's criterion, one tangent at a time and all three at once."""
    mi = _mi()
    scene = _scene("three_media", "prbvolpath")
    params = mi.traverse(scene)
    tans = _tangents(params)
    if which != "all":
        tans = {which: tans[which]}
    img = _gpu_forward(mi, scene, params, tans)
    film = O.render_forward(scene, scene.integrator(), 7, SPP, [params.param_id(k) for k in tans],
                            list(tans.values()))
    ref = O.develop(film, scene.desc.sensor.pixel_format)
    assert np.abs(ref).max() > 0
    d = np.abs(img - ref)
    ok = d <= 1e-4 + 5e-3 * np.abs(ref)
    assert ok.mean() >= 0.99, f"{(~ok).sum()} of {ok.size} off, max {d.max():.3e}"


def test_render_forward_adjoint_identity_three_media():
    """<grad_in, J t> = <J^T grad_in, t> at test_render_forward_adjoint_identity_config3's tolerance."""
    mi = _mi()
    scene = _scene("three_media", "prbvolpath")
    params = mi.traverse(scene)
    tans = _tangents(params)
    img = _gpu_forward(mi, scene, params, tans, seed=3)
    gi = np.random.default_rng(1).random((H, W, 3)).astype(np.float32) / (H * W * 3)
    g = _gpu_backward(mi, scene, params, list(tans), gi, seed=3)
    lhs = float((gi.astype(np.float64) * img).sum())
    rhs = float(sum((a.astype(np.float64) * tans[k].reshape(a.shape)).sum() for k, a in zip(tans, g)))
    assert abs(rhs) > 0
    assert abs(lhs - rhs) <= 2e-3 * abs(rhs), (lhs, rhs)


# ---------------------------------------------------------------------------
# updates
# ---------------------------------------------------------------------------
def test_update_second_grid_equals_a_fresh_scene():
    """SceneParameters.update on three_media: medium2's grid (the grid_offset
    != 0 scatter of mh_scene_update_medium) and medium3's sigma_t, then
    medium1's albedo; after each step the samples equal, bit for bit, those of
    a scene freshly loaded with these values.  After the first step medium1's
    contribution is unchanged: every sample that the oracle leaves unchanged
    (its path and its NEE walks meet neither cube 2 nor cube 3) keeps its bits
    on the device.  Over cube 1 (the left third of the image) that is nearly
    every non-zero sample, 96.3 %; over cube 2 fewer than half."""
    mi = _mi()
    scene = _scene("three_media", "prbvolpath")
    before, _ = _gpu_samples(scene)
    params = mi.traverse(scene)
    g1 = (VC.crop_795(mi) * 1.7 + 0.05).astype(np.float32)
    params["medium2.sigma_t.data"] = g1[..., None]
    params["medium3.sigma_t.value"] = [1.3]
    params.update()
    d = VC.three_media(mi, "prbvolpath", W, H, SPP)
    d["medium2"]["sigma_t"]["data"] = g1
    d["medium3"]["sigma_t"] = 1.3
    step1, _ = _gpu_samples(scene)
    np.testing.assert_array_equal(step1, _gpu_samples(mi.load_dict(d))[0])
    px = (np.arange(W * H * SPP) // SPP) % W          # the sample's pixel column
    lit = np.abs(before).max(1) > 0
    same = np.all(before == step1, axis=1)
    left, right = lit & (px < W // 3), lit & (px >= 2 * W // 3)
    assert left.sum() > 100 and right.sum() > 100
    fresh = mi.load_dict(d)
    n = W * H * SPP
    o0 = O.sample_range(_scene("three_media", "prbvolpath"), scene.integrator(), SEED, SPP, 0, n)[0]
    o1 = O.sample_range(fresh, fresh.integrator(), SEED, SPP, 0, n)[0]
    untouched = np.all(o0 == o1, axis=1)
    print(f"unchanged after updating medium2 / medium3: oracle {untouched[left].mean():.3f} / device "
          f"{same[left].mean():.3f} over cube 1, {untouched[right].mean():.3f} / {same[right].mean():.3f} over cube 2")
    assert same[untouched].all()
    assert untouched[left].mean() > 0.95 and untouched[right].mean() < 0.5
    params["medium1.albedo.value"] = [0.5, 0.7, 0.8]
    params.update()
    d["medium1"]["albedo"] = [0.5, 0.7, 0.8]
    step2, _ = _gpu_samples(scene)
    assert not np.array_equal(step1, step2)
    np.testing.assert_array_equal(step2, _gpu_samples(mi.load_dict(d))[0])


# ---------------------------------------------------------------------------
# two tabulated phase tables in one scene
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("medium", [1, 0])
def test_two_tables_function_level(medium):
    """mh_phase_sample / mh_phase_eval on medium index 1 -- the second table
    of the shared buffer, 1,801 nodes behind the 33 of medium 0 -- and on
    medium 0, against the Distr restatement and with the bounds of
    test_tabulated_sampling / test_tabulated_eval."""
    _mi()
    scene = _scene("two_tables", "volpath")
    small = VC.small_table()
    c, v = TABLES["e"] if medium == 1 else (small["cost"], small["values"])
    assert (c.size, scene.phase_tables[medium][0].size) == ((1801, 1801) if medium == 1 else (33, 33))
    d64, d32 = Distr(c, v, np.float64), Distr(c, v, np.float32)
    u1, u2 = _uniforms()
    wo, pdf = gpu_sample(scene, u1, u2, medium)
    res_dev = np.abs(d64.eval_cdf_normalized(wo[2]) - u1.astype(np.float64)).max()
    res_f32 = np.abs(d64.eval_cdf_normalized(d32.sample(u1)) - u1.astype(np.float64)).max()
    print(f"medium {medium}: CDF residual device {res_dev:.3e}, float32 restatement {res_f32:.3e}")
    assert res_dev <= 4 * res_f32 + 2.0 ** -22
    np.testing.assert_array_equal(pdf, gpu_eval(scene, wo, medium))
    pts = _eval_points(c)
    val = gpu_eval(scene, pts, medium)
    ref = d64.eval_pdf_normalized(pts[2]) / (2 * np.pi)
    f32 = d32.eval_pdf_normalized(pts[2]) * np.float32(1 / (2 * np.pi))
    pos = ref > 0
    np.testing.assert_array_equal(val[~pos], 0.0)
    err_dev = (np.abs(val[pos] - ref[pos]) / ref[pos]).max()
    err_f32 = (np.abs(f32[pos] - ref[pos]) / ref[pos]).max()
    print(f"medium {medium}: eval relative error device {err_dev:.3e}, float32 restatement {err_f32:.3e}")
    assert err_dev <= 4 * err_f32 + 2.0 ** -22


@pytest.mark.parametrize("integrator", ["volpath", "prbvolpath"])
def test_two_tables_engines_agree(integrator):
    """test_engines_agree on two_tables: the megakernel reads both tables from
    global memory, the phase scheduler from its LDS copy of the whole buffer."""
    _mi()
    from mitsuba_hip import _abi as A
    scene = _scene("two_tables", integrator)
    assert sorted(scene.phase_tables) == [0, 1]
    mega, pos = _gpu_samples(scene)
    wave, wpos = _gpu_samples(scene, flags=A.FLAG_WAVEFRONT)
    assert np.isfinite(mega).all() and np.abs(mega).max() > 0
    np.testing.assert_array_equal(mega, wave)
    np.testing.assert_array_equal(pos, wpos)
    # the tables matter: three_media's analytic phase functions give other samples
    assert not np.array_equal(mega, _gpu_samples(_scene("three_media", integrator))[0])


def _hg_table(g, n=2049):
    c = np.linspace(-1.0, 1.0, n)
    return {"type": "tabphase", "cost": c, "values": hg(g, c)}


def _hg_scene(mi, phase2):
    """three_media with medium2's phase function replaced, seen so that cube 2
    fills the image: from (0.9, 0, 4) towards it with a 12 degree field of
    view.  The sun then reaches the sensor by scattering at about 107 degrees,
    where HG(+0.6) and HG(-0.6) differ by a factor of 2.2."""
    d = VC.three_media(mi, "volpath", 16, 16, 256, max_depth=8)
    d["medium2"]["phase"] = phase2
    d["sensor"]["to_world"] = mi.Transform4f.look_at(origin=[0.9, 0.0, 4.0], target=[0.85, -0.05, 0.0], up=[0, 1, 0])
    d["sensor"]["fov"] = 12.0
    return mi.load_dict(d)


@pytest.fixture(scope="module")
def oracle_hg2():
    """Image mean of the oracle's analytic HG in medium2 at g = +0.6 and -0.6
    over seeds 0-7 (mean, seed-to-seed standard deviation)."""
    import mitsuba_hip as mi
    out = {}
    for g in (0.6, -0.6):
        scene = _hg_scene(mi, {"type": "hg", "g": g})
        means = [float(O.develop(O.render(scene, seed=s, spp=256)).astype(np.float64).mean()) for s in range(8)]
        out[g] = (float(np.mean(means)), float(np.std(means, ddof=1)))
    return out


def test_two_tables_tabulated_hg_matches_the_oracle(oracle_hg2):
    """medium2 (medium index 1, behind two other media) a tabulated HG(0.6) on
    the 2,049 nodes of test_tabulated_hg_matches_the_oracle, medium1 its
    analytic HG; the oracle with the analytic HG in medium2.  That test's
    criterion, all of it, at its 16 x 16 @ 256: the image mean within 4 sigma
    of the difference of one render and the oracle's 8-seed mean; the reversed
    table matches g = -0.6 instead and misses g = +0.6 by more than 8 sigma, so
    a flipped cosine convention cannot pass.  On this view the oracle's two
    means, 0.3808 +- 0.0014 and 0.4576 +- 0.0026, are 53 sigma apart."""
    mi = _mi()
    (mu, sigma), (mu_r, sigma_r) = oracle_hg2[0.6], oracle_hg2[-0.6]
    assert abs(mu - mu_r) > 16 * sigma     # the view tells the two apart
    dev = {}
    for reverse in (False, True):
        t = _hg_table(0.6)
        if reverse:
            t["values"] = t["values"][::-1]
        scene = _hg_scene(mi, t)
        assert sorted(scene.phase_tables) == [1]
        img = mi.develop(scene, mi.render_film(scene, seed=100, spp=256)).cpu().numpy()
        dev[reverse] = float(img.astype(np.float64).mean())
    fwd, rev = dev[False], dev[True]
    print(f"oracle hg +0.6: {mu:.4f} +- {sigma:.4f}, -0.6: {mu_r:.4f} +- {sigma_r:.4f}; "
          f"tabulated {fwd:.4f}, reversed {rev:.4f}")
    assert abs(fwd - mu) <= 4 * sigma * np.sqrt(1 + 1 / 8)
    assert abs(rev - mu_r) <= 4 * sigma * np.sqrt(1 + 1 / 8)
    assert abs(rev - mu) > 8 * sigma


def test_two_tables_update_first_table():
    """medium1's table replaced while medium2 keeps its own
    (mh_scene_set_phase_table concatenates every table again): renders like a
    freshly loaded scene, and unlike before."""
    mi = _mi()
    scene = _scene("two_tables", "volpath")
    before = mi.render_film(scene, seed=2, spp=SPP, deterministic=True).cpu().numpy()
    params = mi.traverse(scene)
    c = VC.small_table()["cost"]
    new = hg(-0.4, c.astype(np.float64)).astype(np.float32)
    params["medium1.phase_function.values"] = new
    params.update()
    after = mi.render_film(scene, seed=2, spp=SPP, deterministic=True).cpu().numpy()
    fresh = _scene("two_tables", "volpath", phase1={"type": "tabphase", "cost": c, "values": new})
    ref = mi.render_film(fresh, seed=2, spp=SPP, deterministic=True).cpu().numpy()
    assert not np.array_equal(before, after)
    np.testing.assert_array_equal(after, ref)
