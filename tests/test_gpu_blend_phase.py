"""GPU: the blend phase function (phase/blendphase.cpp with two children and the
volume weight_0; mh_scene_set_phase_blend).

Function level: mh_phase_sample_at / mh_phase_eval_at run the device functions
the volumetric integrators call.  A blend's sample must be bit-equal to the
selected child's own sample (mh_phase_sample of a scene that carries the child
alone), selected by the reference's strict inequalities; its value must be
w e0 + (1 - w) e1 of the children's own device values, with w the float32
constant or the weight grid's trilinear lookup (blend_cases.weight_lookup in
float64; the float32 restatement's own error sets the bound as in
test_gpu_phase_functions.py: 4 x + 2^-22).

Integrator level: weights 1 and 0 (constant, grid, clamped grid) render the
pure child scene's samples, the execution engines agree bit for bit, identical
children render like the child, a blend of two tables renders like the single
mixed table (the sampling proportions), the white furnace stays white, the
prbvolpath gradients of sigma_t, albedo and reflectance work through a blend,
and updated weights / child tables render like a freshly loaded scene.  The
oracle never sees a blend."""
import ctypes as C

import numpy as np
import pytest

from blend_cases import CHILD_PAIRS, blend, const_grid, falling_grid, tab, weight_grid, weight_lookup
from phase_cases import TABLES, hg

pytestmark = pytest.mark.gpu

ULP1 = 2.0 ** -23
W_CONST = np.float32(0.2)


def _mi():
    import mitsuba_hip as mi
    if not mi.is_available():
        pytest.fail("no HIP device / native library: the GPU tests need an MI355X")
    return mi


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _phase_scene(mi, phase):
    """A small homogeneous cube whose medium 0 carries `phase` (function-level queries)."""
    d = mi.volume_cube(8, 8, 1, medium_type="homogeneous", sigma_t=1.0, scale=1.0)
    d["medium1"]["phase"] = phase
    return mi.load_dict(d)


def gpu_sample(scene, u2x, u2y):
    from mitsuba_hip import _abi as A
    n = u2x.size
    u = np.ascontiguousarray(np.concatenate([u2x, u2y]).astype(np.float32))
    wo, pdf = np.zeros(3 * n, np.float32), np.zeros(n, np.float32)
    A.check(A.lib().mh_phase_sample(scene.handle(0), 0, n, _p(u), _p(wo), _p(pdf), 0))
    return wo.reshape(3, n), pdf


def gpu_eval(scene, wo):
    from mitsuba_hip import _abi as A
    wo = np.ascontiguousarray(wo, np.float32)
    n = wo.shape[1]
    val = np.zeros(n, np.float32)
    A.check(A.lib().mh_phase_eval(scene.handle(0), 0, n, _p(wo), _p(val), 0))
    return val


def gpu_sample_at(scene, u1, u2x, u2y, pos):
    from mitsuba_hip import _abi as A
    n = u1.size
    u = np.ascontiguousarray(np.concatenate([u1, u2x, u2y]).astype(np.float32))
    pos = np.ascontiguousarray(pos, np.float32)
    wo, pdf = np.zeros(3 * n, np.float32), np.zeros(n, np.float32)
    A.check(A.lib().mh_phase_sample_at(scene.handle(0), 0, n, _p(u), _p(pos), _p(wo), _p(pdf), 0))
    return wo.reshape(3, n), pdf


def gpu_eval_at(scene, wo, pos):
    from mitsuba_hip import _abi as A
    wo, pos = np.ascontiguousarray(wo, np.float32), np.ascontiguousarray(pos, np.float32)
    n = wo.shape[1]
    val = np.zeros(n, np.float32)
    A.check(A.lib().mh_phase_eval_at(scene.handle(0), 0, n, _p(wo), _p(pos), _p(val), 0))
    return val


# ---------------------------------------------------------------------------
# function level
# ---------------------------------------------------------------------------
def _inputs():
    """65,539 (u1, u2) pairs -- among them u1 in {0, w, the floats next to w,
    1 - 2^-24} for the constant weight w -- and points in and around every
    grid's box."""
    rng = np.random.default_rng(17)
    w = W_CONST
    u1 = np.concatenate([rng.random(65534, np.float32),
                         np.float32([0.0, w, np.nextafter(w, np.float32(0)), np.nextafter(w, np.float32(1)),
                                     1 - 2.0 ** -24])])
    assert u1.size == 65539
    pos = rng.uniform(-1.6, 1.6, (3, u1.size)).astype(np.float32)
    return u1, rng.random(u1.size, np.float32), rng.random(u1.size, np.float32), pos


def _directions(n=8192):
    rng = np.random.default_rng(5)
    z = np.concatenate([np.float32([-1, 1]), rng.uniform(-1, 1, n - 2).astype(np.float32)])
    phi = rng.uniform(0, 2 * np.pi, z.size)
    s = np.sqrt(np.maximum(1 - z.astype(np.float64) ** 2, 0))
    return np.stack([(s * np.cos(phi)).astype(np.float32), (s * np.sin(phi)).astype(np.float32), z])


def _weight(mi, key):
    return {"const": lambda: float(W_CONST), "g234": lambda: weight_grid(mi, (2, 3, 4)),
            "g567": lambda: weight_grid(mi, (5, 6, 7))}[key]()


@pytest.fixture(scope="module")
def pure():
    """The children's own device results on the shared inputs: per pair, per
    child (wo, pdf) of mh_phase_sample at the same u2 and mh_phase_eval at the
    same directions.  Computed once."""
    mi = _mi()
    _, u2x, u2y, _ = _inputs()
    wo = _directions()
    out = {}
    for key, pair in CHILD_PAIRS.items():
        scenes = [_phase_scene(mi, c) for c in pair]
        out[key] = {"sample": [gpu_sample(s, u2x, u2y) for s in scenes], "eval": [gpu_eval(s, wo) for s in scenes]}
    return out


@pytest.mark.parametrize("weight", ["const", "g234", "g567"])
@pytest.mark.parametrize("pair", list(CHILD_PAIRS))
def test_blend_sampling(pair, weight, pure):
    mi = _mi()
    scene = _phase_scene(mi, blend(*CHILD_PAIRS[pair], _weight(mi, weight)))
    u1, u2x, u2y, pos = _inputs()
    wo, pdf = gpu_sample_at(scene, u1, u2x, u2y, pos)
    if weight == "const":
        w = np.full(u1.size, W_CONST, np.float32).astype(np.float64)
        sure = np.ones(u1.size, bool)
    else:
        b = scene.phase_blends[0]
        w = weight_lookup(b.data, b.to_local, pos, np.float64)
        assert (w == 0).sum() > 1000 and (w == 1).sum() > 1000 and ((w > 0) & (w < 1)).sum() > 10000   # the clamp works
        sure = np.abs(u1.astype(np.float64) - w) > 1e-5   # the device's float32 weight decides the others
    u = u1.astype(np.float64)
    sel = [sure & (u > 0) & (u < w), sure & (u > w) & (u < 1)]   # blendphase.cpp:177: strict
    none = sure & ~sel[0] & ~sel[1]
    assert sel[0].sum() > 1000 and sel[1].sum() > 1000
    for i in (0, 1):
        cwo, cpdf = pure[pair]["sample"][i]
        np.testing.assert_array_equal(wo[:, sel[i]].view(np.uint32), cwo[:, sel[i]].view(np.uint32), err_msg=f"child {i} wo")
        np.testing.assert_array_equal(pdf[sel[i]].view(np.uint32), cpdf[sel[i]].view(np.uint32), err_msg=f"child {i} pdf")
    assert none[u1 == 0].all()
    np.testing.assert_array_equal(pdf[none], 0.0)
    np.testing.assert_array_equal(wo[:, none], 0.0)
    if weight == "const":   # u1 = 0, w, the floats next to w, 1 - 2^-24
        tail = slice(u1.size - 5, u1.size)
        assert none[tail].tolist() == [True, True, False, False, False]
        assert sel[0][tail].tolist() == [False, False, True, False, False]
        assert sel[1][tail].tolist() == [False, False, False, True, True]
    # the undecided lanes hold one child's result or none
    for j in np.nonzero(~sure)[0]:
        ok = pdf[j] == 0 or any(np.array_equal(wo[:, j], pure[pair]["sample"][i][0][:, j]) for i in (0, 1))
        assert ok, j


@pytest.mark.parametrize("weight", ["const", "g234", "g567"])
@pytest.mark.parametrize("pair", list(CHILD_PAIRS))
def test_blend_eval(pair, weight, pure):
    mi = _mi()
    scene = _phase_scene(mi, blend(*CHILD_PAIRS[pair], _weight(mi, weight)))
    wo = _directions()
    pos = _inputs()[3][:, :wo.shape[1]]
    val = gpu_eval_at(scene, wo, pos)
    e0, e1 = (pure[pair]["eval"][i] for i in (0, 1))
    if weight == "const":
        w = np.float64(W_CONST)
        ref = w * e0.astype(np.float64) + (1 - w) * e1.astype(np.float64)
        pos_ = ref > 0
        np.testing.assert_array_equal(val[~pos_], 0.0)
        err = (np.abs(val[pos_] - ref[pos_]) / ref[pos_]).max()
        print(f"{pair} constant weight: eval relative error {err:.3e} (bound {4 * ULP1:.3e})")
        assert err <= 4 * ULP1   # two products and a sum of positive terms, with or without FMA contraction
        return
    b = scene.phase_blends[0]
    w64, w32 = weight_lookup(b.data, b.to_local, pos, np.float64), weight_lookup(b.data, b.to_local, pos, np.float32)
    ref = w64 * e0.astype(np.float64) + (1 - w64) * e1.astype(np.float64)
    f32 = e0 * w32 + e1 * (np.float32(1) - w32)
    pos_ = ref > 0
    err_dev = (np.abs(val[pos_] - ref[pos_]) / ref[pos_]).max()
    err_f32 = (np.abs(f32[pos_] - ref[pos_]) / ref[pos_]).max()
    print(f"{pair} {weight}: eval relative error device {err_dev:.3e}, float32 restatement {err_f32:.3e}")
    assert err_dev <= 4 * err_f32 + 2.0 ** -22


def test_queries_at_cover_every_phase_function(pure):
    """mh_phase_sample_at / mh_phase_eval_at on a medium without a blend ignore
    sample1 and the point: the plain queries' results."""
    mi = _mi()
    u1, u2x, u2y, pos = _inputs()
    wo_e = _directions()
    for key, i in (("iso_hg", 0), ("iso_hg", 1), ("rayleigh_d", 0), ("rayleigh_d", 1)):
        scene = _phase_scene(mi, CHILD_PAIRS[key][i])
        wo, pdf = gpu_sample_at(scene, u1, u2x, u2y, pos)
        np.testing.assert_array_equal(wo, pure[key]["sample"][i][0])
        np.testing.assert_array_equal(pdf, pure[key]["sample"][i][1])
        np.testing.assert_array_equal(gpu_eval_at(scene, wo_e, pos[:, :wo_e.shape[1]]), pure[key]["eval"][i])


def test_plain_queries_refuse_a_blend():
    mi = _mi()
    from mitsuba_hip import _abi as A
    scene = _phase_scene(mi, blend(*CHILD_PAIRS["iso_hg"], 0.2))
    h, L = scene.handle(0), A.lib()
    buf = np.zeros(16, np.float32)
    assert L.mh_phase_sample(h, 0, 1, _p(buf), _p(buf[4:]), _p(buf[8:]), 0) == A.MH_ERR_INVALID_ARGUMENT
    assert L.mh_last_error().startswith(b"mh_phase_sample:") and b"mh_phase_sample_at" in L.mh_last_error()
    assert L.mh_phase_eval(h, 0, 1, _p(buf), _p(buf[4:]), 0) == A.MH_ERR_INVALID_ARGUMENT
    assert L.mh_last_error().startswith(b"mh_phase_eval:") and b"mh_phase_eval_at" in L.mh_last_error()


def test_render_without_the_blend_is_refused():
    """A blend medium without its blend, then without its tabulated child's
    table: every entry point that would launch returns
    MH_ERR_INVALID_ARGUMENT first."""
    mi = _mi()
    from mitsuba_hip import _abi as A
    scene = _phase_scene(mi, blend({"type": "rayleigh"}, tab("b"), 0.2))
    blends, scene.phase_blends = scene.phase_blends, {}     # handle() then attaches none
    h = scene.handle(0)
    L = A.lib()
    ic = scene.integrator().c()
    pv = mi.load_dict({"type": "prbvolpath", "max_depth": 4}).c()
    buf = np.zeros(8 * scene.width * scene.height, np.float32)

    def refused(what):
        calls = {
            "mh_render": lambda: L.mh_render(h, C.byref(ic), 0, 1, 0, 0, _p(buf), 0, None),
            "mh_render_samples": lambda: L.mh_render_samples(h, C.byref(ic), 0, 1, 0, 0, _p(buf), 0),
            "mh_phase_eval_at": lambda: L.mh_phase_eval_at(h, 0, 1, _p(buf), _p(buf[4:]), _p(buf[8:]), 0),
            "mh_phase_sample_at": lambda: L.mh_phase_sample_at(h, 0, 1, _p(buf), _p(buf[4:]), _p(buf[8:]), _p(buf[12:]), 0),
            "mh_render_backward": lambda: L.mh_render_backward(h, C.byref(pv), 0, 1, 0, 0, _p(buf), None, 0, None, None, 0, None),
            "mh_render_forward": lambda: L.mh_render_forward(h, C.byref(pv), 0, 1, 0, 0, 0, None, None, _p(buf), 0, None),
        }
        for name, call in calls.items():
            assert call() == A.MH_ERR_INVALID_ARGUMENT, name
            assert name.encode() in L.mh_last_error() and what in L.mh_last_error(), (name, L.mh_last_error())

    refused(b"no blend")
    c, v = blends[0].children[1]["table"]
    cp, vp = c.ctypes.data_as(A.PF), v.ctypes.data_as(A.PF)
    assert L.mh_scene_set_phase_blend_table(h, 0, 1, c.size, cp, vp) == A.MH_ERR_INVALID_ARGUMENT   # no blend yet
    rec = blends[0].record()
    assert L.mh_scene_set_phase_blend(h, 0, C.byref(rec)) == A.MH_OK
    refused(b"no table")
    assert L.mh_scene_set_phase_blend_table(h, 0, 0, c.size, cp, vp) == A.MH_ERR_INVALID_ARGUMENT   # child 0 is rayleigh
    assert L.mh_scene_set_phase_blend_table(h, 0, 2, c.size, cp, vp) == A.MH_ERR_INVALID_ARGUMENT
    bad = v.copy()
    bad[1] = -1
    assert L.mh_scene_set_phase_blend_table(h, 0, 1, c.size, cp, bad.ctypes.data_as(A.PF)) == A.MH_ERR_INVALID_ARGUMENT
    assert L.mh_last_error().startswith(b"mh_scene_set_phase_blend_table") and b"non-negative" in L.mh_last_error()
    rec.phase[0] = A.PHASE_BLEND
    assert L.mh_scene_set_phase_blend(h, 0, C.byref(rec)) == A.MH_ERR_INVALID_ARGUMENT
    assert b"nested blend" in L.mh_last_error()
    assert L.mh_scene_update_phase_blend_weight(h, 0, cp, 2) == A.MH_ERR_INVALID_ARGUMENT   # a constant weight: n = 1
    assert L.mh_scene_set_phase_blend_table(h, 0, 1, c.size, cp, vp) == A.MH_OK
    assert L.mh_render(h, C.byref(ic), 0, 1, 0, 0, _p(buf), 0, None) == A.MH_OK


# ---------------------------------------------------------------------------
# integrator level
# ---------------------------------------------------------------------------
HET = {"grid_res": 16, "scale": 4.0}
HOM = {"medium_type": "homogeneous", "sigma_t": 0.8, "scale": 1.0}
SHAPES = {"heterogeneous": HET, "homogeneous": HOM}
A_PHASE, B_PHASE = tab("d"), {"type": "rayleigh"}


def _real_blend(mi):
    """Air and aerosol: rayleigh plus the 181-node table (d), the aerosol fraction falling with height."""
    return blend({"type": "rayleigh"}, tab("d"), falling_grid(mi))


def _scene(mi, phase, integrator="volpath", w=24, h=20, spp=8, floor=True, max_depth=6, rr_depth=5, **kw):
    """volume_cube (+ the diffuse floor of the parity tests' scenes) with the medium's phase replaced."""
    kw = dict(kw)
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
    return out.reshape(5, n)


def _grid_of(mi, lo, hi):
    g = weight_grid(mi, (5, 6, 7))
    g["data"] = np.random.default_rng(9).uniform(lo, hi, g["data"].shape).astype(np.float32)
    return g


@pytest.mark.parametrize("integrator", ["volpath", "prbvolpath"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_degenerate_weights_render_the_pure_child(shape, integrator):
    """weight_0 = 1 is child A alone and weight_0 = 0 child B alone, per sample:
    only a path that drew sample1 == 0 (2^-24 per scatter) may differ."""
    mi = _mi()
    from mitsuba_hip import _abi as A
    forms = {1: [1.0, const_grid(mi, (5, 6, 7), 1.0), _grid_of(mi, 1.0, 1.7)],
             0: [0.0, const_grid(mi, (5, 6, 7), 0.0), _grid_of(mi, -0.7, 0.0)]}
    for flags in (0, A.FLAG_WAVEFRONT):
        for w, child in ((1, A_PHASE), (0, B_PHASE)):
            ref = _gpu_samples(_scene(mi, child, integrator, **SHAPES[shape]), 3, 8, flags)
            assert np.isfinite(ref).all() and np.abs(ref[:3]).max() > 0
            for k, form in enumerate(forms[w]):
                got = _gpu_samples(_scene(mi, blend(A_PHASE, B_PHASE, form), integrator, **SHAPES[shape]), 3, 8, flags)
                differ = (got != ref).any(axis=0)
                print(f"{integrator} {shape} flags {flags} weight {w} form {k}: {differ.sum()} of {differ.size} samples differ")
                assert differ.mean() <= 1e-3, (flags, w, k)


def _grad_keys(shape):
    sigma_t = "medium1.sigma_t.data" if shape == "heterogeneous" else "medium1.sigma_t.value"
    return [sigma_t, "medium1.albedo.value", "floor.bsdf.reflectance.value"]


@pytest.mark.parametrize("form", ["constant", "clamped-grid"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_degenerate_weight_gradients_are_the_pure_childs(shape, form):
    """deterministic prbvolpath gradients of the weight_0 = 1 scene: pure A's, bit for bit."""
    mi = _mi()
    import torch
    keys = _grad_keys(shape)
    gi = torch.from_numpy(np.random.default_rng(4).standard_normal((20, 24, 3)).astype(np.float32)).cuda()
    out = []
    one = 1.0 if form == "constant" else _grid_of(mi, 1.0, 1.7)
    for phase in (A_PHASE, blend(A_PHASE, B_PHASE, one)):
        scene = _scene(mi, phase, "prbvolpath", **SHAPES[shape])
        g = mi.render_backward(scene, mi.traverse(scene), gi, keys, scene.integrator(), seed=7, spp=8, deterministic=True)
        out.append([a.cpu().numpy() for a in g])
    for k, a, b in zip(keys, *out):
        assert np.abs(a).max() > 0, k
        np.testing.assert_array_equal(a, b, err_msg=k)


@pytest.mark.parametrize("integrator", ["volpath", "prbvolpath"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_engines_agree(shape, integrator):
    """The per-lane megakernel and the wavefront engines (MH_FLAG_WAVEFRONT)
    call the same device functions with the same weight: bit-identical per
    sample on a real blend."""
    mi = _mi()
    from mitsuba_hip import _abi as A
    scene = _scene(mi, _real_blend(mi), integrator, **SHAPES[shape])
    mega = _gpu_samples(scene, 3, 8, 0)
    wave = _gpu_samples(scene, 3, 8, A.FLAG_WAVEFRONT)
    assert np.isfinite(mega).all() and np.abs(mega[:3]).max() > 0
    np.testing.assert_array_equal(mega, wave)
    # and the blend is not one of its children
    for child in ({"type": "rayleigh"}, tab("d")):
        assert not np.array_equal(mega, _gpu_samples(_scene(mi, child, integrator, **SHAPES[shape]), 3, 8, 0))


@pytest.mark.parametrize("rounds", ["rounds", "finish1"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_hbm_wavefront_engine_agrees(shape, rounds, monkeypatch):
    """volpath's HBM wavefront engine (MH_VOL_MODE=rounds: k_vw_main / k_vw_walk,
    which carry the weight of a suspended scatter through the path record;
    MH_VW_ROUNDS=1: k_vw_finish resumes the suspended scatters) against the
    megakernel: bit-identical on the real blend, and the pure child's samples
    for weight 1 and 0."""
    mi = _mi()
    from mitsuba_hip import _abi as A
    cases = {"real": _real_blend(mi), "one": blend(A_PHASE, B_PHASE, _grid_of(mi, 1.0, 1.7)),
             "zero": blend(A_PHASE, B_PHASE, 0.0)}
    mega = {k: _gpu_samples(_scene(mi, ph, "volpath", **SHAPES[shape]), 3, 8, 0) for k, ph in cases.items()}
    child = {"one": _gpu_samples(_scene(mi, A_PHASE, "volpath", **SHAPES[shape]), 3, 8, 0),
             "zero": _gpu_samples(_scene(mi, B_PHASE, "volpath", **SHAPES[shape]), 3, 8, 0)}
    monkeypatch.setenv("MH_VOL_MODE", "rounds")
    if rounds == "finish1":
        monkeypatch.setenv("MH_VW_ROUNDS", "1")
    for k, ph in cases.items():
        wave = _gpu_samples(_scene(mi, ph, "volpath", **SHAPES[shape]), 3, 8, A.FLAG_WAVEFRONT)
        assert np.isfinite(wave).all() and np.abs(wave[:3]).max() > 0
        np.testing.assert_array_equal(wave, mega[k], err_msg=k)
        if k in child:
            differ = (wave != child[k]).any(axis=0)
            print(f"{shape} {rounds} weight {k}: {differ.sum()} of {differ.size} samples differ from the pure child")
            assert differ.mean() <= 1e-3, k
    assert not np.array_equal(mega["real"], child["one"]) and not np.array_equal(mega["real"], child["zero"])


def test_far_weight_lookups_clamp():
    """A weight grid is read wherever the medium scatters: points up to 1e30
    from its box (texel coordinates far beyond the int32 range) read its edge
    texels, as the float64 restatement does."""
    mi = _mi()
    scene = _phase_scene(mi, blend(*CHILD_PAIRS["iso_hg"], weight_grid(mi, (2, 3, 4))))
    rng = np.random.default_rng(23)
    pos = (rng.choice([-1.0, 1.0], (3, 4096)) * 10.0 ** rng.uniform(1, 30, (3, 4096))).astype(np.float32)
    wo = _directions(4096)
    val = gpu_eval_at(scene, wo, pos)
    b = scene.phase_blends[0]
    w = weight_lookup(b.data, b.to_local, pos, np.float64)
    iso, h = np.full(4096, 1 / (4 * np.pi)), hg(0.6, wo[2].astype(np.float64))
    ref = w * iso + (1 - w) * h
    assert np.isfinite(val).all()
    np.testing.assert_allclose(val, ref, rtol=2e-6)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_backward_paths_agree(monkeypatch, shape):
    """sigma_t, albedo and floor reflectance gradients through the real blend:
    the default scheduler, the per-sample kernel (MH_PVP_SCHED=0), the
    NEE-replaying kernel (MH_PVP_NEE_LOG=0) and the scheduler with a path log of
    two entries (MH_PVP_MAIN_CAP=2: nearly every path overflows it and is
    replayed by k_pvb_replay_paths), at
    test_gpu_phase_functions.test_backward_paths_agree's tolerances."""
    mi = _mi()
    import torch
    keys = _grad_keys(shape)
    gi = np.random.default_rng(4).standard_normal((20, 24, 3)).astype(np.float32)
    out = {}
    for mode, env, val in (("sched", None, None), ("sched_off", "MH_PVP_SCHED", "0"), ("replay", "MH_PVP_NEE_LOG", "0"),
                           ("path_replay", "MH_PVP_MAIN_CAP", "2")):
        if env:
            monkeypatch.setenv(env, val)
        scene = _scene(mi, _real_blend(mi), "prbvolpath", **SHAPES[shape])
        params = mi.traverse(scene)
        g = mi.render_backward(scene, params, torch.from_numpy(gi).cuda(), keys, scene.integrator(), seed=7, spp=8)
        out[mode] = [a.cpu().numpy() for a in g]
        if env:
            monkeypatch.delenv(env)
    for mode in ("sched_off", "replay", "path_replay"):
        for k, a, b in zip(keys, out[mode], out["sched"]):
            assert a.shape == b.shape and np.abs(b).max() > 0, (mode, k)
            np.testing.assert_allclose(a, b, rtol=2e-3, atol=1e-7 + 2e-4 * np.abs(b).max(), err_msg=f"{mode} {k}")


@pytest.mark.parametrize("integrator", ["volpath", "prbvolpath"])
def test_identical_children_render_like_the_child(integrator):
    """blend(hg 0.6, hg 0.6, 0.2) against hg 0.6 at the same seed, sky and sun:
    0.2 is not on the sampler's 2^-23 / 2^-24 output grid, so sample1 == w cannot
    occur, the paths are identical and only the NEE evaluation rounds
    differently."""
    mi = _mi()
    hg6 = {"type": "hg", "g": 0.6}
    films = []
    for phase in (hg6, blend(hg6, hg6, 0.2)):
        scene = _scene(mi, phase, integrator, **HET)
        films.append(mi.render_film(scene, seed=5, spp=8, deterministic=True).cpu().numpy())
    assert np.abs(films[0]).max() > 0
    np.testing.assert_allclose(films[1], films[0], rtol=1e-5, atol=0)


MIX_KW = dict(medium_type="homogeneous", sigma_t=1.0, scale=2.0, albedo=0.9, max_depth=8)


def _mix_mean(mi, phase, seed):
    d = mi.volume_cube(16, 16, 256, **MIX_KW)
    del d["sky"]   # the directional sun only: no MIS on the phase pdf
    d["medium1"]["phase"] = phase
    scene = mi.load_dict(d)
    img = mi.develop(scene, mi.render_film(scene, seed=seed, spp=256)).cpu().numpy()
    return float(img.astype(np.float64).mean())


def test_blend_of_two_tables_is_the_mixed_table():
    """On the nodes of table (d), T0 = hg(0.85) and T1 = hg(-0.5), each divided
    by its own table integral: the single table 0.25 T0 + 0.75 T1 is exactly
    blend(T0, T1, weight_0 = 0.25) (shared nodes, piecewise linear).  The
    single-table scene over seeds 0-7 gives mu and sigma; the blend's image mean
    at seed 100 must lie within 4 sigma sqrt(1 + 1/8), and the single table of
    the swapped mixture (0.75 / 0.25) must miss mu by more than 8 sigma, so
    swapped sampling proportions cannot pass."""
    mi = _mi()
    c = TABLES["d"][0]
    c64 = c.astype(np.float64)
    norm = lambda v: v / (0.5 * (c64[1:] - c64[:-1]) * (v[1:] + v[:-1])).sum()
    t0, t1 = norm(hg(0.85, c64)), norm(hg(-0.5, c64))
    table = lambda v: {"type": "tabphase", "cost": c, "values": v}
    means = [_mix_mean(mi, table(0.25 * t0 + 0.75 * t1), s) for s in range(8)]
    mu, sigma = float(np.mean(means)), float(np.std(means, ddof=1))
    got = _mix_mean(mi, blend(table(t0), table(t1), 0.25), 100)
    swapped = _mix_mean(mi, table(0.75 * t0 + 0.25 * t1), 100)
    print(f"single table: mu {mu:.6f} sigma {sigma:.6f}; blend {got:.6f}; swapped single table {swapped:.6f}")
    assert abs(swapped - mu) > 8 * sigma
    assert abs(got - mu) <= 4 * sigma * np.sqrt(1 + 1 / 8)


def test_white_furnace():
    """test_gpu_phase_functions.test_white_furnace's scene and bound with the
    real blend and sample_emitters = false: without NEE emitter hits count in
    full, so the child-pdf carried into MIS cannot bias it."""
    mi = _mi()
    d = mi.volume_cube(32, 32, 256, grid=mi.fbm_grid(32), albedo=1.0, sky=1.0, sun=None, scale=5.0, max_depth=-1)
    d["medium1"]["phase"] = _real_blend(mi)
    d["medium1"]["sample_emitters"] = False
    scene = mi.load_dict(d)
    img = mi.develop(scene, mi.render_film(scene, seed=0, spp=256)).cpu().numpy()
    print(f"white furnace through the blend: mean {img.mean():.6f}")
    assert abs(img.mean() - 1.0) < 0.01


def test_albedo_gradient_vs_finite_differences():
    """test_gpu_phase_functions.test_albedo_gradient_vs_finite_differences on the blend scene."""
    mi = _mi()
    import torch
    scene = _scene(mi, _real_blend(mi), "prbvolpath", max_depth=3, rr_depth=8, **HET)
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
    mi = _mi()
    from mitsuba_hip import _abi as A
    scene = _scene(mi, _real_blend(mi), "prbvolpath", **HET)
    params = mi.traverse(scene)
    for k in ("medium1.sigma_t.data", "medium1.albedo.value"):
        params[k].requires_grad_()
    img = mi.render(scene, params, spp=8, seed=3)
    img.mean().backward()
    for k in ("medium1.sigma_t.data", "medium1.albedo.value"):
        g = params[k].grad
        assert g is not None and g.shape == params[k].shape and bool(g.abs().max() > 0) and bool(g.isfinite().all())
    for k in ("medium1.phase_function.weight_0.data", "medium1.phase_function.phase_1.values"):
        with pytest.raises(A.MitsubaHipError, match="not differentiable"):
            params.param_id(k)


def _falling_scaled(mi, s):
    g = falling_grid(mi)
    g["data"] = (g["data"] * np.float32(s)).astype(np.float32)
    return g


@pytest.mark.parametrize("what", ["data", "value", "values", "g"])
def test_update_equals_a_fresh_scene(what):
    mi = _mi()
    ray, hg3 = {"type": "rayleigh"}, {"type": "hg", "g": 0.3}
    c = TABLES["d"][0]
    new_values = hg(0.3, c.astype(np.float64)).astype(np.float32)
    old, key, value, new = {
        "data": (blend(ray, tab("d"), falling_grid(mi)), "weight_0.data", _falling_scaled(mi, 0.5)["data"],
                 blend(ray, tab("d"), _falling_scaled(mi, 0.5))),
        "value": (blend(ray, tab("d"), 0.3), "weight_0.value", [0.8], blend(ray, tab("d"), 0.8)),
        "values": (blend(ray, tab("d"), 0.3), "phase_1.values", new_values,
                   blend(ray, {"type": "tabphase", "cost": c, "values": new_values}, 0.3)),
        "g": (blend(hg3, tab("d"), 0.6), "phase_0.g", [-0.5], blend({"type": "hg", "g": -0.5}, tab("d"), 0.6)),
    }[what]
    scene = _scene(mi, old, **HET)
    before = mi.render_film(scene, seed=2, spp=8, deterministic=True).cpu().numpy()
    params = mi.traverse(scene)
    params["medium1.phase_function." + key] = value
    params.update()
    after = mi.render_film(scene, seed=2, spp=8, deterministic=True).cpu().numpy()
    ref = mi.render_film(_scene(mi, new, **HET), seed=2, spp=8, deterministic=True).cpu().numpy()
    assert not np.array_equal(before, after)
    np.testing.assert_array_equal(after, ref)
