"""The fused bounce kernels' per-primitive shade records (ShadeRec).

The fused kernels (k_wf_bounce, k_wf_bounce_prb, k_wf_bounce_fwd) read the
frame and the emitter / bsdf / texture ids of a closest hit from a record
built once at scene creation; the unfused wavefront (MH_WF_FUSED=0) and the
oracle still compute them per hit.  Every scene below takes one path through
compute_si_rec, and on each of them:

  path      fused per-sample radiance == the oracle's (bit-exact for >= 99.9 %
            of the samples, the rest BVH-vs-brute-force ties: the criterion of
            test_gpu_parity.py) and == the unfused wavefront's, every sample
  prb       render_backward of an rgb reflectance: fused vs unfused rtol 1e-4,
            atol 1e-8; vs the oracle rtol 1e-3, atol 1e-7 (the tolerances of
            test_gpu_parity.py::test_prb_backward_wavefront_chunked)
  forward   render_forward (k_wf_bounce_fwd) vs the oracle, test_gpu_forward.py's
            criterion
"""
import ctypes as C

import numpy as np
import pytest

import oracle_py as O

pytestmark = pytest.mark.gpu

W, H, SPP = 24, 24, 8


def _mi():
    import mitsuba_hip as mi
    if not mi.is_available():
        pytest.fail("no HIP device / native library: the GPU tests need an MI355X")
    mi.set_variant("hip_ad_rgb")
    return mi


def _base(mi):
    d = mi.cornell_box()
    d["sensor"]["film"]["width"], d["sensor"]["film"]["height"] = W, H
    d["sensor"]["sampler"]["sample_count"] = SPP
    return d


def _cbox(mi):
    """rectangles, the two cubes, and waves that mix both"""
    return _base(mi), {}


def _smooth(mi):
    """a 32-triangle mesh with vertex normals (no constant frame: the frame is built per hit from the
    record's n and dp_du) beside the room's rectangles"""
    from mitsuba_hip import meshio
    n = 5
    x, y = np.meshgrid(np.linspace(-0.8, 0.8, n), np.linspace(-0.8, 0.8, n))
    z = 0.15 * np.sin(3 * x) * np.cos(2 * y)
    V = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)
    UV = np.stack([(x + 0.8) / 1.6, (y + 0.8) / 1.6], -1).reshape(-1, 2).astype(np.float32)
    i = np.arange(n - 1)
    a = (i[:, None] * n + i[None, :]).reshape(-1)
    F = np.concatenate([np.stack([a, a + 1, a + n + 1], 1), np.stack([a, a + n + 1, a + n], 1)]).astype(np.uint32)
    T = mi.Transform4f
    to_world = T.translate([0, 0.1, 0]) @ T.rotate([1, 0, 0], -70)
    Vw = (V.astype(np.float64) @ to_world.matrix[:3, :3].T + to_world.matrix[:3, 3]).astype(np.float32)
    N = meshio.recompute_vertex_normals(Vw, F)
    tex = np.random.default_rng(5).uniform(0.2, 0.9, (8, 8, 3)).astype(np.float32)
    d = _base(mi)
    d.pop("small-box")
    d.pop("large-box")
    d["bumpy"] = {"type": "mesh", "vertex_positions": Vw, "faces": F, "vertex_normals": N, "vertex_texcoords": UV,
                  "bsdf": {"type": "diffuse", "reflectance": {"type": "bitmap", "data": tex, "raw": True,
                                                              "filter_type": "bilinear"}}}
    return d, {}


def _flat_uv(mi):
    """a flat mesh (no vertex normals) with texture coordinates and a bitmap reflectance: dp_du from the
    uvs on three triangles, from coordinate_system(n) on the fourth, whose uv determinant is exactly 0"""
    P = np.array([[-0.7, -0.6, 0.3], [0.0, -0.6, 0.5], [-0.7, 0.1, 0.1], [0.0, 0.1, 0.3],
                  [0.7, -0.6, 0.3], [0.7, 0.1, 0.1]], np.float32)
    tri = [(0, 1, 2), (1, 3, 2), (1, 4, 3), (4, 5, 3)]
    V = np.concatenate([P[list(t)] for t in tri]).astype(np.float32)   # unshared vertices: uvs per triangle
    F = np.arange(12, dtype=np.uint32).reshape(4, 3)
    UV = np.array([[0.0, 0.0], [0.5, 0.0], [0.0, 1.0],
                   [0.5, 0.0], [0.5, 1.0], [0.0, 1.0],
                   [0.5, 0.0], [1.0, 0.0], [0.5, 1.0],
                   [0.0, 0.0], [0.25, 0.25], [0.5, 0.5]], np.float32)   # the last: collinear uvs, det == 0
    d0, d1 = UV[10] - UV[9], UV[11] - UV[9]
    assert np.float32(d0[0] * d1[1]) - np.float32(d0[1] * d1[0]) == 0
    tex = np.random.default_rng(8).uniform(0.2, 0.9, (6, 5, 3)).astype(np.float32)
    d = _base(mi)
    d.pop("small-box")
    d.pop("large-box")
    d["plate"] = {"type": "mesh", "vertex_positions": V, "faces": F, "vertex_texcoords": UV,
                  "bsdf": {"type": "diffuse", "reflectance": {"type": "bitmap", "data": tex, "raw": True,
                                                              "filter_type": "bilinear"}}}
    return d, {}


def _null_bsdf(mi):
    """a null-BSDF rectangle in the room: a record whose bsdf is not diffuse"""
    T = mi.Transform4f
    d = _base(mi)
    d["ghost"] = {"type": "rectangle", "to_world": T.translate([0.1, -0.2, 0.6]).rotate([0, 1, 0], 20).scale(0.35),
                  "bsdf": {"type": "null"}}
    return d, {}


def _open_hidden(mi):
    """hide_emitters, an environment and no back wall: camera rays escape (key MH_INVALID: no record)"""
    d = _base(mi)
    d.pop("back")
    d["sky"] = {"type": "constant", "radiance": {"type": "rgb", "value": [0.3, 0.4, 0.5]}}
    return d, {"hide_emitters": True}


def _two_lights(mi):
    """a second area emitter: the record's emitter id is not always 0"""
    T = mi.Transform4f
    d = _base(mi)
    d["light2"] = {"type": "rectangle",
                   "to_world": T.translate([0.55, -0.99, 0.55]).rotate([1, 0, 0], -90).scale(0.12),
                   "bsdf": {"type": "ref", "id": "white"},
                   "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [3.0, 5.0, 8.0]}}}
    return d, {}


SCENES = {"cbox": _cbox, "smooth-normals": _smooth, "flat-uv-det0": _flat_uv, "null-bsdf": _null_bsdf,
          "hide-emitters-open": _open_hidden, "two-lights": _two_lights}
KEY = "red.reflectance.value"


def _load(mi, name):
    d, opts = SCENES[name](mi)
    return mi.load_dict(d), opts


def _gpu_samples(mi, scene, integ, seed):
    from mitsuba_hip import _abi as A
    n = scene.width * scene.height * SPP
    out = np.zeros(5 * n, np.float32)
    ic = integ.c()
    A.check(A.lib().mh_render_samples(scene.handle(0), C.byref(ic), seed, SPP, 0, 0,
                                      out.ctypes.data_as(C.c_void_p), A.FLAG_WAVEFRONT))
    return out[:3 * n].reshape(3, n).T.copy(), out[3 * n:].reshape(2, n).T.copy()


@pytest.mark.parametrize("name", list(SCENES))
def test_path_samples_fused_vs_oracle_and_unfused(name, monkeypatch):
    mi = _mi()
    scene, opts = _load(mi, name)
    assert scene.desc.n_emitters >= (2 if name == "two-lights" else 1)
    integ = mi.load_dict({"type": "path", "max_depth": 8, **opts})
    L, pos = _gpu_samples(mi, scene, integ, 3)
    rL, rpos, _ = O.sample_range(scene, integ, 3, SPP, 0, L.shape[0])
    np.testing.assert_array_equal(pos, rpos)
    exact = np.all(L == rL, axis=1)
    print(f"{name}: bit-exact fraction vs the oracle {exact.mean():.6f}")
    assert exact.mean() >= 0.999, f"bit-exact fraction {exact.mean()}"
    assert rL.mean() > 0
    if name == "hide-emitters-open":
        assert (rL.sum(1) == 0).mean() > 0.05
    monkeypatch.setenv("MH_WF_FUSED", "0")   # trace / shade / shadow kernels: compute_si per hit
    U, upos = _gpu_samples(mi, scene, integ, 3)
    np.testing.assert_array_equal(upos, pos)
    np.testing.assert_array_equal(L, U)


@pytest.mark.parametrize("name", list(SCENES))
def test_prb_gradient_fused_vs_unfused_and_oracle(name, monkeypatch):
    mi = _mi()
    import torch
    scene, opts = _load(mi, name)
    integ = mi.load_dict({"type": "prb", "max_depth": 8, **opts})
    params = mi.traverse(scene)
    gi = np.random.default_rng(4).random((H, W, 3)).astype(np.float32) / (H * W * 3)
    g = torch.from_numpy(gi).cuda()
    a = mi.render_backward(scene, params, g, [KEY], integ, seed=9, spp=SPP)[0].cpu().numpy()
    ref = O.render_backward(scene, integ, 9, SPP, gi, [params.texture_of(KEY)], [(3,)])[0]
    monkeypatch.setenv("MH_WF_FUSED", "0")
    b = mi.render_backward(scene, params, g, [KEY], integ, seed=9, spp=SPP)[0].cpu().numpy()
    print(f"{name}: fused {a} unfused {b} oracle {ref}")
    assert np.abs(ref).max() > 0
    np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-8)
    np.testing.assert_allclose(a, ref, rtol=1e-3, atol=1e-7)


@pytest.mark.parametrize("name", list(SCENES))
def test_render_forward_fused_vs_oracle(name):
    mi = _mi()
    import torch
    from mitsuba_hip import _abi as A
    scene, opts = _load(mi, name)
    integ = mi.load_dict({"type": "prb", "max_depth": 8, **opts})
    params = mi.traverse(scene)
    tan = np.array([1.0, -0.5, 0.25], np.float32)
    st = A.Stats()
    img = mi.render_forward(scene, params, {KEY: torch.as_tensor(tan).cuda()}, integ, seed=11, spp=SPP,
                            stats=st).cpu().numpy()
    assert st.mode == 2   # the fused forward-mode wavefront
    film = O.render_forward(scene, integ, 11, SPP, [params.param_id(KEY)], [tan])
    ref = O.develop(film, scene.desc.sensor.pixel_format)
    assert img.shape == ref.shape and np.abs(ref).max() > 0
    d = np.abs(img - ref)
    ok = d <= 1e-4 + 2e-3 * np.abs(ref)
    print(f"{name}: {(~ok).sum()} of {ok.size} channels off, max {d.max():.3e}")
    assert ok.mean() >= 0.995, f"{(~ok).sum()} of {ok.size} channels off, max {d.max():.3e}"
    assert d.mean() / max(np.abs(ref).mean(), 1e-12) < 1e-3


def test_records_hold_no_parameter_value():
    """After params.update() of an rgb reflectance and of a bitmap texture the fused render equals a
    freshly created scene with the new values, bit for bit."""
    mi = _mi()
    rng = np.random.default_rng(12)
    new_red = np.array([0.2, 0.6, 0.3], np.float32)
    new_tex = rng.uniform(0.1, 0.9, (4, 4, 3)).astype(np.float32)

    def make(red, tex):
        d = mi.cornell_box_bitmap(tex_res=4, width=W, height=H, spp=SPP)
        if red is not None:
            d["red"]["reflectance"]["value"] = [float(x) for x in red]
        if tex is not None:
            d["white"]["reflectance"]["data"] = tex.copy()
        return mi.load_dict(d)

    integ = mi.load_dict({"type": "path", "max_depth": 8})
    scene = make(None, None)
    before, _ = _gpu_samples(mi, scene, integ, 7)   # creates the device scene and its records
    params = mi.traverse(scene)
    params[KEY] = new_red
    params["white.reflectance.data"] = new_tex
    params.update()
    after, _ = _gpu_samples(mi, scene, integ, 7)
    fresh, _ = _gpu_samples(mi, make(new_red, new_tex), integ, 7)
    assert not np.array_equal(before, after)
    np.testing.assert_array_equal(after, fresh)
