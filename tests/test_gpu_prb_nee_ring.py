"""The NEE ring of the non-generating rgb PRB bounce kernel
(k_wf_bounce_prb<1, false, false, false>, mh_wavefront.hip): shadow rays of
several iterations of a wave are collected in an LDS ring and traced in full
packets; their gradient terms are added to the block's sum whenever they are
traced.  The gradient therefore changes in float summation order only, and
the ray counts not at all.

`prb` render_backward with respect to white.reflectance.value on the cornell
box against the CPU oracle (rtol 1e-3) and against the unfused pipeline
(MH_WF_FUSED=0: trace / shade / shadow kernels, no ring) at the rtol 1e-4 the
two-stream test uses for reordered sums, with equal closest and shadow ray
counts.

Launch geometry decides what the ring does.  A call launches wf_blocks
workgroups whatever the path count (256 CUs x 30 = 7,680 alone), dealt over
64 queue segments: 480 waves and 30,720 paths per iteration and segment.  At
the small films of test_ring_gradient_matches_oracle_and_unfused every wave
runs at most one iteration, which is its last: nothing is pushed, and those
cases check the trace path of the ring instance and its shadow-ray count.
test_ring_push_fill_drain sets MH_WF_BPC=1 (256 workgroups: 16 waves, 1,024
paths per iteration and segment), so that waves run several iterations and
the ring is pushed to, popped from and drained (see its docstring).  The
four-slot instance (two keys) and the deterministic instance have no ring.
"""
import numpy as np
import pytest

import oracle_py as O

pytestmark = pytest.mark.gpu

KEY = "white.reflectance.value"


def _mi():
    import mitsuba_hip as mi
    if not mi.is_available():
        pytest.fail("no HIP device / native library: the GPU tests need an MI355X")
    mi.set_variant("hip_ad_rgb")
    return mi


def _cbox(mi, w, h, spp):
    d = mi.cornell_box()
    d["sensor"]["film"]["width"], d["sensor"]["film"]["height"] = w, h
    d["sensor"]["sampler"]["sample_count"] = spp
    return mi.load_dict(d)


def _backward(mi, scene, keys, max_depth, spp, seed, **kw):
    import torch
    from mitsuba_hip import _abi as A
    integ = mi.load_dict({"type": "prb", "max_depth": max_depth})
    H, W = scene.height, scene.width
    gi = torch.full((H, W, 3), 1.0 / (H * W * 3), device="cuda")
    st = A.Stats()
    g = mi.render_backward(scene, mi.traverse(scene), gi, keys, integ, seed=seed, spp=spp, stats=st, **kw)
    return [x.cpu().numpy() for x in g], (st.rays_closest, st.rays_shadow)


def _oracle(mi, scene, keys, max_depth, spp, seed):
    integ = mi.load_dict({"type": "prb", "max_depth": max_depth})
    H, W = scene.height, scene.width
    gi = np.full((H, W, 3), 1.0 / (H * W * 3), np.float32)
    params = mi.traverse(scene)
    return O.render_backward(scene, integ, seed, spp, gi, [params.texture_of(k) for k in keys], [(3,)] * len(keys))


@pytest.mark.parametrize("w,h,spp,max_depth", [(24, 24, 8, 8), (8, 8, 1, 8), (24, 24, 8, 1), (24, 24, 8, 2)])
def test_ring_gradient_matches_oracle_and_unfused(w, h, spp, max_depth, monkeypatch):
    mi = _mi()
    scene = _cbox(mi, w, h, spp)
    (g,), rays = _backward(mi, scene, [KEY], max_depth, spp, 11)
    (ref,) = _oracle(mi, scene, [KEY], max_depth, spp, 11)
    monkeypatch.setenv("MH_WF_FUSED", "0")
    (u,), rays_u = _backward(mi, scene, [KEY], max_depth, spp, 11)
    print(f"{w}x{h}@{spp} depth {max_depth}: g {g} oracle {ref} unfused {u} rays {rays} / {rays_u}")
    assert rays == rays_u
    assert (rays[1] > 0) == (max_depth >= 2)  # NEE needs depth + 1 < max_depth: none at 1, one bounce at 2
    assert (np.abs(ref).max() > 0) == (max_depth >= 2)
    np.testing.assert_allclose(g, ref, rtol=1e-3, atol=1e-7)
    np.testing.assert_allclose(g, u, rtol=1e-4)


@pytest.mark.parametrize("w,h,spp", [(48, 48, 64), (32, 32, 128), (64, 64, 64)])
def test_ring_push_fill_drain(w, h, spp, monkeypatch):
    """Several iterations per wave (MH_WF_BPC=1: 1,024 paths per iteration and
    queue segment).  With k new shadow rays per iteration and r items in the
    ring, an iteration that is not the wave's last pushes while r + k < 64 and
    otherwise pops min(r, 64 - k) items into its idle lanes; the last
    iteration always traces, and what it has no room for is drained after
    the loop.  On the cornell box k is about 45 of 64 at the first bounces
    and falls with the depth.
      48 x 48 @ 64   2,304 paths per segment, 3 iterations at the first
                     bounces: push (r = k), fill (r + k >= 64 for k >= 32:
                     64 - k lanes pop, r = 2k - 64), last iteration pops
                     64 - k and leaves 3k - 128 > 0 items for the drain
                     (k >= 43); later bounces with fewer paths run 2 and 1
      32 x 32 @ 128  2,048 paths per segment, 2 iterations: push, then the
                     last iteration pops 64 - k and the drain takes 2k - 64
      64 x 64 @ 64   4,096 paths per segment, 4 iterations: two fills
    A ring that lost, repeated or mixed up items would move the gradient by
    far more than the tolerance: about a third of all shadow rays pass
    through it."""
    mi = _mi()
    monkeypatch.setenv("MH_WF_BPC", "1")
    scene = _cbox(mi, w, h, spp)
    (g,), rays = _backward(mi, scene, [KEY], 8, spp, 11)
    (ref,) = _oracle(mi, scene, [KEY], 8, spp, 11)
    monkeypatch.setenv("MH_WF_FUSED", "0")
    (u,), rays_u = _backward(mi, scene, [KEY], 8, spp, 11)
    print(f"{w}x{h}@{spp}: g {g} oracle {ref} unfused {u} rays {rays} / {rays_u}; "
          f"max rel vs unfused {np.max(np.abs(g - u) / np.abs(u)):.2e}, vs oracle {np.max(np.abs(g - ref) / np.abs(ref)):.2e}")
    assert rays == rays_u and rays[1] > w * h * spp  # more than one shadow ray per path
    np.testing.assert_allclose(g, ref, rtol=1e-3, atol=1e-7)
    np.testing.assert_allclose(g, u, rtol=1e-4)


def test_two_keys_take_the_four_slot_instance():
    mi = _mi()
    scene = _cbox(mi, 24, 24, 8)
    keys = [KEY, "red.reflectance.value"]
    g, _ = _backward(mi, scene, keys, 8, 8, 11)
    ref = _oracle(mi, scene, keys, 8, 8, 11)
    for a, b in zip(g, ref):
        assert np.abs(b).min() > 0
        np.testing.assert_allclose(a, b, rtol=1e-3, atol=1e-7)


def test_deterministic_call_is_bit_identical():
    mi = _mi()
    scene = _cbox(mi, 24, 24, 8)
    (a,), ra = _backward(mi, scene, [KEY], 8, 8, 11, deterministic=True)
    (b,), rb = _backward(mi, scene, [KEY], 8, 8, 11, deterministic=True)
    assert ra == rb
    np.testing.assert_array_equal(a, b)
    (ref,) = _oracle(mi, scene, [KEY], 8, 8, 11)
    np.testing.assert_allclose(a, ref, rtol=1e-3, atol=1e-7)
