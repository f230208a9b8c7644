"""CPU: the oracle at the launch shapes of ragged_cases.py, pinned before
test_gpu_ragged_launch.py uses it as the judge, so that a failure there is the
device code's.  The oracle has none of the device's branches on these shapes
(shift or division in lane_of, 16-lane splat rounds, queue segments, column
bands, chunks): it is plain C indexed by the lane.  Held to:

* every sample's position floors to pixel lane // spp (integrator.cpp:323-340);
* the films and W images of a case's slabs sum to the full render (the
  suite's film criterion, on 100 % of the pixels; W at prb_weights' rtol 1e-5);
* the PRB gradients of the slabs, given the full W image, sum to the full
  gradient (rtol 1e-5: the same per-sample terms in another order, in double);
* plan::split_chunks at 1024 samples per chunk (tools/plan_check.cpp; the
  literal values are in test_plan_host.py): a chunk holds at most 1024
  samples, the chunks tile [0, n_px) exactly and there are
  ceil(n_px / chunk_px) of them.
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_py as O
import ragged_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [n for n in RC.CASES if n != "chunks1s"]   # the same shape as `chunks`
SEED = 3


def _mi():
    import mitsuba_hip as mi
    mi.set_variant("hip_ad_rgb")
    return mi


@pytest.mark.parametrize("name", NAMES)
def test_positions_floor_to_the_lanes_pixel(name):
    mi = _mi()
    c = RC.CASES[name]
    scene = RC.cbox(mi, c)
    integ = mi.load_dict({"type": "path", "max_depth": 2})
    n = RC.n_px(c) * c.spp
    _, pos, _ = O.sample_range(scene, integ, SEED, c.spp, 0, n)
    pix = np.arange(n) // c.spp
    np.testing.assert_array_equal(np.floor(pos[:, 0]).astype(np.int64), pix % c.w)
    np.testing.assert_array_equal(np.floor(pos[:, 1]).astype(np.int64), pix // c.w)
    for b, e in c.slabs:   # the slab helper picks lanes [b, e) of every pixel, pixel-major
        lanes = RC.slab_lanes(c, b, e)
        assert lanes.shape == (RC.n_px(c) * (e - b),)
        np.testing.assert_array_equal(lanes // c.spp, np.repeat(np.arange(RC.n_px(c)), e - b))
        np.testing.assert_array_equal(lanes % c.spp, np.tile(np.arange(b, e), RC.n_px(c)))


def _cover(c):
    """Slabs that partition [0, spp): the case's own, completed at both ends."""
    cuts = sorted({0, c.spp} | {x for s in c.slabs for x in s})
    return list(zip(cuts[:-1], cuts[1:]))


@pytest.mark.parametrize("name", RC.SLABBED + ["odd", "tiny"])
def test_slab_films_and_weights_sum_to_the_full_render(name):
    mi = _mi()
    c = RC.CASES[name]
    cover = _cover(c) if name in RC.SLABBED else [(0, 2), (2, c.spp)]
    scene = RC.cbox(mi, c)
    integ = mi.load_dict({"type": "path", "max_depth": 6})
    full = O.render(scene, integ, seed=SEED, spp=c.spp)
    acc = sum(O.render(scene, integ, seed=SEED, spp=c.spp, spp_begin=b, spp_end=e) for b, e in cover)
    assert full[..., 3].min() > 0
    ok, frac = RC.film_close(acc, full, 1.0)
    assert ok, f"slab films: {frac} of the pixels"
    w = O.prb_weights(scene, SEED, c.spp)
    wacc = sum(O.prb_weights(scene, SEED, c.spp, b, e) for b, e in cover)
    np.testing.assert_allclose(wacc, w, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(w, full[..., 3], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", RC.SLABBED)
def test_slab_gradients_sum_to_the_full_gradient(name):
    mi = _mi()
    c = RC.CASES[name]
    scene = RC.cbox(mi, c)
    integ = mi.load_dict({"type": "prb", "max_depth": 6})
    params = mi.traverse(scene)
    keys = ["white.reflectance.value", "red.reflectance.value"]
    tex = [params.texture_of(k) for k in keys]
    gi = np.random.default_rng(2).random((c.h, c.w, 3)).astype(np.float32) / (c.h * c.w * 3)
    w = O.prb_weights(scene, SEED, c.spp)
    full = O.render_backward(scene, integ, SEED, c.spp, gi, tex, [(3,), (3,)])
    with_w = O.render_backward(scene, integ, SEED, c.spp, gi, tex, [(3,), (3,)], weights=w)
    acc = [np.zeros(3, np.float64), np.zeros(3, np.float64)]
    for b, e in _cover(c):
        for a, g in zip(acc, O.render_backward(scene, integ, SEED, c.spp, gi, tex, [(3,), (3,)], weights=w,
                                               spp_begin=b, spp_end=e)):
            a += g
    for a, f, fw in zip(acc, full, with_w):
        assert np.abs(f).min() > 0
        np.testing.assert_allclose(fw, f, rtol=1e-5)
        np.testing.assert_allclose(a, f, rtol=1e-5)


# ---- plan::split_chunks at these shapes -----------------------------------------
@pytest.fixture(scope="module")
def splits(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path_factory.mktemp("ragged_plan") / "plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "tools", "plan_check.cpp"), "-o", exe], check=True,
                   capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True)
    rows = [json.loads(line) for line in r.stdout.splitlines()]
    return {row["case"]: row for row in rows if row["case"].startswith("split_ragged_")}


def test_split_chunks_covers_every_launch(splits):
    want = {"split_ragged_" + (n if (b, e) == (0, c.spp) else f"{n}_{b}_{e}")
            for n, c in RC.CASES.items() for b, e in c.slabs}
    assert set(splits) == want


@pytest.mark.parametrize("name", list(RC.CASES))
def test_split_chunks_properties(name, splits):
    c = RC.CASES[name]
    n_px = RC.n_px(c)
    for b, e in c.slabs:
        row = splits["split_ragged_" + (name if (b, e) == (0, c.spp) else f"{name}_{b}_{e}")]
        chunk_px, n_chunks = row["chunk_px"], row["n_chunks"]
        assert chunk_px >= 1 and chunk_px * (e - b) <= RC.CHUNK
        # mh_render's loop: chunk i is [i * chunk_px, min((i + 1) * chunk_px, n_px))
        begins = list(range(0, n_px, chunk_px))
        ends = [min(p + chunk_px, n_px) for p in begins]
        assert len(begins) == n_chunks == -(-n_px // chunk_px)
        assert begins[0] == 0 and ends[-1] == n_px and begins[1:] == ends[:-1] and all(e_ > b_ for b_, e_ in zip(begins, ends))
        if (b, e) == (0, c.spp):
            assert n_chunks == RC.n_chunks(c)
    if name.startswith("chunks"):   # what the case is for: no whole waves, mid-row starts, both streams
        row = splits["split_ragged_" + name]
        assert (row["chunk_px"] * c.spp) % 64 != 0 and row["chunk_px"] % c.w != 0 and row["n_chunks"] == 7
        assert row["two"] == (0 if name == "chunks1s" else 1)
