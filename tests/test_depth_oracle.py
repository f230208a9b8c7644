"""CPU: what the oracle does at the edges of max_depth and rr_depth, pinned
before test_gpu_depth_limits.py uses it as the judge -- so that oracle and
kernel cannot share a misreading of the reference.

The reference's own lines (paths below the reference tree's src/):

path        integrators/path.cpp
  :103-104  max_depth == 0 returns { 0.f, false } before the loop: black, not valid
  :177      active_next = (depth + 1 < m_max_depth) && si.is_valid() -- after the
            emitter hit of this vertex has been added (:158-174): max_depth = k
            keeps emitter hits at vertices 0 .. k-1 and emitter samples at
            vertices 0 .. k-2
  :266      depth += 1 (valid intersections), BEFORE the roulette
  :270-272  rr_prob = min(max(throughput) eta^2, .95); rr_active = depth >= m_rr_depth
            on the incremented depth: the first roulette is at the end of the
            iteration of vertex rr_depth - 1
  :279      active = active_next && (!rr_active || rr_continue) && throughput_max != 0
prb         python/python/ad/integrators/prb.py
  (none)    no max_depth == 0 test: the first iteration always runs and adds the
            emitter the camera ray sees (:121-135), so max_depth 0 equals 1
  :140      active_next &= (depth + 1 < self.max_depth) & si.is_valid()
  :193-198  rr_prob = min(beta_max eta^2, .95); rr_active = depth >= self.rr_depth
            on the depth NOT yet incremented ...
  :250      ... depth[si.is_valid()] += 1 comes last: the first roulette is at the
            end of the iteration of vertex rr_depth, one later than path.  path
            at rr_depth k + 1 is prb at rr_depth k
volpath     integrators/volpath.cpp
  :145-148  at the loop head: q = min(max(throughput) eta^2, .95);
            perform_rr = depth > m_rr_depth (strictly: one vertex later than
            path at the same rr_depth); the draw is taken for every active lane
  :150      active &= depth < m_max_depth: max_depth == 0 ends before anything is
            added -- black, but valid_ray keeps its initial value
            !hide_emitters && environment (:115), so alpha is 1 under a sky
  :198, :314  depth += 1 at a medium scatter / a non-null surface
  :203      active &= depth < m_max_depth again after the scatter: the vertex
            that reaches max_depth adds nothing
  :285      surface emitter sampling needs depth + 1 < m_max_depth
prbvolpath  python/python/ad/integrators/prbvolpath.py
  :146-149  q = min(max(throughput) eta^2, 0.99) -- not .95; perform_rr =
            depth > self.rr_depth
  (none)    no depth test at the loop head and none for max_depth == 0
  :188, :321  depth += 1 at a medium scatter / a non-null surface
  :192      active &= depth < self.max_depth after the medium scatter
  :243      active_e_surface needs depth + 1 < self.max_depth
  :216-234  emitter hits are not counted (the fork), so max_depth 0 and 1 are
            black with valid_ray false: nothing is added before depth reaches 1

The oracle (oracle/mh_oracle.c) restates these conditions literally; the tests
below hold it to their consequences.
"""
import functools

import numpy as np
import pytest

import depth_cases as DC
import oracle_py as O

SEED = 3
EPS = 2.0 ** -24
RADIANCE = np.array([18.387, 13.9873, 6.75357], np.float32)


def _mi():
    import mitsuba_hip as mi
    mi.set_variant("hip_ad_rgb")
    return mi


@functools.lru_cache(maxsize=None)
def _scene(name, w, h, spp):
    mi = _mi()
    if name == "room":
        return mi.load_dict(DC.room(mi, w, h, spp))
    if name == "room_boxes":
        return mi.load_dict(DC.room(mi, w, h, spp, boxes=True))
    kind, itype = name.split(":")
    kw = {"dense": {}, "dense09": {"albedo": 0.9}, "dense20": {"scale": 20.0, "albedo": 0.99}}[kind]
    return mi.load_dict(DC.dense(mi, itype, w, h, spp, **kw))


@functools.lru_cache(maxsize=None)
def _samples(name, itype, max_depth, rr_depth, w=24, h=None, spp=8):
    """(L, pos, valid) of every sample; computed once, shared, read-only."""
    h = h or (24 if name.startswith("room") else 20)
    scene = _scene(name, w, h, spp)
    out = O.sample_range(scene, DC.integrator(_mi(), itype, max_depth, rr_depth), SEED, spp, 0, w * h * spp)
    for a in out:
        a.setflags(write=False)
    return out


def _room(itype, max_depth, rr_depth, **kw):
    return _samples("room", itype, max_depth, rr_depth, **kw)


def _dense(itype, max_depth, rr_depth, kind="dense", **kw):
    return _samples(f"{kind}:{itype}", itype, max_depth, rr_depth, **kw)


def _changed(a, b):
    return np.any(a != b, axis=1).mean()


# ---------------------------------------------------------------------------
# max_depth 0 and 1
# ---------------------------------------------------------------------------
def test_max_depth_0():
    L, _, valid = _room("path", 0, 5)
    assert not L.any() and not valid.any()                       # path.cpp:103-104
    L0, _, v0 = _room("prb", 0, 5)
    L1, _, v1 = _room("prb", 1, 5)
    assert np.array_equal(L0, L1) and np.array_equal(v0, v1) and L0.any()   # prb.py: no such test
    L, _, valid = _dense("volpath", 0, 5)
    assert not L.any() and valid.all()                           # volpath.cpp:150, :115 (a sky: valid)
    for md in (0, 1):
        L, _, valid = _dense("prbvolpath", md, 5)
        assert not L.any() and not valid.any()                   # prbvolpath.py:216-234


def _sees_light(pos, w, h):
    """The camera ray of film position pos meets the room's light: from
    (0, 0, 0.95) along (dx, dy, -1), fov 90 over a square film, to the plane
    y = 0.99 and the light's rectangle |x| <= 0.23, |z - 0.01| <= 0.19.
    Returns (inside, near): near marks the hits within 1e-4 of its border."""
    dx = 1.0 - 2.0 * pos[:, 0].astype(np.float64) / w
    dy = 1.0 - 2.0 * pos[:, 1].astype(np.float64) / h
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(dy > 0, 0.99 / dy, np.inf)
        ex = np.abs(dx * t) - 0.23
        ez = np.abs(0.95 - t - 0.01) - 0.19
    e = np.maximum(ex, ez)
    e = np.where(np.isfinite(e), e, np.inf)
    return e < 0, np.abs(e) < 1e-4


@pytest.mark.parametrize("itype", ["path", "prb"])
def test_max_depth_1_room_sees_only_the_light(itype):
    L, pos, _ = _room(itype, 1, 5)
    inside, near = _sees_light(pos, 24, 24)
    lit = L.any(axis=1)
    assert 20 < inside.sum() < 0.05 * len(L)
    assert np.array_equal(lit[~near], inside[~near])
    # throughput 1, MIS weight 1: the radiance itself (path.cpp:158-174, prb.py:121-135)
    assert np.all(L[lit] == RADIANCE)


def test_max_depth_1_dense_sees_only_the_sky():
    """volpath: a camera ray that misses the cube returns the sky; one that
    enters scatters (transmittance exp(-200 * length)) and stops at depth 1."""
    L, pos, _ = _dense("volpath", 1, 5)
    fov = np.deg2rad(39.3077)
    s = np.tan(fov / 2)   # fov over the smaller axis (20 rows); the aspect widens x
    dx = (1.0 - 2.0 * pos[:, 0].astype(np.float64) / 24) * s * 24 / 20
    dy = (1.0 - 2.0 * pos[:, 1].astype(np.float64) / 20) * s
    # the front face z = 1 of [-1, 1]^3 from (0, 0, 4) along (dx, dy, -1): t = 3
    e = np.maximum(np.abs(3 * dx), np.abs(3 * dy)) - 1.0
    # a ray that enters |e| inside the silhouette leaves through a side face
    # after a chord of about 3 |e| (it drifts outwards by 1/3 per unit of t):
    # transmittance exp(-600 |e|), below 1e-13 once |e| > 0.05
    near = (e > -0.05) & (e < 1e-3)
    lit = L.any(axis=1)
    assert (e > 0).mean() > 0.1 and (e < 0).mean() > 0.3
    assert np.array_equal(lit[~near], (e > 0)[~near])
    assert np.all(L[lit] == np.float32(0.2))


# ---------------------------------------------------------------------------
# monotone in max_depth: the same RNG prefix, only non-negative terms added
# ---------------------------------------------------------------------------
SURFACE_DEPTHS = [0, 1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65]


@pytest.mark.parametrize("itype", ["path", "prb"])
def test_monotone_in_max_depth_room(itype):
    for a, b in zip(SURFACE_DEPTHS[:-1], SURFACE_DEPTHS[1:]):
        assert np.all(_room(itype, b, 1000)[0] >= _room(itype, a, 1000)[0]), (a, b)


@pytest.mark.parametrize("itype", ["volpath", "prbvolpath"])
def test_monotone_in_max_depth_dense(itype):
    depths = SURFACE_DEPTHS + [1023, 1024, 1025, 1026]
    for a, b in zip(depths[:-1], depths[1:]):
        La, Lb = _dense(itype, a, 100000)[0], _dense(itype, b, 100000)[0]
        assert np.isfinite(Lb).all()
        assert np.all(Lb >= La), (a, b)


# ---------------------------------------------------------------------------
# max_depth = -1
# ---------------------------------------------------------------------------
def test_unbounded_equals_a_large_bound():
    for itype in ("path", "prb"):
        for rr in (1, 5, 1000):
            inf = _room(itype, -1, rr)[0]
            assert np.array_equal(inf, _room(itype, 100000, rr)[0]), (itype, rr)
            if rr <= 5:   # the roulette ends every path of the room before vertex 65
                assert np.array_equal(inf, _room(itype, 65, rr)[0]), (itype, rr)
    for itype in ("volpath", "prbvolpath"):
        for rr in (1, 100000):
            assert np.array_equal(_dense(itype, -1, rr)[0], _dense(itype, 100000, rr)[0]), (itype, rr)


# ---------------------------------------------------------------------------
# path at rr_depth k + 1 is prb at rr_depth k
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 5])
@pytest.mark.parametrize("max_depth", [8, 65])
def test_path_prb_roulette_offset(k, max_depth):
    """Not bit-equal (about a quarter of the samples are; measured 25-26 %):
    both walk the same vertices with the same throughput bits, but path adds
    an emitter sample as fma(throughput, (bsdf_val * em_weight) * mis, result)
    (path.cpp:220-230) and prb as L + ((beta * mis) * bsdf_val) * em_weight
    (prb.py:156-163, 174): another association of the same product.  Each of
    the at most 2 * max_depth terms (an emitter hit and an emitter sample per
    vertex) carries at most 4 roundings in either form, and the partial sums
    are non-negative and grow, so each form is within (2 * max_depth + 4) * eps
    * L of the exact sum and the two within twice that of each other, eps =
    2^-24.  Measured: at most 9.6e-7 absolute on L up to 21.  At the SAME
    rr_depth the two differ in all but the 1.4 % of samples that see the light
    and stop -- the offset is not cosmetic."""
    a = _room("path", max_depth, k + 1)[0]
    b = _room("prb", max_depth, k)[0]
    bound = 2 * (2 * max_depth + 4) * EPS * np.maximum(a, b)
    d = np.abs(a - b)
    print(f"k={k} max_depth={max_depth}: bit-equal {np.all(a == b, axis=1).mean():.4f}, max |d| {d.max():.3e}, "
          f"max d/bound {np.max(d / np.maximum(bound, 1e-30)):.3f}")
    assert np.array_equal(a > 0, b > 0)
    assert np.all(d <= bound)
    same = _room("prb", max_depth, k + 1)[0]
    assert np.any(np.abs(a - same) > bound, axis=1).mean() > 0.5


# ---------------------------------------------------------------------------
# the roulette is unbiased: per-channel image means within 4 standard errors
# ---------------------------------------------------------------------------
def _mean_se(L):
    return L.mean(axis=0, dtype=np.float64), L.std(axis=0, dtype=np.float64, ddof=1) / np.sqrt(len(L))


def _assert_unbiased(get, never):
    m0, s0 = _mean_se(get(never))
    for rr in (1, 5):
        m, s = _mean_se(get(rr))
        z = np.abs(m - m0) / np.sqrt(s * s + s0 * s0)
        print(f"rr_depth {rr}: mean {m}, never {m0}, |z| {z}")
        assert np.all(z < 4.0), (rr, m, m0, z)


@pytest.mark.parametrize("itype", ["path", "prb"])
def test_roulette_unbiased_room(itype):
    _assert_unbiased(lambda rr: _room(itype, -1, rr, w=16, h=16, spp=64)[0], 1000)


@pytest.mark.parametrize("itype", ["volpath", "prbvolpath"])
def test_roulette_unbiased_dense(itype):
    _assert_unbiased(lambda rr: _dense(itype, -1, rr, kind="dense09", w=16, h=16, spp=64)[0], 100000)


# ---------------------------------------------------------------------------
# reach floors at the GPU tests' sizes: their boundary cases are not vacuous
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("itype", ["path", "prb"])
def test_reach_room(itype):
    """Measured at 24 x 24 @ 8: 82 % (31 -> 32), 81 % (32 -> 33), 80 %
    (63 -> 64), 79 % (64 -> 65)."""
    for a, b in ((31, 32), (32, 33), (63, 64), (64, 65)):
        f = _changed(_room(itype, a, 1000)[0], _room(itype, b, 1000)[0])
        print(f"{itype} room {a} -> {b}: {f:.4f}")
        assert f >= 0.5, (a, b, f)


def test_reach_dense():
    """Measured at 24 x 20 @ 8: volpath 2.7 % (1023 -> 1024) and 3.0 %
    (1024 -> 1025); max_depth -1 against 65 differs in 31 % (volpath) and 32 %
    (prbvolpath) of the samples; the scale-20 medium 4.5 % / 4.7 % at 63 -> 64."""
    for a, b in ((1023, 1024), (1024, 1025)):
        f = _changed(_dense("volpath", a, 100000)[0], _dense("volpath", b, 100000)[0])
        print(f"volpath dense {a} -> {b}: {f:.4f}")
        assert f >= 0.01, (a, b, f)
    for itype in ("volpath", "prbvolpath"):
        f = _changed(_dense(itype, -1, 100000)[0], _dense(itype, 65, 100000)[0])
        print(f"{itype} dense -1 against 65: {f:.4f}")
        assert f >= 0.02, (itype, f)
        f = _changed(_dense(itype, 63, 100000, kind="dense20")[0], _dense(itype, 64, 100000, kind="dense20")[0])
        print(f"{itype} scale 20, 63 -> 64: {f:.4f}")
        assert f >= 0.02, (itype, f)


def test_reach_roulette_clamp():
    """The 0.95 clamp is active: with rr_depth 1 some paths of the room live
    past vertex 32 (a probability of at most 0.95 per vertex; without the clamp
    white's 0.97 would carry more), none past 64."""
    for itype in ("path", "prb"):
        f = _changed(_room(itype, 32, 1)[0], _room(itype, 33, 1)[0])
        print(f"{itype} rr_depth 1, 32 -> 33: {f:.4f}")
        assert f >= 0.005
        assert np.array_equal(_room(itype, 64, 1)[0], _room(itype, 65, 1)[0])
