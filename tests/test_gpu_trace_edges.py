"""GPU: every traversal engine against the oracle on the adversarial rays of
trace_cases (axis-aligned, far origin, in-plane, maxt edges, ties).

The criteria admit no fraction of rays, unlike test_gpu_parity's 99.99 %:

  no lost hit      where the oracle hits, the engine hits, and not farther;
                   where the oracle's shadow ray is occluded, so is the engine's
                   (the conservative-culling promise of mh_bvh.cpp)
  no invented hit  the engine never hits, hits nearer or reports occlusion
                   where the oracle does not (D <= 50 keeps the oracle's own
                   per-shape cull, 1e-4 absolute padding, out of the question)
  same payload     the same primitive gives the same t, u, v (as floats); the
                   same t gives the same primitive (ties: the lowest
                   (shape, prim), which is the one the oracle's scan keeps)

Engines (mh_api.hip picks by size and environment when the scene is created):

  lds-lane   <= 64 primitives: per-lane `traverse` on the LDS-resident BVH
  lds-65     65 primitives: the same, one primitive past the packet limit
  bvh2       MH_BVH4=0: per-lane BVH2 in global memory
  wide       > 32 KiB of BVH: stream engine, float BVH4
  wide-c     MH_PRIMC=1: float BVH4 + 48-byte PrimC records
  quant      MH_BVH4Q=1: quantised BVH4
  *-ovf      MH_STREAM_STACK=4: most pushes go to the global overflow columns

The packet engine and the fused bounce kernels are behind mh_render_samples
only: test_render_tiny_sphere.

Observed on the library before the box tests were made conservative in the
ray as well as in the box: see DESIGN.md §Parity (the table of this test's
cases) -- the render leg passed there, since camera rays are not aimed at
vertices, while class B lost hits.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_py as O
import trace_cases as TC

pytestmark = pytest.mark.gpu
INVALID = 0xFFFFFFFF

ENGINES = {
    "lds-lane": ("small", {}),
    "lds-65": ("65", {}),
    "bvh2": ("large", {"MH_BVH4": "0"}),
    "wide": ("large", {}),
    "wide-c": ("large", {"MH_PRIMC": "1"}),
    "quant": ("large", {"MH_BVH4Q": "1"}),
    "wide-ovf": ("large", {"MH_STREAM_STACK": "4"}),
    "quant-ovf": ("large", {"MH_BVH4Q": "1", "MH_STREAM_STACK": "4"}),
}
SWITCHES = ("MH_BVH4", "MH_BVH4Q", "MH_PRIMC", "MH_STREAM_STACK", "MH_BVH_LEAF", "MH_BVH_CT", "MH_TRAVERSAL",
            "MH_WF_FUSED", "MH_MODE")


def _mi():
    import mitsuba_hip as mi
    if not mi.is_available():
        pytest.fail("no HIP device / native library: the GPU tests need an MI355X")
    mi.set_variant("hip_ad_rgb")
    return mi


def _shapes(kind, size):
    big = size == "large"
    if kind == "sphere":
        return TC.tiny_sphere(12) if big else TC.tiny_sphere(4, extra=1 if size == "65" else 0)
    if kind in ("grid0", "grid03"):
        return TC.flat_grid(15 if big else 4, 0.0 if kind == "grid0" else 0.3)
    return TC.ties(15 if big else 1)


# ---------------------------------------------------------------------------
# the cases of one scene and the oracle's answers, computed once per
# (scene, size) and shared by the engines; never modified
# ---------------------------------------------------------------------------
_cases = {}


def _oracle(scene, rays):
    t, u, v, prim, shape = O.trace_closest(scene, rays)
    return {"t": t, "u": u, "v": v, "prim": prim, "shape": shape, "occ": O.trace_shadow(scene, rays)}


def cases(kind, size):
    """[(class name, rays, oracle result)] for the scene `kind` at `size`"""
    if (kind, size) in _cases:
        return _cases[(kind, size)]
    shapes = _shapes(kind, size)
    scene = TC.load(shapes)
    out = []

    def add(name, rays):
        r = _oracle(scene, rays)
        for a in r.values():
            a.setflags(write=False)
        out.append((name, rays, r))
        return r

    if kind == "sphere":
        V, F = TC.mesh_arrays(shapes)
        add("A", TC.rays_A(V, F))
        for D in (5, 50):
            for tg in ("vertex", "edge", "centroid"):
                add(f"B-{tg}-{D}", TC.rays_B(V, F, tg, D))
        base = TC.rays_generic(V, F)
    elif kind in ("grid0", "grid03"):
        V, F = TC.mesh_arrays(shapes)
        z = 0.0 if kind == "grid0" else 0.3
        add("A", TC.rays_A(V, F, flat=2))
        for part in ("in", "on", "graze", "off"):
            add(f"C-{part}", TC.rays_C(z, part))
        base = TC.rays_generic(V, F)
    else:
        base = TC.rays_E()
    # class D on every scene (for ties: E itself with maxt at the tie)
    r = add("E" if kind == "ties" else "D-inf", base)
    hit = r["shape"] != INVALID
    assert hit.mean() > 0.5
    at = add("D-at", TC.with_maxt(base, np.where(hit, r["t"], 1.0)))
    assert np.array_equal(at["shape"], r["shape"]) and np.all(at["occ"][hit] == 1)
    below = add("D-below", TC.with_maxt(base, np.where(hit, np.nextafter(r["t"], np.float32(0)), 1.0)))
    moved = hit & (r["t"] > 0)
    assert not (moved & (below["shape"] == r["shape"]) & (below["prim"] == r["prim"])).any()
    _cases[(kind, size)] = out
    return out


def gpu_trace(scene, rays):
    from mitsuba_hip import _abi as A
    n = rays.shape[1]
    t, u, v, t2, u2, v2 = (np.full(n, np.nan, np.float32) for _ in range(6))
    prim, shape, occ, prim2, shape2, inst = (np.full(n, 7, np.uint32) for _ in range(6))
    h = scene.handle(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rays = np.ascontiguousarray(rays)
    A.check(A.lib().mh_trace_closest(h, n, p(rays), p(t), p(u), p(v), p(prim), p(shape), 0, None))
    A.check(A.lib().mh_trace_shadow(h, n, p(rays), p(occ), 0, None))
    A.check(A.lib().mh_trace_preliminary(h, n, p(rays), p(t2), p(u2), p(v2), p(prim2), p(shape2), p(inst), 0, None))
    g = {"t": t, "u": u, "v": v, "prim": prim, "shape": shape, "occ": occ}
    # the preliminary entry point is the same trace plus the (null) instance
    for k, a in (("t", t2), ("u", u2), ("v", v2), ("prim", prim2), ("shape", shape2)):
        np.testing.assert_array_equal(a, g[k], err_msg=f"mh_trace_preliminary {k} differs from mh_trace_closest")
    assert np.all(inst == INVALID)
    return g


def bvh_bytes(scene):
    from mitsuba_hip import _abi as A
    nn, npr, dep = C.c_uint32(), C.c_uint32(), C.c_uint32()
    A.check(A.lib().mh_scene_bvh_info(scene.handle(0), C.byref(nn), C.byref(npr), C.byref(dep)))
    return 64 * (nn.value + npr.value), npr.value


def _show(rays, g, r, idx):
    lines = []
    for i in idx[:4]:
        lines.append(f"    ray {i}: o {rays[:3, i].tolist()} d {rays[3:6, i].tolist()} maxt {rays[6, i]!r}\n"
                     f"      engine (shape, prim, t, u, v, occ) = ({g['shape'][i]}, {g['prim'][i]}, {g['t'][i]!r}, "
                     f"{g['u'][i]!r}, {g['v'][i]!r}, {g['occ'][i]})\n"
                     f"      oracle (shape, prim, t, u, v, occ) = ({r['shape'][i]}, {r['prim'][i]}, {r['t'][i]!r}, "
                     f"{r['u'][i]!r}, {r['v'][i]!r}, {r['occ'][i]})")
    return "\n".join(lines)


def judge(case, rays, g, r):
    """the list of this case's failures (empty: the engine equals the oracle)"""
    ghit, rhit = g["shape"] != INVALID, r["shape"] != INVALID
    same = ghit & rhit & (g["shape"] == r["shape"]) & (g["prim"] == r["prim"])
    checks = {
        "lost hits": rhit & (~ghit | (g["t"] > r["t"])),
        "invented hits": ghit & (~rhit | (g["t"] < r["t"])),
        "lost occlusions": (r["occ"] != 0) & (g["occ"] == 0),
        "invented occlusions": (r["occ"] == 0) & (g["occ"] != 0),
        "payload differences on the same primitive": same & ~((g["t"] == r["t"]) & (g["u"] == r["u"]) & (g["v"] == r["v"])),
        "other primitive at the same t (tie rule)": ghit & rhit & ~same & (g["t"] == r["t"]),
        "miss payload not (prim 0, u = v = 0, t = +inf)":
            ~ghit & ~((g["prim"] == 0) & (g["u"] == 0) & (g["v"] == 0) & np.isposinf(g["t"])),
        "NaN outputs": np.isnan(g["t"]) | np.isnan(g["u"]) | np.isnan(g["v"]),
        "occlusion flag not 0 / 1": g["occ"] > 1,
    }
    fails = []
    for what, m in checks.items():
        idx = np.flatnonzero(m)
        if idx.size:
            fails.append(f"  {case}: {idx.size} of {rays.shape[1]} rays with {what}\n" + _show(rays, g, r, idx))
    return fails


# the 65th primitive belongs to the sphere: lds-65 has no other scene
@pytest.mark.parametrize("engine,kind", [(e, k) for e in ENGINES for k in ("sphere", "grid0", "grid03", "ties")
                                         if e != "lds-65" or k == "sphere"])
def test_trace_edges(engine, kind, monkeypatch):
    size, env = ENGINES[engine]
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _mi()
    cs = cases(kind, size)
    scene = TC.load(_shapes(kind, size))
    nbytes, nprims = bvh_bytes(scene)
    # the scene reaches the engine it is meant for
    if size == "large":
        assert nbytes > 32768, f"{kind}: the BVH ({nbytes} B) is LDS-resident, the global-memory engines are not reached"
    else:
        assert nbytes <= 32768 and (nprims == 65 if size == "65" else nprims <= 64), (nbytes, nprims)
    fails, hits = [], 0
    for name, rays, r in cs:
        g = gpu_trace(scene, rays)
        fails += judge(f"class {name}, scene {kind} ({nprims} primitives), engine {engine}", rays, g, r)
        hits += int((g["shape"] != INVALID).sum())
    scene.release()
    assert hits > 1000
    assert not fails, f"{len(fails)} failed checks:\n" + "\n".join(fails)


# ---------------------------------------------------------------------------
# the packet engine and the fused bounce kernels: mh_render_samples on the
# 64-triangle sphere seen through a narrow camera from 5 and from 50 away
# ---------------------------------------------------------------------------
SKY = np.array([1.0, 0.9, 0.8], np.float32)
_samples = {}


def _render_scene(distance, max_depth, extra=0):
    # the sphere (R = 0.01) spans 60 % of the frame
    fov = float(np.degrees(2 * np.arctan(TC.SPHERE_R / 0.6 / distance)))
    return TC.load(TC.tiny_sphere(4, extra=extra), distance=distance, fov=fov, max_depth=max_depth, spp=8, res=24)


def _oracle_samples(distance, max_depth, extra=0):
    key = (distance, max_depth, extra)
    if key not in _samples:
        scene = _render_scene(distance, max_depth, extra)
        L, pos, _ = O.sample_range(scene, scene.integrator(), 5, 8, 0, 24 * 24 * 8)
        L.setflags(write=False)
        pos.setflags(write=False)
        _samples[key] = (L, pos)
    return _samples[key]


def render_leg(distance, max_depth, flags, extra=0):
    """the per-sample criterion of test_gpu_parity (positions equal, >= 99.9 %
    of the samples bit-exact), and the same samples black, and the same
    samples seeing the sky directly, on both sides"""
    from mitsuba_hip import _abi as A
    rL, rpos = _oracle_samples(distance, max_depth, extra)
    scene = _render_scene(distance, max_depth, extra)
    n = 24 * 24 * 8
    out = np.zeros(5 * n, np.float32)
    ic = scene.integrator().c()
    A.check(A.lib().mh_render_samples(scene.handle(0), C.byref(ic), 5, 8, 0, 0, out.ctypes.data_as(C.c_void_p), flags))
    scene.release()
    L, pos = out[:3 * n].reshape(3, n).T, out[3 * n:].reshape(2, n).T
    np.testing.assert_array_equal(pos, rpos)
    exact = np.all(L == rL, axis=1)
    black, rblack = np.all(L == 0, axis=1), np.all(rL == 0, axis=1)
    sky, rsky = np.all(L == SKY, axis=1), np.all(rL == SKY, axis=1)
    on = ~rsky
    assert 0.15 < on.mean() < 0.6, f"the sphere covers {on.mean():.3f} of the samples"
    bad = np.flatnonzero(~exact)
    msg = f"distance {distance}, max_depth {max_depth}: " + "; ".join(
        f"sample {i} at {pos[i].tolist()}: L {L[i].tolist()} oracle {rL[i].tolist()}" for i in bad[:4])
    assert exact.mean() >= 0.999, f"bit-exact fraction {exact.mean()}; {msg}"
    assert np.array_equal(black, rblack), f"{(black != rblack).sum()} samples black on one side only; {msg}"
    assert np.array_equal(sky, rsky), f"{(sky != rsky).sum()} samples see the sky on one side only (pinholes); {msg}"


@pytest.mark.parametrize("max_depth", [2, 3])
@pytest.mark.parametrize("distance", [5, 50])
@pytest.mark.parametrize("mode", ["fused", "unfused", "lane", "mega", "fused-65"])
def test_render_tiny_sphere(mode, distance, max_depth, monkeypatch):
    """fused: the fused bounce kernel on the packet engine (64 primitives, the
    limit); unfused: trace / shade / shadow kernels on the packet engine;
    lane: those on the per-lane engine; mega: the megakernel; fused-65: one
    primitive past the packet limit.  Passed on the library whose box tests
    were conservative in the box only (camera rays are not aimed at vertices)."""
    from mitsuba_hip import _abi as A
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if mode == "unfused":
        monkeypatch.setenv("MH_WF_FUSED", "0")
    if mode == "lane":
        monkeypatch.setenv("MH_TRAVERSAL", "lane")
    _mi()
    render_leg(distance, max_depth, A.FLAG_MEGAKERNEL if mode == "mega" else A.FLAG_WAVEFRONT,
               extra=1 if mode == "fused-65" else 0)


def test_render_below_packet_limit():
    """MH_PACKET_MAX_PRIMS=32: the 64-triangle sphere is past the limit and the
    fused kernel takes the per-lane engine.  The limit is read once per
    process, so this leg runs in a child process of its own."""
    _mi()
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env["MH_PACKET_MAX_PRIMS"] = "32"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "5", "2"], env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, f"child failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}"
    assert "render leg ok" in p.stdout


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    for q in (os.path.join(os.path.dirname(here), "mitsuba3-nasa_amd"), here):
        if q not in sys.path:
            sys.path.insert(0, q)
    from mitsuba_hip import _abi as A_
    render_leg(int(sys.argv[1]), int(sys.argv[2]), A_.FLAG_WAVEFRONT)
    print("render leg ok")
