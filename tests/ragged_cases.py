"""Launch shapes that are not "round" ("Launch geometry"): sample
counts and slab sizes that are no power of two, path counts below a wave and
no multiple of 64, film widths below 8 and no multiple of 8, chunks that start
in the middle of a pixel row.  One table, shared by the CPU test that pins the
oracle at these shapes (test_ragged_oracle.py) and by the device-against-oracle
tests (test_gpu_ragged_launch.py).  A plain helper module; importing it needs
no GPU.

  name     W x H @ spp  slab(s)               what it reaches
  tiny      7 x 1 @ 3   full                  21 samples: less than a wave, 43 empty queue segments,
                                              spp < 4 (the non-coalesced generic splat), W < 8 (no
                                              column bands in k_vol_sched), H = 1
  odd      13 x 7 @ 5   full                  455 samples, S < 16, W >= 8 with W % 8 != 0, a short
                                              last segment
  over16   20 x 9 @ 17  full                  the second 16-lane round of the splat holds one sample
  over32   11 x 6 @ 33  full                  the third round holds one sample
  chunks   27 x 20 @ 12 full, MH_WF_CHUNK=1024  85 pixels = 1,020 samples per chunk (no whole number
                                              of waves), ceil(540 / 85) = 7 chunks that start mid-row
                                              on alternating streams; `chunks1s`: the same on one stream
  slabs12  27 x 5 @ 12  [0,4) [4,7) [7,12)    a power-of-two S inside a non-power-of-two spp (shift +
                                              division in lane_of), S = 3, S = 5, s_begin != 0
  slab16   13 x 7 @ 16  [3,10)                S = 7 inside spp = 16 (division + shift)

The environment of a case (`env`) applies to the calls that chunk
(mh_render, mh_render_backward); mh_render_samples always runs one launch.
"""
from collections import namedtuple

import numpy as np

import vol_cases as VC

Case = namedtuple("Case", "name w h spp slabs env")

CHUNK = 1024  # MH_WF_CHUNK of `chunks`; also plan::split_chunks' max_samples in the planner cases


def _case(name, w, h, spp, slabs=None, env=()):
    return Case(name, w, h, spp, tuple(slabs or [(0, spp)]), tuple(env))


CASES = {c.name: c for c in (
    _case("tiny", 7, 1, 3),
    _case("odd", 13, 7, 5),
    _case("over16", 20, 9, 17),
    _case("over32", 11, 6, 33),
    _case("chunks", 27, 20, 12, env=[("MH_WF_CHUNK", str(CHUNK))]),
    _case("chunks1s", 27, 20, 12, env=[("MH_WF_CHUNK", str(CHUNK)), ("MH_WF_STREAMS", "1")]),
    _case("slabs12", 27, 5, 12, [(0, 4), (4, 7), (7, 12)]),
    _case("slab16", 13, 7, 16, [(3, 10)]),
)}
FULL = ["tiny", "odd", "over16", "over32", "chunks"]   # the table's full-slab cases (chunks1s: where calls chunk)
SLABBED = ["slabs12", "slab16"]


def n_px(case):
    return case.w * case.h


def n_chunks(case):
    """Chunks of a chunking call under the case's MH_WF_CHUNK (plan::split_chunks)."""
    chunk_px = max(1, min(n_px(case), CHUNK // case.spp))
    return -(-n_px(case) // chunk_px)


def launches(names):
    """[(case, b, e)]: every slab of every named case, as pytest parameters with readable ids."""
    import pytest
    out = []
    for n in names:
        c = CASES[n]
        for b, e in c.slabs:
            full = (b, e) == (0, c.spp)
            out.append(pytest.param(c, b, e, id=n if full else f"{n}[{b},{e})"))
    return out


def apply_env(case, monkeypatch):
    for k in ("MH_WF_CHUNK", "MH_WF_STREAMS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env:
        monkeypatch.setenv(k, v)


def slab_lanes(case, b, e):
    """Oracle lane indices pixel * spp + s of slab [b, e), pixel-major with
    S = e - b lanes per pixel: the order in which mh_render_samples writes a
    slab.  O.sample_range(...)[i][slab_lanes(case, b, e)] is the slab's reference."""
    px = np.arange(n_px(case), dtype=np.int64)[:, None]
    return (px * case.spp + np.arange(b, e, dtype=np.int64)[None, :]).reshape(-1)


def slab_kw(case, b, e):
    """spp_begin / spp_end of a call (nothing for the full slab)."""
    return {} if (b, e) == (0, case.spp) else {"spp_begin": b, "spp_end": e}


# ---- scenes -------------------------------------------------------------------
def _shape(d, case, fmt=None):
    d["sensor"]["film"].update(width=case.w, height=case.h)
    d["sensor"]["sampler"]["sample_count"] = case.spp
    if fmt:
        d["sensor"]["film"]["pixel_format"] = fmt
    return d


def cbox(mi, case, fmt=None):
    return mi.load_dict(_shape(mi.cornell_box(), case, fmt))


def cbox_bitmap(mi, case, tex_res=8):
    return mi.load_dict(_shape(mi.cornell_box_bitmap(tex_res=tex_res), case))


HOMOGENEOUS = {"medium_type": "homogeneous", "sigma_t": 0.8, "scale": 1.0}


def vol(mi, case, integrator="volpath", homogeneous=False):
    """volume_cube (fbm_grid(16), scale 4, or the homogeneous medium of the
    parity tests) with the floor below it, max_depth 6, rr_depth 5."""
    return mi.load_dict(VC.base(mi, integrator, case.w, case.h, case.spp, **(HOMOGENEOUS if homogeneous else {})))


def vol_keys(homogeneous=False):
    return ["medium1.sigma_t." + ("value" if homogeneous else "data"), "medium1.albedo.value", VC.FLOOR_KEY]


def blob(mi, case, n_tri=6000, max_depth=6):
    """The cornell box with a displaced UV sphere of about 6,000 triangles
    (test_gpu_chunk_streams._blob): a BVH in global memory, traced by the
    per-lane stream engine on the unfused trace / shade / shadow kernels."""
    m = max(8, int(np.sqrt(n_tri / 4)))
    th = np.linspace(0, np.pi, m + 1)
    ph = np.linspace(0, 2 * np.pi, 2 * m + 1)
    T_, P_ = np.meshgrid(th, ph, indexing="ij")
    r = 1.0 + 0.08 * np.sin(7 * T_) * np.cos(9 * P_)
    V = np.stack([r * np.sin(T_) * np.cos(P_), r * np.cos(T_), r * np.sin(T_) * np.sin(P_)], -1).reshape(-1, 3)
    a = (np.arange(m)[:, None] * (2 * m + 1) + np.arange(2 * m)[None, :]).reshape(-1)
    F = np.concatenate([np.stack([a, a + 2 * m + 1, a + 1], 1), np.stack([a + 1, a + 2 * m + 1, a + 2 * m + 2], 1)])
    d = _shape(mi.cornell_box(), case)
    d["integrator"]["max_depth"] = max_depth
    T = mi.Transform4f
    d["blob"] = {"type": "mesh", "vertex_positions": V.astype(np.float32), "faces": F.astype(np.uint32),
                 "to_world": T.translate([0, -0.45, 0]) @ T.scale(0.45), "bsdf": {"type": "ref", "id": "white"}}
    return mi.load_dict(d)


# ---- criteria (tests/test_gpu_parity.py's docstring) -------------------------
def film_close(a, b, frac=0.995):
    ok = np.all(np.abs(a - b) <= 1e-4 * np.maximum(1.0, np.abs(b)), axis=-1)
    return ok.mean() >= frac, ok.mean()


def assert_per_sample(L, rL):
    """>= 99.9 % of the samples bit-identical, every other one within
    1e-4 max(1, |L|).  Below 1,000 samples 0.1 % is less than one sample:
    at most one may differ in bits."""
    assert L.shape == rL.shape
    exact = np.all(L == rL, axis=1)
    close = np.all(np.abs(L - rL) <= 1e-4 * np.maximum(1, np.abs(rL)), axis=1)
    n, bad = exact.size, int((~exact).sum())
    print(f"per sample: {bad} of {n} differ in bits, {int((~close).sum())} beyond the tolerance")
    assert bad <= max(1, int(n * 0.001)), f"{bad} of {n} samples differ in bits"
    assert close.all(), f"{int((~close).sum())} of {n} samples beyond 1e-4 max(1, |L|)"
