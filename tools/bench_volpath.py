#!/usr/bin/env python3
"""Config 4 measurement: volpath, heterogeneous 256^3 fBm
medium + HG, 256x256 @ 64 spp, one MI355X.  --integrator prbvolpath times the
§8(f) extension instead: one step = prbvolpath forward + render_backward wrt
the sigma_t grid and the albedo.  Prints one JSON line (not the driver's
bench line: bench.py measures BASELINE.json's headline metric).
--phase replaces the medium's HG (g = 0.85) by `rayleigh`, or by `tab`: the same
HG tabulated for `tabphase` on 1,801 cosines of a grid uniform in angle (0.1
degree), the size of a Mie table; the difference to hg is the cost of the
table searches; or by `blend`: a `blendphase` of `rayleigh` (air) and that table
(aerosol), the table's weight falling with height on a 64^3 grid of its own.
The CPU oracle has none of them, so these runs skip its baseline."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "mitsuba3-nasa_amd"), os.path.join(ROOT, "tests")]


def phase_spec(name):
    if name == "rayleigh":
        return {"type": "rayleigh"}
    if name == "tab":
        import numpy as np
        c = np.cos(np.deg2rad(np.linspace(180.0, 0.0, 1801)))
        c[0], c[-1] = -1.0, 1.0
        g = 0.85
        return {"type": "tabphase", "cost": c,
                "values": (1 - g * g) / (4 * np.pi * (1 + g * g - 2 * g * c) ** 1.5)}
    if name == "blend":
        import numpy as np
        from mitsuba_hip import Transform4f as T
        # child 0 = rayleigh: its weight rises with height (y), the aerosol's falls
        w = np.broadcast_to(np.linspace(0.1, 0.9, 64, dtype=np.float32)[None, :, None], (64, 64, 64))
        return {"type": "blendphase", "air": {"type": "rayleigh"}, "aerosol": phase_spec("tab"),
                "weight_0": {"type": "gridvolume", "data": np.ascontiguousarray(w),
                             "to_world": T.translate([-1.0, -1.0, -1.0]) @ T.scale([2.0, 2.0, 2.0])}}
    return {"type": "hg", "g": 0.85}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--cpu-spp", type=int, default=4)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--integrator", default="volpath", choices=["volpath", "prbvolpath"])
    ap.add_argument("--no-nee", action="store_true", help="medium sample_emitters = false (diagnostic)")
    ap.add_argument("--deterministic", action="store_true",
                    help="prbvolpath: MH_FLAG_DETERMINISTIC backward (int64 fixed-point grid + albedo gradients)")
    ap.add_argument("--overlap", action="store_true",
                    help="prbvolpath: forward || backward on two scene handles and streams (grad_in is constant)")
    ap.add_argument("--phase", default="hg", choices=["hg", "rayleigh", "tab", "blend"],
                    help="the medium's phase function: hg (g = 0.85), rayleigh, that hg as an 1,801-node tabphase, "
                         "or a blendphase of rayleigh and that table with a 64^3 weight grid")
    ap.add_argument("--phase-g", action="store_true",
                    help="prbvolpath: also differentiate the HG asymmetry (medium1.phase_function.g); the backward "
                         "then runs the per-sample kernel with its logs instead of the scheduler")
    a = ap.parse_args()
    a.no_cpu = a.no_cpu or a.phase != "hg" or a.phase_g   # the oracle has only isotropic and hg, and no g gradient
    import torch
    import mitsuba_hip as mi
    from mitsuba_hip import _abi as A
    mi.set_variant("hip_ad_rgb")
    t0 = time.time()
    grid = mi.fbm_grid(a.grid)
    d = mi.volume_cube(a.res, a.res, a.spp, grid=grid)
    d["integrator"]["type"] = a.integrator
    d["medium1"]["phase"] = phase_spec(a.phase)
    if a.no_nee:
        d["medium1"]["sample_emitters"] = False
    scene = mi.load_dict(d)
    t_load = time.time() - t0
    if a.integrator == "prbvolpath":
        return bench_prbvolpath(a, mi, A, scene, t_load)
    film = torch.empty((a.res, a.res, 4), dtype=torch.float32, device="cuda")
    st = A.Stats()
    mi.render_film(scene, seed=100, spp=a.spp, film=film, stats=st)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ks = []
    for i in range(a.steps):
        mi.render_film(scene, seed=i, spp=a.spp, film=film, stats=st)
        ks.append(st.ms_kernel)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    n = a.res * a.res * a.spp
    out = {"metric": "Msamples/s volpath config 4", "value": round(n / dt / 1e6, 2), "unit": "Msamples/s",
           "ms_per_render": round(dt * 1e3, 3), "kernel_ms": round(sum(ks) / len(ks), 3),
           "rays_closest_per_sample": round(st.rays_closest / n, 3),
           "rays_shadow_per_sample": round(st.rays_shadow / n, 3),
           "config": {"film": f"{a.res}x{a.res}", "spp": a.spp, "grid": f"{a.grid}^3 fBm", "phase": a.phase,
                      "scene_load_s": round(t_load, 2)}}
    if not a.no_cpu:
        import oracle_py as O
        thr = max(1, min(len(os.sched_getaffinity(0)), int(os.environ.get("OMP_NUM_THREADS", "16") or 16)))
        t0 = time.perf_counter()
        O.render(scene, seed=0, spp=a.cpu_spp, threads=thr)
        tc = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": round(a.res * a.res * a.cpu_spp / tc / 1e6, 3), "unit": "Msamples/s",
                               "cores": thr, "kind": "port", "sample": f"{a.res}^2 @ {a.cpu_spp} spp, {tc:.1f} s"}
    sub = vs_sub(A)
    if sub is not None:
        out["vs_subphases"] = sub
    print(json.dumps(out), flush=True)


def vs_sub(A):
    """MH_EXP_VSCNT builds: PvBwdMachine's POST / END sub-phase cycles summed
    over the calls since the library loaded (mh_exp_vs_sub); None otherwise."""
    import ctypes as C
    f = getattr(A.lib(), "mh_exp_vs_sub", None)
    if f is None:
        return None
    buf = (C.c_ulonglong * 16)()
    f(buf, 0)
    names = ["post_lane", "post_wave", "post_wave_load", "post_wave_scatter", "nee_entries", "end_lane",
             "end_wave", "end_wave_load", "end_wave_charge", "main_entries", "post_wave_steps", "end_wave_steps",
             "trace_traversal", "trace_continuation"]
    return {k: int(buf[i]) for i, k in enumerate(names)}


def bench_prbvolpath(a, mi, A, scene, t_load):
    import torch
    params = mi.traverse(scene)
    keys = ["medium1.sigma_t.data", "medium1.albedo.value"] + (["medium1.phase_function.g"] if a.phase_g else [])
    gi = torch.full((a.res, a.res, 3), 1.0 / (a.res * a.res * 3), device="cuda")
    sf, sb = A.Stats(), A.Stats()
    scene_f, run = scene, None
    if a.overlap:
        from mitsuba_hip import distributed as D
        d = mi.volume_cube(a.res, a.res, a.spp, grid=mi.fbm_grid(a.grid))
        d["integrator"]["type"] = a.integrator
        d["medium1"]["phase"] = phase_spec(a.phase)
        scene_f = mi.load_dict(d)  # the forward's own handle
        dev = torch.device("cuda:0")
        run = D.PairRunner((torch.cuda.Stream(dev), torch.cuda.Stream(dev)), dev)

    def step(seed):
        fwd = lambda: mi.render_film(scene_f, seed=seed, spp=a.spp, stats=sf)
        bwd = lambda: mi.render_backward(scene, params, gi, keys, seed=seed + 1, spp=a.spp, stats=sb,
                                         deterministic=a.deterministic)
        return run(fwd, bwd) if run else (fwd(), bwd())

    step(100)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kf, kb = [], []
    for i in range(a.steps):
        _, g = step(2 * i)
        kf.append(sf.ms_kernel)
        kb.append(sb.ms_kernel)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    n = a.res * a.res * a.spp
    sub = vs_sub(A)
    out = {"metric": "Msamples/s prbvolpath fwd + grad (sigma_t grid, albedo)", "value": round(n / dt / 1e6, 2),
           "unit": "Msamples/s", "ms_per_step": round(dt * 1e3, 3),
           "fwd_kernel_ms": round(sum(kf) / len(kf), 3), "bwd_kernel_ms": round(sum(kb) / len(kb), 3),
           "grad_sigma_t_abs_sum": float(g[0].abs().sum()), "grad_albedo": [float(x) for x in g[1]],
           "keys": keys, "grad_g": float(g[2][0]) if a.phase_g else None,
           "deterministic": a.deterministic, "overlap": a.overlap, "bwd_subphases": sub,
           "fwd_rays_closest_per_sample": round(sf.rays_closest / n, 3),
           "fwd_rays_shadow_per_sample": round(sf.rays_shadow / n, 3),
           "config": {"film": f"{a.res}x{a.res}", "spp": a.spp, "grid": f"{a.grid}^3 fBm", "phase": a.phase,
                      "scene_load_s": round(t_load, 2)}}
    if not a.no_cpu:
        import numpy as np
        import oracle_py as O
        thr = max(1, min(len(os.sched_getaffinity(0)), int(os.environ.get("OMP_NUM_THREADS", "16") or 16)))
        integ = scene.integrator()
        t0 = time.perf_counter()
        O.render(scene, integ, seed=0, spp=a.cpu_spp, threads=thr)
        O.render_backward(scene, integ, 1, a.cpu_spp, gi.cpu().numpy(), [params.param_id(k) for k in keys],
                          [tuple(params[k].shape) for k in keys], threads=thr)
        tc = time.perf_counter() - t0
        out["cpu_baseline"] = {"value": round(a.res * a.res * a.cpu_spp / tc / 1e6, 3), "unit": "Msamples/s",
                               "cores": thr, "kind": "port", "sample": f"{a.res}^2 @ {a.cpu_spp} spp fwd+bwd, {tc:.1f} s"}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
