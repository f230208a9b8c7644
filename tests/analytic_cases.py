"""Single-scatter closed forms of the medium cube, evaluated in float64 numpy:
the references of test_sigma_t_analytic_oracle.py (CPU oracle) and
test_gpu_sigma_t_analytic.py (device), independent of both.

The set-up.  prbvolpath with max_depth = 2, the directional sun as the only
emitter and a near-zero field of view: every camera ray is the camera's axis,
a path scatters once, and the sun is attenuated along the shadow ray
(prbvolpath.py:357-359).  With x(u) the camera segment inside the cube, w the
sun-ward direction, l(u) the distance from x(u) along w to the cube's boundary,
sigma(x) = scale * tri(grid, x) (a constant when homogeneous) and

    T(u) = exp(- int_0^u sigma dcam - int_0^l(u) sigma dsun),

the mean radiance and its derivative along a texel direction `mask` are

    L        = E a f  int sigma(x(u)) T(u) du
    dL[mask] = E a f  int [ m(x(u)) - sigma(x(u)) (int_0^u m dcam + int_0^l(u) m dsun) ] T(u) du
    m(x)     = scale * tri(mask, x)

with E the sun's irradiance, a the albedo and f the phase function at the one
scattering angle.  The homogeneous value has the one-dimensional form

    dL / d sigma_t = scale E a f  int (1 - S (u + l)) exp(-S (u + l)) du,   S = scale * sigma_t

and dL / da = L / a.  With albedo 0 and a diffuse wall (reflectance rho) behind
the cube nothing scatters in the medium, and the wall is seen and lit through
it (scene C):

    L        = rho / pi  E cos(theta)  exp(-tau_cam - tau_sun)
    dL[mask] = -(int m dcam + int m dsun) L.

One quirk of the reference enters the forms.  A ray that
crosses the cube's null boundary is spawned again 1.79e-4 inside the face
(Interaction::offset_p), and the medium is tracked from there: the camera
integrals start at u0 = 1.79e-4, not at 0, and so does the wall's shadow ray
inside the cube; the sun-ward integrals from a scattering point run to the face
itself.  Without it the forms are off by -0.07 % at S = 2, many standard errors.

dL[mask] is linear in the mask, so the quadrature is done once per texel (the
float64 gradient field G) and dL[mask] = <G, mask>.  Every quadrature is the
trapezoid rule along u and, per u, along the sun segment; each helper returns
the value at a coarse and at a fine resolution, and the tests assert that the
two agree to 1e-4 relative before they use the fine one.

The grid lookup is restated from its rule (grid.cpp:502-558): texel centres at
(i + 0.5) / res, linear weights, clamped indices, array order [z, y, x], world
-> [0, 1]^3 by the inverse of the volume's to_world.

Only numpy and the scene dictionaries of mitsuba_hip.volume_cube are used here.
"""
import functools

import numpy as np

# ---------------------------------------------------------------------------
# the sizes every test of the two files shares
# ---------------------------------------------------------------------------
W = H = 8
SPP = 16384                               # 8192 leaves three of the masks of case B above the SE cap (1.0 - 1.3 %)
BACKWARD_SEEDS = tuple(range(1, 17))      # 16 seeds: 8 underestimate the standard error (a spurious |z| of 5)
PRIMAL_SEEDS = tuple(range(101, 117))     # disjoint from the backward seeds
FOV = 0.01
SUN = 5.0
ALBEDO = 0.7
SE_CAP = 0.01                             # a condition on the case, not a measurement
QUAD_RTOL = 1e-4
RES_COARSE, RES_FINE = (2001, 401), (4001, 801)


# ---------------------------------------------------------------------------
# trilinear lookup
# ---------------------------------------------------------------------------
def taps(res_zyx, q):
    """The 8 texels and weights of the lookup at q, (n, 3) points (x, y, z) of [0, 1]^3:
    flat indices into the [z, y, x] array and float64 weights, both (n, 8)."""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    res = np.array([res_zyx[2], res_zyx[1], res_zyx[0]])          # (x, y, z)
    p = q * res - 0.5
    i0 = np.floor(p).astype(np.int64)
    w1 = p - i0
    w0 = 1.0 - w1
    lo, hi = np.clip(i0, 0, res - 1), np.clip(i0 + 1, 0, res - 1)
    idx = np.empty((q.shape[0], 8), np.int64)
    wgt = np.empty((q.shape[0], 8), np.float64)
    for c in range(8):
        b = (c & 1, (c >> 1) & 1, c >> 2)
        ix, iy, iz = ((hi if b[k] else lo)[:, k] for k in range(3))
        idx[:, c] = (iz * res[1] + iy) * res[0] + ix
        wgt[:, c] = np.prod([(w1 if b[k] else w0)[:, k] for k in range(3)], axis=0)
    return idx, wgt


def tri(grid, q):
    """float64 trilinear lookup of grid[z, y, x] at the points q of [0, 1]^3"""
    g = np.asarray(grid, np.float64)
    idx, wgt = taps(g.shape[:3], q)
    return (g.reshape(-1)[idx] * wgt).sum(-1)


# ---------------------------------------------------------------------------
# geometry, read from the scene dictionary
# ---------------------------------------------------------------------------
def _matrix(t):
    return np.eye(4) if t is None else np.asarray(t.matrix, np.float64)


def _slab(o, d, lo=-1.0, hi=1.0):
    """entry and exit distance of o + t d against the cube [lo, hi]^3"""
    t0, t1 = -np.inf, np.inf
    for k in range(3):
        if d[k] == 0.0:
            assert lo < o[k] < hi
            continue
        a, b = (lo - o[k]) / d[k], (hi - o[k]) / d[k]
        t0, t1 = max(t0, min(a, b)), min(t1, max(a, b))
    return t0, t1


RAY_EPSILON = 1500.0 * 2.0 ** -24      # math::RayEpsilon<float>


def _ray_gap(p, d):
    """A ray that crosses the cube's null boundary at p is spawned again from p moved along the face normal by
    (1 + max |p|) RayEpsilon (Interaction::offset_p, interaction.h:158-162), and the medium is tracked from there:
    the first `gap` of the way inside the cube attenuates nothing and scatters nothing.  p lies on one face of the
    axis-aligned cube, so the normal is the axis of p's largest coordinate."""
    p = np.asarray(p, np.float64)
    k = int(np.argmax(np.abs(p)))
    return (1.0 + np.abs(p).max()) * RAY_EPSILON / abs(d[k])


class Geometry:
    """What the closed forms need of a volume_cube dictionary (the cube is [-1, 1]^3: it has no to_world)."""

    def __init__(self, d):
        assert "to_world" not in d["cube"] and "sky" not in d
        cam = _matrix(d["sensor"]["to_world"])
        self.origin = cam[:3, 3].copy()
        self.axis = cam[:3, :3] @ np.array([0.0, 0.0, 1.0])
        self.axis /= np.linalg.norm(self.axis)
        t0, t1 = _slab(self.origin, self.axis)
        assert 0.0 < t0 < t1, "the camera looks at the cube from outside"
        self.t_in, self.length = t0, t1 - t0
        self.u0 = _ray_gap(self.cam(np.array(0.0)), self.axis)
        sd = np.asarray(d["sun"]["direction"], np.float64)
        self.w = -sd / np.linalg.norm(sd)                            # towards the sun
        self.E = float(np.mean(d["sun"]["irradiance"]["value"]))
        med = d["medium1"]
        self.scale = float(med["scale"])
        self.albedo = float(np.mean(med["albedo"]))
        self.hom = med["type"] == "homogeneous"
        if self.hom:
            self.sigma_t, self.grid, self.to_local = float(med["sigma_t"]), None, None
        else:
            self.grid = np.asarray(med["sigma_t"]["data"], np.float64)
            self.grid = self.grid.reshape(self.grid.shape[:3])
            self.to_local = np.linalg.inv(_matrix(med["sigma_t"].get("to_world")))
        ph = med["phase"]
        if ph["type"] == "isotropic":
            self.f = 1.0 / (4.0 * np.pi)
        else:
            # eval_hg(g, dot(wo, wi)) with wi = -ray.d and wo = w (hg.cpp:66-104)
            g, c = float(ph["g"]), float(np.dot(self.w, -self.axis))
            self.f = (1.0 - g * g) / (4.0 * np.pi * (1.0 + g * g + 2.0 * g * c) ** 1.5)
        self.wall = None
        if "wall" in d:
            m = _matrix(d["wall"]["to_world"])
            n = np.linalg.inv(m).T[:3, :3] @ np.array([0.0, 0.0, 1.0])
            n /= np.linalg.norm(n)
            t = np.dot(m[:3, 3] - self.origin, n) / np.dot(self.axis, n)
            p = self.origin + t * self.axis
            loc = np.linalg.inv(m) @ np.append(p, 1.0)
            assert t > self.t_in + self.length, "the wall lies behind the cube"
            assert abs(loc[0]) < 1.0 and abs(loc[1]) < 1.0, "the axis meets the rectangle"
            assert np.dot(n, -self.axis) > 0.0 and np.dot(n, self.w) > 0.0, "seen and lit from its front"
            s0, s1 = _slab(p, self.w)
            assert 0.0 < s0 < s1, "the wall's shadow ray crosses the cube"
            enter, leave = p + s0 * self.w, p + s1 * self.w
            assert np.abs(enter[:2] - leave[:2]).max() > 0.25, "... obliquely"
            self.wall = dict(p=p, cos=float(np.dot(n, self.w)), s0=s0 + _ray_gap(enter, self.w), s1=s1,
                             rho=float(np.mean(d["wall"]["bsdf"]["reflectance"]["value"])))

    def cam(self, u):
        return self.origin + (self.t_in + np.asarray(u, np.float64))[..., None] * self.axis

    def sun_exit(self, x):
        """l: the distance from the points x inside the cube along w to its boundary"""
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(self.w != 0.0, (np.sign(self.w) - x) / self.w, np.inf)
        return np.maximum(t.min(-1), 0.0)

    def local(self, x):
        x = np.asarray(x, np.float64)
        return x @ self.to_local[:3, :3].T + self.to_local[:3, 3]


def _trapezoid_weights(n, length):
    w = np.full(n, length / (n - 1))
    w[0] *= 0.5
    w[-1] *= 0.5
    return w


# ---------------------------------------------------------------------------
# homogeneous: the one-dimensional forms
# ---------------------------------------------------------------------------
def _hom_single(geo, n_u):
    u = np.linspace(geo.u0, geo.length, n_u)
    d = (u - geo.u0) + geo.sun_exit(geo.cam(u))       # camera-ward and sun-ward way through the medium
    S = geo.scale * geo.sigma_t
    k = geo.E * geo.albedo * geo.f
    L = k * np.trapezoid(S * np.exp(-S * d), u)
    dS = geo.scale * k * np.trapezoid((1.0 - S * d) * np.exp(-S * d), u)
    return L, dS


# ---------------------------------------------------------------------------
# heterogeneous: L and the per-texel gradient field
# ---------------------------------------------------------------------------
def _line_field(geo, p0, p1, n):
    """int tri(grid, .) and the per-texel int w_t along the segment p0 -> p1 (n trapezoid nodes)"""
    s = np.linspace(0.0, 1.0, n)
    idx, wgt = taps(geo.grid.shape, geo.local(p0 + s[:, None] * (p1 - p0)))
    q = _trapezoid_weights(n, float(np.linalg.norm(p1 - p0)))
    field = np.bincount(idx.ravel(), (wgt * q[:, None]).ravel(), minlength=geo.grid.size)
    return float(field @ geo.grid.ravel()), field


def _het_single(geo, n_u, n_s, chunk=128):
    n_tex, flat = geo.grid.size, geo.grid.ravel()
    u = np.linspace(geo.u0, geo.length, n_u)
    h = (geo.length - geo.u0) / (n_u - 1)
    qu = _trapezoid_weights(n_u, geo.length - geo.u0)
    x = geo.cam(u)
    l = geo.sun_exit(x)
    ci, cw = taps(geo.grid.shape, geo.local(x))
    dens = (flat[ci] * cw).sum(-1)                                        # tri(grid, x(u))
    cum = np.concatenate([[0.0], np.cumsum(0.5 * h * (dens[1:] + dens[:-1]))])   # int_0^u tri dcam
    # pass 1: the sun-ward integrals, T and L
    s = np.linspace(0.0, 1.0, n_s)
    qs = _trapezoid_weights(n_s, 1.0)
    sun = np.empty(n_u)
    for b in range(0, n_u, chunk):
        e = min(n_u, b + chunk)
        pts = x[b:e, None, :] + (s[None, :, None] * l[b:e, None, None]) * geo.w
        si, sw = taps(geo.grid.shape, geo.local(pts.reshape(-1, 3)))
        v = (flat[si] * sw).sum(-1).reshape(e - b, n_s)
        sun[b:e] = (v * qs).sum(-1) * l[b:e]
    T = np.exp(-geo.scale * (cum + sun))
    k = geo.E * geo.albedo * geo.f
    L = k * np.sum(qu * geo.scale * dens * T)
    # pass 2: the field.  A_u = q_u sigma(x(u)) T(u) multiplies both inner integrals
    A = qu * geo.scale * dens * T
    R = np.concatenate([np.cumsum(A[::-1])[::-1][1:], [0.0]])            # sum_{k > v} A_k
    c = h * R + 0.5 * h * A                                                # cumulative trapezoid, sums swapped
    c[0] = 0.5 * h * R[0]
    G = np.bincount(ci.ravel(), (cw * (qu * T - c)[:, None]).ravel(), minlength=n_tex)
    for b in range(0, n_u, chunk):
        e = min(n_u, b + chunk)
        pts = x[b:e, None, :] + (s[None, :, None] * l[b:e, None, None]) * geo.w
        si, sw = taps(geo.grid.shape, geo.local(pts.reshape(-1, 3)))
        coef = (A[b:e, None] * l[b:e, None] * qs[None, :]).reshape(-1)
        G -= np.bincount(si.ravel(), (sw * coef[:, None]).ravel(), minlength=n_tex)
    return L, (k * geo.scale * G).reshape(geo.grid.shape)


# ---------------------------------------------------------------------------
# scene C: transmittance only
# ---------------------------------------------------------------------------
def _wall(geo, n):
    wl = geo.wall
    a0, a1 = geo.cam(np.array(geo.u0)), geo.cam(np.array(geo.length))
    b0, b1 = wl["p"] + wl["s0"] * geo.w, wl["p"] + wl["s1"] * geo.w
    k = wl["rho"] / np.pi * geo.E * wl["cos"]
    if geo.hom:
        dist = (geo.length - geo.u0) + (wl["s1"] - wl["s0"])
        L = k * np.exp(-geo.scale * geo.sigma_t * dist)
        return L, -geo.scale * dist * L
    (tc, fc), (ts, fs) = _line_field(geo, a0, a1, n), _line_field(geo, b0, b1, n)
    L = k * np.exp(-geo.scale * (tc + ts))
    return L, (-geo.scale * L * (fc + fs)).reshape(geo.grid.shape)


class Reference:
    """L and the sigma_t derivative (a scalar when homogeneous, else the per-texel field) at one resolution"""

    def __init__(self, geo, res):
        self.geo = geo
        if geo.wall is not None:
            self.L, self.dsigma = _wall(geo, res[0])
        elif geo.hom:
            self.L, self.dsigma = _hom_single(geo, res[0])
        else:
            self.L, self.dsigma = _het_single(geo, *res)

    def d_mask(self, mask=None):
        if self.geo.hom:
            return float(self.dsigma)
        return float((self.dsigma * (1.0 if mask is None else np.asarray(mask, np.float64))).sum())

    def d_albedo(self):
        return self.L / self.geo.albedo


def references(d):
    """(coarse, fine) References of a scene dictionary"""
    geo = Geometry(d)
    return Reference(geo, RES_COARSE), Reference(geo, RES_FINE)


# ---------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------
def _mi():
    import mitsuba_hip as mi
    return mi


def _cube(**kw):
    mi = _mi()
    d = mi.volume_cube(W, H, SPP, albedo=kw.pop("albedo", ALBEDO), sun=SUN, max_depth=2, rr_depth=100, fov=FOV, **kw)
    del d["sky"]
    d["integrator"] = {"type": "prbvolpath", "max_depth": 2, "rr_depth": 100}
    return d


def _headroom(g):
    """The majorant is put 0.2 above the data, in the far bottom corner texel that neither the axis nor a sun-ward
    ray from it reads (as test_prbvolpath_oracle.py does).  Delta tracking's derivative of a null collision is
    -1 / sigma_n, met with probability sigma_n / majorant: where the density touches the majorant its variance
    diverges logarithmically, the standard error of 16 seeds means nothing and a z-test cannot be made."""
    g[0, 0, 0] = g.max() + 0.2
    return g


def random_grid(res_zyx=(6, 8, 7), seed=21):
    return _headroom(np.random.default_rng(seed).uniform(0.3, 1.0, res_zyx).astype(np.float32))


def fbm8():
    return _headroom(np.ascontiguousarray(_mi().fbm_grid(8), np.float32).reshape(8, 8, 8).copy())


def _with_wall(d, sun_dir):
    T = _mi().Transform4f
    d["sun"]["direction"] = list(sun_dir)
    d["wall"] = {"type": "rectangle", "to_world": T.translate([0.0, 0.0, -1.5]) @ T.scale([2.0, 2.0, 1.0]),
                 "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.6, 0.6, 0.6]}}}
    return d


WALL_SUN = (0.0, -0.3, -1.0)


def scene_dict(name, grid=None, sigma_t=None):
    """The dictionary of case `name`; `grid` / `sigma_t` replace the case's own (the update tests)."""
    if name in HOM_CASES:
        c = dict(HOM_CASES[name])
        if sigma_t is not None:
            c["sigma_t"] = sigma_t
        return _cube(medium_type="homogeneous", **c)
    if name in HET_CASES:
        g = grid if grid is not None else HET_CASES[name]["grid"]()
        return _cube(grid=g, scale=HET_CASES[name]["scale"], g=0.5)
    if name == "wall_hom":
        return _with_wall(_cube(medium_type="homogeneous", sigma_t=sigma_t or 0.6, scale=1.5, albedo=0.0, g=0.5), WALL_SUN)
    if name == "wall_het":
        g = grid if grid is not None else random_grid()
        return _with_wall(_cube(grid=g, scale=1.5, albedo=0.0, g=0.5), WALL_SUN)
    raise KeyError(name)


# A: homogeneous.  S = scale * sigma_t stays away from the derivative's zero crossing near 0.7
HOM_CASES = {
    "hom_thin": dict(sigma_t=0.3, scale=1.0, g=0.5),
    "hom_thick": dict(sigma_t=2.0, scale=1.0, g=0.5),
    "hom_scaled": dict(sigma_t=0.4, scale=2.5, g=0.5),
    "hom_isotropic": dict(sigma_t=0.3, scale=1.0, g=0.0),
}
# B: heterogeneous
HET_CASES = {
    "het_random_6x8x7": dict(grid=random_grid, scale=1.5),
    "het_fbm_8": dict(grid=fbm8, scale=1.5, near=1),
}
WALL_CASES = ("wall_hom", "wall_het")


def sun_only_mask(res_zyx):
    """Texels at least one texel above the axis' own (the sun stands towards +y): their trilinear support does not
    touch the camera axis, so only the shadow rays' term of the derivative survives."""
    rz, ry, rx = res_zyx
    m = np.zeros(res_zyx, np.float32)
    j = np.arange(ry)
    m[:, (j - 0.5) / ry > 0.5 + 1.0 / ry, :] = 1.0
    return m


def masks(res_zyx, near=2):
    """name -> 0/1 mask of the grid's shape (z, y, x).  The camera looks down -z from +z, so the near face is the
    last z slab; the axis passes texels (ry / 2 - 1, ry / 2) x (rx / 2 ...).  `near`: the z slabs of the near-face
    block.  The fBm grid takes one: its last two cancel (+4.8e-3 - 1.5e-3), which leaves their sum with a standard
    error of 1.16 % at these sizes, above the cap; the single-texel mask is the extreme of the same thing."""
    rz, ry, rx = res_zyx
    out = {"ones": np.ones(res_zyx, np.float32)}
    m = np.zeros(res_zyx, np.float32)
    m[1:rz - 1, ry // 2 - 1:ry // 2 + 1, (rx - 1) // 2 - 1:rx // 2 + 2] = 1.0
    out["axis_block"] = m
    m = np.zeros(res_zyx, np.float32)
    m[rz - near:] = 1.0
    out["near_slabs"] = m
    m = np.zeros(res_zyx, np.float32)
    m[:2] = 1.0
    out["far_slabs"] = m
    out["sun_only"] = sun_only_mask(res_zyx)
    rng = np.random.default_rng(77)
    for i in range(6):
        out[f"random{i}"] = (rng.random(res_zyx) < 0.5).astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def case_references(name):
    """(coarse, fine) of the case's own dictionary, computed once per process"""
    return references(scene_dict(name))


def quantities(name):
    """[(label, key, mask or None, coarse value, fine value)] of a case: what its backward pass is held to"""
    lo, hi = case_references(name)
    if name in HOM_CASES:
        return [("sigma_t", "medium1.sigma_t.value", None, lo.d_mask(), hi.d_mask()),
                ("albedo", "medium1.albedo.value", None, lo.d_albedo(), hi.d_albedo())]
    if name == "wall_hom":
        return [("sigma_t", "medium1.sigma_t.value", None, lo.d_mask(), hi.d_mask())]
    near = HET_CASES.get(name, {}).get("near", 2)
    return [(k, "medium1.sigma_t.data", m, lo.d_mask(m), hi.d_mask(m))
            for k, m in masks(hi.geo.grid.shape, near).items()]


ALL_CASES = tuple(HOM_CASES) + tuple(HET_CASES) + WALL_CASES


def z_row(case, label, ref, samples):
    """mean, SE and z of the per-seed values against the quadrature, and the printed table row"""
    x = np.asarray(samples, np.float64)
    mean, se = x.mean(), x.std(ddof=1) / np.sqrt(x.size)
    z = (mean - ref) / se if se > 0 else (0.0 if mean == ref else np.inf)
    row = f"{case:18s} {label:11s} quadrature {ref:+.6e} mean {mean:+.6e} SE/|ref| {se / abs(ref):.4%} z {z:+.2f}"
    return mean, se, z, row


# ---------------------------------------------------------------------------
# after params.update(): the value of hom_thin becomes hom_thick's, the random grid another one
# ---------------------------------------------------------------------------
UPDATED_VALUE = ("hom_thin", "hom_thick")
assert HOM_CASES["hom_thick"] == dict(HOM_CASES["hom_thin"], sigma_t=2.0)
UPDATED_GRID = "het_random_6x8x7"


def updated_grid():
    g = random_grid(seed=22)
    g[0, 0, 0] += 0.3               # the majorant moves with the update
    assert g.max() != random_grid().max()
    return g


@functools.lru_cache(maxsize=None)
def updated_grid_quantities():
    g = updated_grid()
    lo, hi = references(scene_dict(UPDATED_GRID, grid=g))
    m = masks(g.shape)
    return [(k, "medium1.sigma_t.data", m[k], lo.d_mask(m[k]), hi.d_mask(m[k])) for k in ("ones", "sun_only", "random0")]
