"""Adversarial scenes and rays for the traversal engines (a plain helper, no
fixtures): the cases where a slab test, a triangle test or a tie rule goes
wrong while random rays in a unit room never notice.

Scenes are lists of shape specs for `scene_dict` (scene order = list order);
ray classes return (7, n) float32 arrays in the mh_trace_* layout (origin,
direction, maxt as planes).  Everything is deterministic: fixed seeds, and
every value is rounded to float32 here, so the oracle, the float64 reference
and the device read the same numbers.

  A  axis-aligned: zero, negative-zero and tiny direction components
  B  far origin: aimed at vertices / edge midpoints / centroids from D = 5, 50
  C  in-plane: rays in, starting on and grazing a flat grid
  D  maxt edges: maxt = t and maxt = nextafter(t, 0) of a known hit
  E  ties: coincident surfaces and zero-area triangles
"""
import numpy as np

N_RAYS = 1 << 13
SPHERE_R = 0.01
INF = np.float32(np.inf)
# direction components of class A: the slab test's reciprocal switches to a
# substitute at |d| <= 2^-80, so both sides of that threshold, zero with both
# signs, and a value whose reciprocal (1e30) is near the top of the range
TINY = [0.0, -0.0, 2.0 ** -81, -2.0 ** -81, 2.0 ** -80, -2.0 ** -80, 2.0 ** -79, -2.0 ** -79, 1e-30, -1e-30]


# ---------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------
def _mesh(V, F):
    return {"type": "mesh", "vertex_positions": np.asarray(V, np.float32), "faces": np.asarray(F, np.uint32)}


def tiny_sphere(m, extra=0):
    """UV sphere, R = 0.01, centred on the origin: 4 m^2 triangle records
    (m = 12: 576, m = 4: 64; the pole rows are zero-area triangles, kept as
    records).  The seam column repeats the first column's vertices exactly.
    extra = 1 appends one free-standing triangle (64 -> 65 primitives)."""
    th = np.linspace(0, np.pi, m + 1)
    ph = np.linspace(0, 2 * np.pi, 2 * m + 1)
    T_, P_ = np.meshgrid(th, ph, indexing="ij")
    V = SPHERE_R * np.stack([np.sin(T_) * np.cos(P_), np.cos(T_), np.sin(T_) * np.sin(P_)], -1)
    V[0] = [0, SPHERE_R, 0]
    V[-1] = [0, -SPHERE_R, 0]
    V[:, -1] = V[:, 0]
    V = V.reshape(-1, 3)
    a = (np.arange(m)[:, None] * (2 * m + 1) + np.arange(2 * m)[None, :]).reshape(-1)
    # outward normals (the render leg lights the sphere from outside)
    F = np.concatenate([np.stack([a, a + 1, a + 2 * m + 1], 1), np.stack([a + 1, a + 2 * m + 2, a + 2 * m + 1], 1)])
    if extra:
        k = len(V)
        V = np.concatenate([V, [[0.03, -0.004, -0.003], [0.03, 0.005, -0.002], [0.03, 0.001, 0.006]]])
        F = np.concatenate([F, [[k, k + 1, k + 2]]])
    return [_mesh(V, F)]


def flat_grid(n, z):
    """n x n quads (2 n^2 triangles) on [-0.5, 0.5]^2 in the plane `z`: every
    box of the BVH has zero extent along z."""
    c = np.linspace(-0.5, 0.5, n + 1)
    X, Y = np.meshgrid(c, c, indexing="ij")
    V = np.stack([X, Y, np.full_like(X, z)], -1).reshape(-1, 3)
    a = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).reshape(-1)
    F = np.concatenate([np.stack([a, a + n + 1, a + 1], 1), np.stack([a + 1, a + n + 1, a + n + 2], 1)])
    return [_mesh(V, F)]


# the zero-area mesh of ties(): triangles 0-1 are sound (the unit-ish quad on
# [0.625, 0.875] x [-0.125, 0.125]); 2-3 repeat a vertex, 4-5 have collinear
# vertices, all inside or on the edges of the sound ones
DEGENERATE_PRIMS = (2, 3, 4, 5)


def ties(n=1):
    """Shape 0 and shape 2: the same n x n quad grid on [-0.5, 0.5]^2, z = 0,
    twice (bit-identical records: the lower shape must win every ray).
    Shape 1: a rectangle on the same square (same plane; its own t formula).
    Shape 3: two sound triangles and four zero-area ones that share their
    vertices; the zero-area ones must never be reported."""
    import mitsuba_hip as mi
    g = flat_grid(n, 0.0)[0]
    # dyadic coordinates: the collinear triples are collinear in float32 too
    V = np.array([[0.625, -0.125, 0], [0.875, -0.125, 0], [0.625, 0.125, 0], [0.875, 0.125, 0], [0.75, 0.0, 0],
                  [0.75, -0.125, 0]])
    F = np.array([[0, 1, 2], [2, 1, 3],        # sound
                  [0, 0, 3], [1, 4, 4],        # repeated vertex
                  [0, 4, 3], [0, 5, 1]])       # collinear: the diagonal 0-4-3, the edge 0-5-1
    rect = {"type": "rectangle", "to_world": mi.Transform4f.scale([0.5, 0.5, 1.0])}
    return [g, rect, dict(g), _mesh(V, F)]


def scene_dict(shapes, distance=None, fov=None, max_depth=2, spp=8, res=24):
    """The scene of `shapes` in list order.  distance / fov: a perspective
    camera on the +z axis looking at the origin, and a constant emitter (the
    render leg); otherwise a default camera nobody uses (the trace legs)."""
    import mitsuba_hip as mi
    d = {"type": "scene", "integrator": {"type": "path", "max_depth": max_depth},
         "white": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.8, 0.7, 0.6]}}}
    sensor = {"type": "perspective", "near_clip": 0.001, "far_clip": 1000.0,
              "sampler": {"type": "independent", "sample_count": spp},
              "film": {"type": "hdrfilm", "width": res, "height": res, "rfilter": {"type": "gaussian"},
                       "pixel_format": "rgb", "component_format": "float32"}}
    if distance is not None:
        sensor.update(fov=fov, fov_axis="x",
                      to_world=mi.Transform4f.look_at(origin=[0, 0, distance], target=[0, 0, 0], up=[0, 1, 0]))
        d["sky"] = {"type": "constant", "radiance": {"type": "rgb", "value": [1.0, 0.9, 0.8]}}
    d["sensor"] = sensor
    for i, s in enumerate(shapes):
        s = dict(s)
        s["bsdf"] = {"type": "ref", "id": "white"}
        d[f"shape{i:02d}"] = s
    return d


def load(shapes, **kw):
    import mitsuba_hip as mi
    mi.set_variant("hip_ad_rgb")
    return mi.load_dict(scene_dict(shapes, **kw))


def mesh_arrays(shapes, i=0):
    """float32 vertices and faces of mesh shape i, as the scene stores them."""
    return np.asarray(shapes[i]["vertex_positions"], np.float32), np.asarray(shapes[i]["faces"], np.int64)


# ---------------------------------------------------------------------------
# rays
# ---------------------------------------------------------------------------
def pack(o, d, maxt=None):
    n = o.shape[0]
    m = np.full(n, INF, np.float32) if maxt is None else np.asarray(maxt, np.float32)
    return np.ascontiguousarray(np.concatenate([np.asarray(o, np.float32).T, np.asarray(d, np.float32).T, m[None]], 0))


def with_maxt(rays, maxt):
    r = rays.copy()
    r[6] = np.asarray(maxt, np.float32)
    return r


def _unit(rng, n):
    w = rng.normal(size=(n, 3))
    return w / np.linalg.norm(w, axis=1, keepdims=True)


def _sound(V, F):
    """faces with a non-zero area"""
    V = V.astype(np.float64)
    ar = np.linalg.norm(np.cross(V[F[:, 1]] - V[F[:, 0]], V[F[:, 2]] - V[F[:, 0]]), axis=1)
    return F[ar > 0]


def surface_points(V, F, n, rng, lo=0.15):
    """points inside sound triangles, every barycentric coordinate >= lo"""
    F = _sound(V, F)
    f = F[rng.integers(0, len(F), n)]
    b = rng.dirichlet([1.0, 1.0, 1.0], n) * (1 - 3 * lo) + lo
    P = V.astype(np.float64)
    return b[:, :1] * P[f[:, 0]] + b[:, 1:2] * P[f[:, 1]] + b[:, 2:] * P[f[:, 2]]


def rays_A(V, F, n=N_RAYS, seed=11, flat=None):
    """Axis-aligned rays through a mesh: one or two direction components from
    TINY, the others a random unit vector.  Each ray is laid through a point of
    the surface, so the tiny components' coordinates are the point's (inside
    the slabs); a quarter has one of them moved outside the mesh's bounds, and
    one ray in 16 has it equal to a vertex coordinate instead.  flat: the axis
    a flat mesh has no extent on; only one ray in 20 gets its tiny component
    there (a ray in the mesh's plane is class C's subject)."""
    rng = np.random.default_rng(seed)
    p = surface_points(V, F, n, rng)
    d = _unit(rng, n)
    ext = float(np.abs(V).max())
    two = rng.random(n) < 0.4
    ax0 = rng.integers(0, 3, n)
    ax1 = (ax0 + 1 + rng.integers(0, 2, n)) % 3
    if flat is not None:
        ax0 = (flat + 1 + rng.integers(0, 2, n)) % 3
        ax1 = 3 - flat - ax0
        inplane = rng.random(n) < 0.05
        ax0[inplane], two[inplane] = flat, False
    tiny = np.array(TINY)
    d[np.arange(n), ax0] = 0.0
    d[two, ax1[two]] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = p - d * rng.uniform(2.0, 6.0, (n, 1)) * ext
    d[np.arange(n), ax0] = tiny[rng.integers(0, len(tiny), n)]
    d[two, ax1[two]] = tiny[rng.integers(0, len(tiny), two.sum())]
    kind = rng.random(n)
    out = kind < 0.25
    o[out, ax0[out]] = np.where(rng.random(out.sum()) < 0.5, -1, 1) * rng.uniform(1.5, 4.0, out.sum()) * ext
    vtx = (kind >= 0.25) & (kind < 0.25 + 1.0 / 16)
    o[vtx, ax0[vtx]] = V[rng.integers(0, len(V), vtx.sum()), ax0[vtx]]
    return pack(o, d)


def targets_B(V, F, kind):
    """what class B aims at: the distinct vertices, the edge midpoints or the
    centroids of the sound triangles"""
    F = _sound(V, F)
    P = V.astype(np.float64)
    if kind == "vertex":
        return np.unique(P[np.unique(F)], axis=0)
    if kind == "edge":
        e = np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]])
        return np.unique(0.5 * (P[e[:, 0]] + P[e[:, 1]]), axis=0)
    return (P[F[:, 0]] + P[F[:, 1]] + P[F[:, 2]]) / 3.0


def rays_B(V, F, kind, D, n=N_RAYS, seed=12):
    """Far origin: from distance D in a random direction, aimed at a target
    of targets_B.  The origin's coordinates are ~D, so one ulp of the origin
    is D * 2^-23 in world units -- 6e-6 at D = 50, against triangles of 1e-3."""
    rng = np.random.default_rng(seed + int(D))
    tg = targets_B(V, F, kind)
    p = tg[rng.integers(0, len(tg), n)]
    # from the target's own side of the (convex, origin-centred) mesh, so the
    # target is the first surface the ray meets, and not at a grazing angle
    w, out = _unit(rng, n), p / np.linalg.norm(p, axis=1, keepdims=True)
    w *= np.where((w * out).sum(1) < 0, -1.0, 1.0)[:, None]
    low = (w * out).sum(1) < 0.6
    w[low] = (w[low] + out[low]) / np.linalg.norm(w[low] + out[low], axis=1, keepdims=True)
    o = (p + D * w).astype(np.float32).astype(np.float64)
    d = p - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return pack(o, d)


def rays_generic(V, F, n=N_RAYS, seed=14, near=0.5, far=40.0):
    """plain rays through interior points of the surface from `near`..`far`
    mesh sizes away (the base of classes C off-plane and D)"""
    rng = np.random.default_rng(seed)
    p = surface_points(V, F, n, rng)
    ext = float(np.abs(V).max())
    o = (p + _unit(rng, n) * rng.uniform(near, far, (n, 1)) * ext).astype(np.float32).astype(np.float64)
    d = p - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return pack(o, d)


def rays_C(z, part, n=N_RAYS, seed=13):
    """Against flat_grid(., z), the grid on [-0.5, 0.5]^2:
    in     d.z == 0 and o.z == z: the determinant of every triangle is 0, a miss
    on     origin exactly on the plane, d.z != 0: t == 0 is a hit
    graze  |d.z| = 1e-6, from a height that puts the hit 0.05..0.6 away
    off    plain oblique rays onto the plane (the comfortable share)"""
    rng = np.random.default_rng(seed + {"in": 0, "on": 1, "graze": 2, "off": 3}[part])
    zf = float(np.float32(z))
    xy = rng.uniform(-0.47, 0.47, (n, 2))
    if part == "in":
        o = np.concatenate([rng.uniform(-0.8, 0.8, (n, 2)), np.full((n, 1), zf)], 1)
        a = rng.uniform(0, 2 * np.pi, n)
        d = np.stack([np.cos(a), np.sin(a), np.zeros(n)], 1)
        d[::2, 2] = -0.0
        return pack(o, d)
    if part == "on":
        o = np.concatenate([xy, np.full((n, 1), zf)], 1)
        d = _unit(rng, n)
        d[np.abs(d[:, 2]) < 0.05, 2] = 0.5
        return pack(o, d)
    if part == "graze":
        a = rng.uniform(0, 2 * np.pi, n)
        s = np.where(rng.random(n) < 0.5, -1.0, 1.0)
        d = np.stack([np.cos(a), np.sin(a), -s * 1e-6], 1).astype(np.float32).astype(np.float64)
        t = rng.uniform(0.05, 0.6, n)
        # the height as the float32 origin will hold it: o.z - z is then exact
        oz = (zf + s * t * 1e-6).astype(np.float32).astype(np.float64)
        t = (oz - zf) / -d[:, 2]
        o = np.concatenate([xy - d[:, :2] * t[:, None], oz[:, None]], 1)
        return pack(o, d)
    p = np.concatenate([xy, np.full((n, 1), zf)], 1)
    w = _unit(rng, n)
    w[np.abs(w[:, 2]) < 0.1, 2] = 0.6
    o = (p + w * rng.uniform(0.1, 2.0, (n, 1))).astype(np.float32).astype(np.float64)
    d = p - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return pack(o, d)


def rays_E(n=N_RAYS, seed=15):
    """Through the coincident surfaces of ties(), z = 0: a third straight down
    or up (two zero direction components), the rest oblique, from both sides;
    aimed at [-0.55, 0.95] x [-0.2, 0.2] and the whole square, so the sound
    and the zero-area triangles of shape 3 are crossed as well."""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(-0.55, 0.95, n), rng.uniform(-0.55, 0.55, n), np.zeros(n)], 1)
    band = rng.random(n) < 0.3
    p[band, 1] = rng.uniform(-0.2, 0.2, band.sum())
    w = _unit(rng, n)
    w[np.abs(w[:, 2]) < 0.1, 2] = 0.7
    w[: n // 3] = [0, 0, 1]
    w[: n // 6] = [0, 0, -1]
    o = (p + w * rng.uniform(0.1, 1.5, (n, 1))).astype(np.float32).astype(np.float64)
    d = -w
    d[n // 3:] = p[n // 3:] - o[n // 3:]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return pack(o, d)
