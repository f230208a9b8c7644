"""Medium topologies beyond the one axis-aligned cube of
`mitsuba_hip.scenes.volume_cube`, shared by the CPU property
tests of the oracle (test_vol_topologies_oracle.py) and the device-against-
oracle tests (test_gpu_vol_topologies.py).  A plain helper module.

CASES maps a name to `f(mi, integrator, w=24, h=20, spp=8) -> scene dict`.
Every scene starts from volume_cube(w, h, spp, grid=fbm_grid(16), scale=4,
max_depth=6) and carries the floor of the parity tests' scenes unless its
entry says otherwise.  KEYS lists each case's differentiable parameters:
every medium's sigma_t and albedo and the floor's (or the inner object's)
reflectance.

Every boundary face stays at least 0.05 away from every other shape's faces
and from the floor, so that the BVH and the oracle's brute-force loop meet no
more equal-distance hits than on the base scene.
"""
import numpy as np

from phase_cases import TABLES

FLOOR_KEY = "floor.bsdf.reflectance.value"


def floor(mi, y=-1.2):
    """The diffuse floor below the cube (the parity tests' _pvp_scene / _vol_floor_scene)."""
    T = mi.Transform4f
    return {"type": "rectangle",
            "to_world": T.translate([0, y, 0]) @ T.rotate([1, 0, 0], -90) @ T.scale([3, 3, 3]),
            "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.6, 0.5, 0.4]}}}


def unit_grid_to_world(mi):
    """[0, 1]^3 -> [-1, 1]^3: volume_cube's grid placement."""
    T = mi.Transform4f
    return T.translate([-1.0, -1.0, -1.0]) @ T.scale([2.0, 2.0, 2.0])


def base(mi, integrator, w=24, h=20, spp=8, with_floor=True, **kw):
    kw.setdefault("grid", mi.fbm_grid(16))
    kw.setdefault("scale", 4.0)
    kw.setdefault("max_depth", 6)
    d = mi.volume_cube(w, h, spp, **kw)
    d["integrator"] = {"type": integrator, "max_depth": kw["max_depth"], "rr_depth": kw.get("rr_depth", 5)}
    if with_floor:
        d["floor"] = floor(mi)
    return d


def crop_795(mi):
    """The dense centre of the 16^3 fBm cube, numpy shape (7, 9, 5) -- as
    test_prbvolpath_grid_corner_scatter crops it."""
    o = [(16 - n) // 2 for n in (7, 9, 5)]
    return np.ascontiguousarray(mi.fbm_grid(16)[o[0]:o[0] + 7, o[1]:o[1] + 9, o[2]:o[2] + 5])


def three_media(mi, integrator, w=24, h=20, spp=8, **kw):
    """medium1: the cube and its grid moved together by a rotation and a
    non-uniform scale (a general affine grid_to_local).  medium2: a second
    cube at x = +0.9 whose grid box lies strictly inside it (grid_offset,
    corner offset and bitmap slot of a second grid; bbox != shape).  medium3:
    a small homogeneous cube above (vol_flags of both medium types at once).
    x extents: cube 1 [-1.79, -0.01], cube 2 [0.3, 1.5]; cube 3 y >= 1.0 over
    the others' y <= 0.9."""
    T = mi.Transform4f
    d = base(mi, integrator, w, h, spp, **kw)
    M1 = T.translate([-0.9, 0.0, 0.0]) @ T.rotate([0, 1, 0], 25) @ T.scale([0.7, 0.9, 0.6])
    d["medium1"]["sigma_t"]["to_world"] = M1 @ unit_grid_to_world(mi)
    d["cube"]["to_world"] = M1
    d["medium2"] = {"type": "heterogeneous",
                    "sigma_t": {"type": "gridvolume", "data": crop_795(mi),
                                "to_world": T.translate([0.45, -0.5, -0.4]) @ T.scale([0.8, 0.9, 0.7])},
                    "scale": 6.0, "albedo": [0.9, 0.6, 0.3], "phase": {"type": "isotropic"}}
    d["cube2"] = {"type": "cube", "to_world": T.translate([0.9, 0.0, 0.0]) @ T.scale([0.6, 0.6, 0.6]),
                  "bsdf": {"type": "null"}, "interior": {"type": "ref", "id": "medium2"}}
    d["medium3"] = {"type": "homogeneous", "sigma_t": 0.8, "scale": 1.5, "albedo": 0.7,
                    "phase": {"type": "hg", "g": 0.3}}
    d["cube3"] = {"type": "cube", "to_world": T.translate([0.2, 1.3, 0.0]) @ T.scale([0.3, 0.3, 0.3]),
                  "bsdf": {"type": "null"}, "interior": {"type": "ref", "id": "medium3"}}
    return d


def camera_inside(mi, integrator, w=24, h=20, spp=8, **kw):
    """The sensor inside the cube with sensor.medium set (volpath starts in
    the medium; prbvolpath ignores it, as the reference does).  The view from
    (0.2, 0.1, 0.5) down -z is aimed at (0, 0, -1): straight along -z the floor
    ends just below the bottom pixel row, and prbvolpath, which does not count
    emitter hits, would then return zero for every sample."""
    d = base(mi, integrator, w, h, spp, **kw)
    d["sensor"]["to_world"] = mi.Transform4f.look_at(origin=[0.2, 0.1, 0.5], target=[0.0, 0.0, -1.0], up=[0, 1, 0])
    d["sensor"]["medium"] = {"type": "ref", "id": "medium1"}
    return d


def camera_in_third(mi, integrator, w=24, h=20, spp=8, **kw):
    """three_media seen from inside cube 3, looking down at the other two:
    sensor.medium is the homogeneous medium of a scene that also holds
    heterogeneous ones (medium index 2; both vol_flags set)."""
    d = three_media(mi, integrator, w, h, spp, **kw)
    d["sensor"]["to_world"] = mi.Transform4f.look_at(origin=[0.2, 1.3, 0.1], target=[0.0, 0.0, 0.0], up=[0, 0, -1])
    d["sensor"]["medium"] = {"type": "ref", "id": "medium3"}
    return d


def no_emitter_sampling(mi, integrator, w=24, h=20, spp=8, **kw):
    d = base(mi, integrator, w, h, spp, albedo=[0.9, 0.5, 0.2], **kw)
    d["medium1"]["sample_emitters"] = False
    return d


def no_spectral_extinction(mi, integrator, w=24, h=20, spp=8, **kw):
    d = base(mi, integrator, w, h, spp, albedo=[0.9, 0.5, 0.2], **kw)
    d["medium1"]["has_spectral_extinction"] = False
    return d


def no_spectral_extinction_s37(mi, integrator, w=24, h=20, spp=8, **kw):
    """no_spectral_extinction at scale 3.7.  At scale 4 the majorant is a
    power of two and the two extinction branches round alike: every sample has
    the same bits with the flag and without it, so a kernel that ignored the
    flag would pass.  At 3.7 about two thirds of volpath's samples differ in
    their last bits (prbvolpath does not read the flag, as in the reference)."""
    return no_spectral_extinction(mi, integrator, w, h, spp, scale=3.7, **kw)


def grid_inside_cube(mi, integrator, w=24, h=20, spp=8, **kw):
    """The grid's box [-0.5, 0.5] x [-0.7, 0.5] x [-0.2, 0.7] strictly inside the cube."""
    T = mi.Transform4f
    d = base(mi, integrator, w, h, spp, **kw)
    d["medium1"]["sigma_t"]["to_world"] = T.translate([-0.5, -0.7, -0.2]) @ T.scale([1.0, 1.2, 0.9])
    return d


def use_grid_bbox(mi, integrator, w=24, h=20, spp=8, **kw):
    """The placement from the VolumeGrid's own bounding box: the base scene, said differently."""
    d = base(mi, integrator, w, h, spp, **kw)
    g = d["medium1"]["sigma_t"]["data"]
    d["medium1"]["sigma_t"] = {"type": "gridvolume", "grid": mi.VolumeGrid(g, (-1, -1, -1), (1, 1, 1)),
                               "use_grid_bbox": True}
    return d


def octahedron(r=1.3):
    """6 vertices at +-r on the axes, 8 faces wound so that the normals point outwards."""
    V = [[r, 0, 0], [-r, 0, 0], [0, r, 0], [0, -r, 0], [0, 0, r], [0, 0, -r]]
    F = []
    for sx in (0, 1):
        for sy in (0, 1):
            for sz in (0, 1):
                a, b, c = sx, 2 + sy, 4 + sz
                F.append([a, b, c] if (sx + sy + sz) % 2 == 0 else [a, c, b])
    return np.asarray(V, np.float32), np.asarray(F, np.uint32)


def mesh_boundary(mi, integrator, w=24, h=20, spp=8, **kw):
    """A triangle-mesh boundary (null BSDF) that is not the grid's box.  Its
    lowest vertex is at y = -1.3, so the floor lies at y = -1.45 here."""
    d = base(mi, integrator, w, h, spp, **kw)
    V, F = octahedron()
    d["cube"] = {"type": "mesh", "vertex_positions": V, "faces": F, "bsdf": {"type": "null"},
                 "interior": {"type": "ref", "id": "medium1"}}
    d["floor"] = floor(mi, -1.45)
    return d


INNER_KEY = "inner.bsdf.reflectance.value"


def object_inside(mi, integrator, w=24, h=20, spp=8, **kw):
    """A diffuse cube of half-size 0.3 inside the medium (exterior = medium1): no floor."""
    T = mi.Transform4f
    d = base(mi, integrator, w, h, spp, with_floor=False, **kw)
    d["inner"] = {"type": "cube", "to_world": T.translate([0.1, -0.2, 0.2]) @ T.scale([0.3, 0.3, 0.3]),
                  "bsdf": {"type": "diffuse", "reflectance": {"type": "rgb", "value": [0.7, 0.4, 0.3]}},
                  "exterior": {"type": "ref", "id": "medium1"}}
    return d


def nested_media(mi, integrator, w=24, h=20, spp=8, **kw):
    """A null-BSDF cube of half-size 0.45 holding a homogeneous medium2 inside
    medium1 (interior = medium2, exterior = medium1): the boundary leads from
    one medium straight into another, for camera paths and NEE walks alike."""
    T = mi.Transform4f
    d = base(mi, integrator, w, h, spp, **kw)
    d["medium2"] = {"type": "homogeneous", "sigma_t": 2.0, "scale": 1.0, "albedo": [0.5, 0.8, 0.9],
                    "phase": {"type": "isotropic"}}
    d["core"] = {"type": "cube", "to_world": T.translate([-0.1, 0.1, 0.0]) @ T.scale([0.45, 0.45, 0.45]),
                 "bsdf": {"type": "null"}, "interior": {"type": "ref", "id": "medium2"},
                 "exterior": {"type": "ref", "id": "medium1"}}
    return d


def area_light(mi, integrator, w=24, h=20, spp=8, **kw):
    """No sky and no sun: a rectangle area light above the cube, facing down."""
    T = mi.Transform4f
    d = base(mi, integrator, w, h, spp, sun=None, **kw)
    del d["sky"]
    d["light"] = {"type": "rectangle",
                  "to_world": T.translate([0.0, 1.6, 0.0]) @ T.rotate([1, 0, 0], 90) @ T.scale([0.8, 0.8, 0.8]),
                  "emitter": {"type": "area", "radiance": {"type": "rgb", "value": [8.0, 7.0, 6.0]}}}
    return d


def small_table():
    """Henyey-Greenstein g = 0.5 on 33 nodes uniform in the cosine."""
    c = np.linspace(-1.0, 1.0, 33)
    return {"type": "tabphase", "cost": c.astype(np.float32),
            "values": ((1 - 0.25) / (4 * np.pi * (1 + 0.25 - c) ** 1.5)).astype(np.float32)}


def two_tables(mi, integrator, w=24, h=20, spp=8, phase1=None, phase2=None, **kw):
    """three_media with medium1 and medium2 tabulated: two tables of different
    lengths in the one table buffer (tab_offset != 0 for the second).
    Defaults: medium1 the 33-node table, medium2 the 1,801-node table (e) of
    the phase-function tests."""
    d = three_media(mi, integrator, w, h, spp, **kw)
    if phase2 is None:
        phase2 = {"type": "tabphase", "cost": TABLES["e"][0], "values": TABLES["e"][1]}
    d["medium1"]["phase"] = phase1 if phase1 is not None else small_table()
    d["medium2"]["phase"] = phase2
    return d


CASES = {"three_media": three_media, "camera_inside": camera_inside, "camera_in_third": camera_in_third,
         "no_emitter_sampling": no_emitter_sampling, "no_spectral_extinction": no_spectral_extinction,
         "no_spectral_extinction_s37": no_spectral_extinction_s37, "grid_inside_cube": grid_inside_cube,
         "use_grid_bbox": use_grid_bbox, "mesh_boundary": mesh_boundary, "object_inside": object_inside,
         "nested_media": nested_media, "area_light": area_light, "two_tables": two_tables}

_ONE = ["medium1.sigma_t.data", "medium1.albedo.value"]
_THREE = ["medium1.sigma_t.data", "medium2.sigma_t.data", "medium3.sigma_t.value", "medium2.albedo.value",
          "medium1.albedo.value", "medium3.albedo.value", FLOOR_KEY]
KEYS = {name: _ONE + [FLOOR_KEY] for name in CASES}
KEYS["three_media"] = KEYS["camera_in_third"] = KEYS["two_tables"] = _THREE
KEYS["object_inside"] = _ONE + [INNER_KEY]
KEYS["nested_media"] = _ONE + ["medium2.sigma_t.value", "medium2.albedo.value", FLOOR_KEY]


def key_calls(name):
    """KEYS[name] split into render_backward calls of at most 4 small (rgb /
    scalar) parameters each; three_media's first call holds both grids and
    the homogeneous sigma_t."""
    k = KEYS[name]
    return [k[:4], k[4:]] if len(k) > 4 else [k]
