"""Scenes in which the depth limits decide what a sample returns (DESIGN.md §4,
"depth and roulette contract"), shared by the CPU property tests of the
oracle (test_depth_oracle.py) and the device-against-oracle tests
(test_gpu_depth_limits.py).  A plain helper module.

In the open Cornell box and the sparse fBm cube of the parity tests a path
leaves long before max_depth 32 or 64 matters, and no throughput comes near
the roulette's 0.95 clamp.  Here paths stay:

room    the Cornell box closed by a sixth wall at z = +1 that faces inward,
        seen from inside ((0, 0, 0.95) looking down -z, fov 90) with
        reflectances near one: white 0.97, green (0.3, 0.98, 0.3), red
        (1.0, 0.4, 0.4).  No ray escapes; with rr_depth above max_depth every
        path runs to max_depth, and with the roulette on its probability
        max(throughput) stays at the 0.95 clamp for many bounces.
dense   volume_cube with a homogeneous medium of sigma_t * scale = 200 and
        albedo 1 under the sky, no floor: a path that enters scatters
        hundreds of times before it leaves.
"""
import numpy as np

WHITE, GREEN, RED = [0.97, 0.97, 0.97], [0.3, 0.98, 0.3], [1.0, 0.4, 0.4]
LIGHT_KEY = "light.emitter.radiance.value"
RGB_KEYS = ["white.reflectance.value", "red.reflectance.value", "green.reflectance.value"]
BACK_KEY = "back.bsdf.reflectance.data"

# (max_depth, rr_depth): the depths at which an engine is chosen or a
# condition flips, with the roulette from the first bounce (1), at the default
# (5), one past max_depth (8, 9) and never (1000 / 100000)
GRID_PATH = [(0, 5), (1, 5), (2, 5), (3, 1), (8, 1), (8, 9), (32, 1000), (33, 1000), (64, 1000), (65, 1000),
             (-1, 1), (-1, 5)]
GRID_VOL = [(0, 5), (1, 5), (2, 5), (6, 1), (64, 100000), (65, 100000), (1024, 100000), (1025, 100000),
            (-1, 1), (-1, 100000)]


def room(mi, w=24, h=24, spp=8, boxes=False, bitmap=None):
    """The closed room.  boxes=False drops small-box / large-box: the deep
    cases then meet equal-distance hits only at the seams of the six walls.
    bitmap=(h, w, c): a bitmap reflectance with values in [0.9, 1.0] on the
    back wall (key BACK_KEY)."""
    T = mi.Transform4f
    d = mi.cornell_box()
    d["sensor"]["film"]["width"], d["sensor"]["film"]["height"] = w, h
    d["sensor"]["sampler"]["sample_count"] = spp
    d["sensor"]["fov"] = 90.0
    d["sensor"]["to_world"] = T.look_at(origin=[0, 0, 0.95], target=[0, 0, 0], up=[0, 1, 0])
    d["white"]["reflectance"]["value"] = list(WHITE)
    d["green"]["reflectance"]["value"] = list(GREEN)
    d["red"]["reflectance"]["value"] = list(RED)
    # the sixth wall: a rectangle's normal is +z, turned to face the room
    d["front"] = {"type": "rectangle", "to_world": T.translate([0.0, 0.0, 1.0]).rotate([0, 1, 0], 180),
                  "bsdf": {"type": "ref", "id": "white"}}
    if not boxes:
        del d["small-box"], d["large-box"]
    if bitmap is not None:
        data = np.random.default_rng(12).uniform(0.9, 1.0, bitmap).astype(np.float32)
        d["back"]["bsdf"] = {"type": "diffuse",
                             "reflectance": {"type": "bitmap", "data": data, "filter_type": "bilinear",
                                             "wrap_mode": "repeat", "raw": True}}
    return d


def dense(mi, integrator, w=24, h=20, spp=8, scale=200.0, albedo=1.0):
    """The homogeneous cube under the sky (and the sun), no floor."""
    d = mi.volume_cube(w, h, spp, medium_type="homogeneous", sigma_t=1.0, albedo=albedo, scale=scale)
    d["integrator"] = {"type": integrator, "max_depth": 64, "rr_depth": 5}
    return d


def integrator(mi, itype, max_depth, rr_depth, **kw):
    return mi.load_dict({"type": itype, "max_depth": max_depth, "rr_depth": rr_depth, **kw})
