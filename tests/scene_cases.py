"""Scene descriptions for the scene-build tests (test_scene_host.py on the host,
test_gpu_scene_create.py through the C ABI): a minimal valid description, the
faults mh_scene_create refuses with their literal codes and texts, and the
file form tools/scene_check.cpp reads.  A plain helper module."""
import copy
import ctypes as C

import numpy as np

from mitsuba_hip import _abi as A

INVALID_ARGUMENT, UNSUPPORTED = 1, 4  # MH_ERR_INVALID_ARGUMENT, MH_ERR_UNSUPPORTED
TABLES = ("shapes", "bsdfs", "textures", "emitters", "media", "positions", "normals", "texcoords", "faces", "texels",
          "grid")


def _rect_to_world():
    """a light under the ceiling, facing down: translate(0.1, 0.9, -0.05) rotate_y(30) rotate_x(90) scale(0.4, 0.3, 1)"""
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    ry = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]])
    rx = np.array([[1, 0, 0, 0], [0, 0, -1, 0], [0, 1, 0, 0], [0, 0, 0, 1]], np.float64)
    m = ry @ rx @ np.diag([0.4, 0.3, 1.0, 1.0])
    m[:3, 3] = (0.1, 0.9, -0.05)
    return m


class Desc:
    """A description as lists of the ctypes records and numpy tables.  null: tables passed as NULL whatever they
    hold; counts: n_* fields that differ from the tables' sizes."""

    def __init__(self):
        self.sensor = A.Sensor()
        self.sensor.width = self.sensor.height = 16
        self.sensor.medium = A.INVALID
        self.shapes, self.bsdfs, self.textures, self.emitters, self.media = [], [], [], [], []
        self.positions = np.zeros((0, 3), np.float32)
        self.normals = self.texcoords = None
        self.faces = np.zeros((0, 3), np.uint32)
        self.texels = np.zeros(0, np.float32)
        self.grid = np.zeros(0, np.float32)
        self.environment = A.INVALID
        self.null = set()
        self.counts = {}

    def copy(self):
        return copy.deepcopy(self)

    def _tables(self):
        rec = lambda xs: b"".join(bytes(x) for x in xs)
        arr = lambda a: None if a is None else np.ascontiguousarray(a).tobytes()
        t = dict(shapes=rec(self.shapes), bsdfs=rec(self.bsdfs), textures=rec(self.textures),
                 emitters=rec(self.emitters), media=rec(self.media), positions=arr(self.positions),
                 normals=arr(self.normals), texcoords=arr(self.texcoords), faces=arr(self.faces),
                 texels=arr(self.texels), grid=arr(self.grid))
        return [None if k in self.null else t[k] for k in TABLES]

    def _head(self):
        d = A.SceneDesc()
        d.abi_version = A.ABI_VERSION
        d.sensor = self.sensor
        d.n_shapes, d.n_bsdfs, d.n_textures = len(self.shapes), len(self.bsdfs), len(self.textures)
        d.n_emitters, d.n_media = len(self.emitters), len(self.media)
        d.n_vertices, d.n_faces = len(self.positions), len(self.faces)
        d.n_texels, d.n_grid = self.texels.size, self.grid.size
        d.environment = self.environment
        for k, v in self.counts.items():
            setattr(d, k, v)
        return d

    def blob(self):
        """the file form of tools/scene_check.cpp"""
        tabs = self._tables()
        lens = np.array([0xFFFFFFFFFFFFFFFF if t is None else len(t) for t in tabs], np.uint64)
        return bytes(self._head()) + lens.tobytes() + b"".join(t or b"" for t in tabs)

    def ctypes_desc(self):
        """(mh_scene_desc, what keeps its tables alive)"""
        d, keep = self._head(), []
        names = dict(grid="grid_data")
        for k, t in zip(TABLES, self._tables()):
            if t is None:
                continue
            buf = C.create_string_buffer(t, max(len(t), 1))
            keep.append(buf)
            field = names.get(k, k)
            setattr(d, field, C.cast(buf, dict(A.SceneDesc._fields_)[field]))
        return d, keep


def base():
    """One rectangle with an area emitter, one two-triangle mesh (a floor), one homogeneous and one heterogeneous
    (5 x 3 x 2) medium that no shape refers to, one rgb and one 2 x 2 bitmap texture."""
    d = Desc()
    m = _rect_to_world()
    inv = np.linalg.inv(m)
    r = A.Shape()
    r.type, r.bsdf, r.emitter = A.SHAPE_RECTANGLE, 0, 0
    r.interior_medium = r.exterior_medium = A.INVALID
    r.face_count = 1
    r.to_world[:] = m[:3].astype(np.float32).ravel().tolist()
    r.to_object[:] = inv[:3].astype(np.float32).ravel().tolist()
    du, dv = m[:3, 0] * 2, m[:3, 1] * 2
    n = np.cross(du, dv)
    r.frame_s[:] = (du / np.linalg.norm(du)).tolist()
    r.frame_t[:] = (dv / np.linalg.norm(dv)).tolist()
    r.frame_n[:] = (n / np.linalg.norm(n)).tolist()
    r.inv_area = 1.0 / np.linalg.norm(n)
    f = A.Shape()
    f.type, f.bsdf, f.emitter = A.SHAPE_MESH, 1, A.INVALID
    f.interior_medium = f.exterior_medium = A.INVALID
    f.face_count, f.vertex_count = 2, 4
    d.shapes = [r, f]
    # the subtractions v1 - v0 and v2 - v0 round in float32
    d.positions = np.array([[-1.1, -1.0, -1.05], [1.3, -1.00001, -0.9], [1.2, -0.99, 1.1], [-0.9, -1.02, 1.0]], np.float32)
    d.faces = np.array([[0, 2, 1], [0, 3, 2]], np.uint32)
    d.bsdfs = [A.Bsdf(A.BSDF_DIFFUSE, 0), A.Bsdf(A.BSDF_DIFFUSE, 1)]
    rgb, bmp = A.Texture(), A.Texture()
    rgb.type = A.TEX_RGB
    rgb.value[:] = [0.7, 0.6, 0.5]
    bmp.type, bmp.width, bmp.height, bmp.channels, bmp.filter, bmp.wrap = A.TEX_BITMAP, 2, 2, 3, 1, 2
    bmp.to_uv[:] = [1, 0, 0, 0, 1, 0]
    d.textures = [rgb, bmp]
    d.texels = np.linspace(0.2, 0.9, 12).astype(np.float32)
    e = A.Emitter()
    e.type, e.shape = A.EMITTER_AREA, 0
    e.radiance[:] = [9.0, 8.0, 7.0]
    d.emitters = [e]
    hom, het = A.Medium(), A.Medium()
    hom.type, hom.phase, hom.g, hom.scale, hom.sigma_t_const = A.MEDIUM_HOMOGENEOUS, A.PHASE_HG, 0.5, 1.3, 0.7
    hom.albedo[:] = [0.9, 0.8, 0.7]
    het.type, het.phase, het.scale, het.max_density = A.MEDIUM_HETEROGENEOUS, A.PHASE_ISOTROPIC, 2.5, 1.9
    het.albedo[:] = [0.5, 0.5, 0.5]
    het.grid_res[:] = [5, 3, 2]
    het.flags = A.MEDIUM_NO_SPECTRAL_EXTINCTION
    het.grid_to_local[:] = [0.5, 0, 0, 0.5, 0, 0.5, 0, 0.5, 0, 0, 0.5, 0.5]
    het.bbox_min[:] = [-1, -1, -1]
    het.bbox_max[:] = [1, 1, 1]
    d.media = [hom, het]
    d.grid = (np.arange(30, dtype=np.float32) + 1) / 16
    return d


def _set(path, value):
    """d.<path> = value, e.g. 'shapes[1].face_count'"""
    def fn(d):
        exec(f"d.{path} = value", {}, dict(d=d, value=value))
    return fn


def _null(name):
    return lambda d: d.null.add(name)


def _count(name, value):
    return lambda d: d.counts.__setitem__(name, value)


def _both(*fs):
    def fn(d):
        for f in fs:
            f(d)
    return fn


P = "mh_scene_create: "
RAYLEIGH = (P + "the rayleigh phase function is supported with depolarization = 0 only: otherwise its value differs from "
            "its sampling density and the sampling weight is not 1, which the volumetric integrators here do not carry")
AREA = P + "area emitters are supported on rectangles only"

# name: (edit of base(), code, text) -- one per rejection, in validate's order
FAULTS = {
    "film_size": (_set("sensor.width", 0), INVALID_ARGUMENT, P + "film size must be positive"),
    "film_height": (_set("sensor.height", 0), INVALID_ARGUMENT, P + "film size must be positive"),
    "area_emitter_on_mesh": (_set("emitters[0].shape", 1), UNSUPPORTED, AREA),
    "area_emitter_range": (_set("emitters[0].shape", 2), UNSUPPORTED, AREA),
    "mesh_face_range": (_set("shapes[1].face_count", 3), INVALID_ARGUMENT, P + "mesh range out of bounds"),
    "mesh_vertex_range": (_set("shapes[1].vertex_offset", 1), INVALID_ARGUMENT, P + "mesh range out of bounds"),
    "face_index": (_set("faces[1, 2]", 4), INVALID_ARGUMENT, P + "face index out of bounds"),
    "shape_type": (_set("shapes[1].type", 2), UNSUPPORTED, P + "unknown shape type"),
    "bsdf_index": (_set("shapes[0].bsdf", 2), INVALID_ARGUMENT, P + "bsdf index out of bounds"),
    "interior_medium": (_set("shapes[1].interior_medium", 2), INVALID_ARGUMENT, P + "medium index out of bounds"),
    "exterior_medium": (_set("shapes[0].exterior_medium", 7), INVALID_ARGUMENT, P + "medium index out of bounds"),
    "grid_zero_res": (_set("media[1].grid_res[1]", 0), INVALID_ARGUMENT, P + "volume grid out of bounds"),
    "grid_range": (_set("media[1].grid_offset", 1), INVALID_ARGUMENT, P + "volume grid out of bounds"),
    # 2^32 texels inside an n_grid nobody reads before the refusal
    "grid_2_32": (_both(_set("media[1].grid_res[:]", [4096, 4096, 256]), _count("n_grid", 2 ** 33)), UNSUPPORTED,
                  P + "volume grid above 2^32 texels"),
    "hg_g": (_set("media[0].g", 1.0), INVALID_ARGUMENT, "The asymmetry parameter must lie in the interval (-1, 1)!"),
    "hg_g_nan": (_set("media[0].g", float("nan")), INVALID_ARGUMENT,
                 "The asymmetry parameter must lie in the interval (-1, 1)!"),
    "phase_unknown": (_set("media[1].phase", 5), INVALID_ARGUMENT, P + "unknown phase function"),
    "rayleigh_depolarized": (_both(_set("media[0].phase", A.PHASE_RAYLEIGH), _set("media[0].g", 0.25)),
                             INVALID_ARGUMENT, RAYLEIGH),
    "pixel_format": (_set("sensor.pixel_format", 6), INVALID_ARGUMENT, P + "unknown pixel format"),
    "sensor_medium": (_set("sensor.medium", 2), INVALID_ARGUMENT, P + "sensor medium index out of bounds"),
    "texture_index": (_set("bsdfs[1].reflectance", 2), INVALID_ARGUMENT, P + "texture index out of bounds"),
    "bitmap_range": (_set("textures[1].data_offset", 1), INVALID_ARGUMENT, P + "bitmap data out of bounds"),
    # ---- what used to be trusted ----
    "null_shapes": (_null("shapes"), INVALID_ARGUMENT, P + "shapes is NULL with n_shapes > 0"),
    "null_bsdfs": (_null("bsdfs"), INVALID_ARGUMENT, P + "bsdfs is NULL with n_bsdfs > 0"),
    "null_textures": (_null("textures"), INVALID_ARGUMENT, P + "textures is NULL with n_textures > 0"),
    "null_emitters": (_null("emitters"), INVALID_ARGUMENT, P + "emitters is NULL with n_emitters > 0"),
    "null_media": (_null("media"), INVALID_ARGUMENT, P + "media is NULL with n_media > 0"),
    "null_positions": (_null("positions"), INVALID_ARGUMENT, P + "positions is NULL but a mesh has faces"),
    "null_faces": (_null("faces"), INVALID_ARGUMENT, P + "faces is NULL but a mesh has faces"),
    "null_grid": (_null("grid"), INVALID_ARGUMENT, P + "grid_data is NULL but a medium is heterogeneous"),
    "shape_emitter": (_set("shapes[1].emitter", 1), INVALID_ARGUMENT, P + "shape emitter index out of bounds"),
    "environment": (_set("environment", 1), INVALID_ARGUMENT, P + "environment emitter index out of bounds"),
    "normals_missing": (_set("shapes[1].has_normals", 1), INVALID_ARGUMENT, P + "a mesh has_normals but normals is NULL"),
    "texcoords_missing": (_set("shapes[1].has_texcoords", 1), INVALID_ARGUMENT,
                          P + "a mesh has_texcoords but texcoords is NULL"),
    # 2^64 - 10 + 30 wraps to 20 <= n_grid; 2^64 - 6 + 12 wraps to 6 <= n_texels
    "grid_wraps": (_set("media[1].grid_offset", 2 ** 64 - 10), INVALID_ARGUMENT, P + "volume grid range wraps 64 bits"),
    "bitmap_wraps": (_set("textures[1].data_offset", 2 ** 64 - 6), INVALID_ARGUMENT,
                     P + "bitmap data range wraps 64 bits"),
    # 2^24 x 2^24 texels of 2^16 channels: the product alone wraps to 0
    "bitmap_product_wraps": (_both(_set("textures[1].width", 2 ** 24), _set("textures[1].height", 2 ** 24),
                                   _set("textures[1].channels", 2 ** 16)), INVALID_ARGUMENT,
                             P + "bitmap data range wraps 64 bits"),
}


def _f(name):
    return FAULTS[name][0]


# two faults each: the one reported is the first in validate's order, not the first in the tables
ORDER = {
    "film_before_null": (_both(_f("null_shapes"), _f("film_size")), *FAULTS["film_size"][1:]),
    # shape 0 is no rectangle any more: its area emitter is refused before the shape loop finds the type
    "emitter_before_shape_type": (_set("shapes[0].type", 2), UNSUPPORTED, AREA),
    # loop 3 (meshes) ends before loop 4 (bsdf, media) starts, although shape 0 precedes shape 1
    "face_before_bsdf": (_both(_f("bsdf_index"), _f("face_index")), *FAULTS["face_index"][1:]),
    "shape_type_before_medium": (_both(_f("exterior_medium"), _f("shape_type")), *FAULTS["shape_type"][1:]),
    # per medium: medium 0's last check before medium 1's first
    "medium_order": (_both(_f("grid_range"), _f("rayleigh_depolarized")), INVALID_ARGUMENT, RAYLEIGH),
    "pixel_before_sensor_medium": (_both(_f("sensor_medium"), _f("pixel_format")), *FAULTS["pixel_format"][1:]),
    "old_before_new": (_both(_f("shape_emitter"), _f("bitmap_range")), *FAULTS["bitmap_range"][1:]),
    "null_before_index": (_both(_f("environment"), _f("null_grid")), *FAULTS["null_grid"][1:]),
    "environment_before_wrap": (_both(_f("grid_wraps"), _f("environment")), *FAULTS["environment"][1:]),
}


def faulty(name):
    edit = (FAULTS.get(name) or ORDER[name])[0]
    d = base()
    edit(d)
    return d
