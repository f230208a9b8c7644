"""The numpy restatement of IrregularContinuousDistribution (distr_1d.h:618-991),
the Henyey-Greenstein function and the phase tables shared by the phase-function
tests (test_gpu_phase_functions.py, test_gpu_vol_topologies.py, vol_cases.py).
A plain helper module."""
import numpy as np


# ---------------------------------------------------------------------------
# numpy restatement of IrregularContinuousDistribution (distr_1d.h:618-991)
# ---------------------------------------------------------------------------
class Distr:
    """nodes / pdf are the float32 inputs.  dt = float32: the arithmetic of the
    reference's single-precision variants (cdf accumulated in double, stored as
    float); dt = float64: the same formulas without rounding (the reference
    the errors are measured against)."""

    def __init__(self, nodes, pdf, dt):
        self.dt = dt
        self.x = np.asarray(nodes, np.float32).astype(dt)
        self.y = np.asarray(pdf, np.float32).astype(dt)
        x64, y64 = self.x.astype(np.float64), self.y.astype(np.float64)
        mass = 0.5 * (x64[1:] - x64[:-1]) * (y64[:-1] + y64[1:])
        self.cdf = np.cumsum(mass).astype(dt)           # double accumulation, stored as dt
        nz = np.nonzero(mass > 0)[0]
        self.valid = (int(nz[0]), int(nz[-1]))
        self.integral = self.cdf[self.valid[1]]
        self.normalization = dt(1) / self.integral
        self.n = self.x.size

    @staticmethod
    def _search(lo, hi, size, pred):
        """dr::binary_search: log2i(hi - lo) + 1 trips."""
        start, end = np.full(size, lo, np.int64), np.full(size, hi, np.int64)
        for _ in range(int(hi - lo).bit_length() if hi > lo else 0):
            mid = (start + end) >> 1
            c = pred(mid)
            start = np.where(c, np.minimum(mid + 1, end), start)
            end = np.where(c, end, mid)
        return start

    def _fma(self, a, b, c):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(self.dt)

    def _interval(self, x):
        i = self._search(0, self.n, x.size, lambda m: self.x[np.minimum(m, self.n - 1)] < x)
        return np.maximum(np.minimum(i, self.n - 1), 1) - 1

    def eval_pdf_normalized(self, x):
        x = np.asarray(x).astype(self.dt)
        active = (x >= self.x[0]) & (x <= self.x[-1])
        i = self._interval(x)
        x0, x1, y0, y1 = self.x[i], self.x[i + 1], self.y[i], self.y[i + 1]
        t = (x - x0) / (x1 - x0)
        return np.where(active, self._fma(t, y1 - y0, y0), self.dt(0)) * self.normalization

    def eval_cdf_normalized(self, x):
        x = np.asarray(x).astype(self.dt)
        i = self._interval(x)
        x0, x1, y0, y1 = self.x[i], self.x[i + 1], self.y[i], self.y[i + 1]
        c0 = np.where(i > 0, self.cdf[np.maximum(i, 1) - 1], self.dt(0))
        w = x1 - x0
        t = np.clip((x - x0) / w, 0, 1)
        return (c0 + w * t * (y0 + self.dt(0.5) * t * (y1 - y0))) * self.normalization

    def sample(self, u):
        s = np.asarray(u).astype(self.dt) * self.integral
        i = self._search(self.valid[0], self.valid[1], s.size,
                         lambda m: ((self.cdf[m] < s) | (self.cdf[m] == 0)) & (self.cdf[m] != self.integral))
        x0, x1, y0, y1 = self.x[i], self.x[i + 1], self.y[i], self.y[i + 1]
        c0 = np.where(i > 0, self.cdf[np.maximum(i, 1) - 1], self.dt(0))
        w = x1 - x0
        q = (s - c0) / w
        with np.errstate(invalid="ignore", divide="ignore"):
            t_linear = (y0 - np.sqrt(np.maximum(y0 * y0 + self.dt(2) * q * (y1 - y0), 0))) / (y0 - y1)
            t_const = q / y0
        return self._fma(np.where(y0 == y1, t_const, t_linear), w, x0)


def hg(g, cos_theta):
    """Henyey-Greenstein in the physics convention (+1 = forward)."""
    cos_theta = np.asarray(cos_theta, np.float64)
    return (1 - g * g) / (4 * np.pi * (1 + g * g - 2 * g * cos_theta) ** 1.5)


def _angles(step_deg):
    """cos of 180 .. 0 degrees: increasing cosines on a grid uniform in angle."""
    n = int(round(180 / step_deg)) + 1
    c = np.cos(np.deg2rad(np.linspace(180.0, 0.0, n)))
    c[0], c[-1] = -1.0, 1.0
    return c


def _mie_like(c):
    th = np.arccos(np.clip(c, -1, 1))
    return (0.8 * hg(0.93, c) + 0.15 * hg(0.5, c) + 0.05 * hg(-0.6, c)) * (1 + 0.3 * np.cos(40 * th))


def _tables():
    cd, ce, cf = _angles(1.0), _angles(0.1), np.linspace(-1.0, 1.0, 16385)
    t = {
        "a": ([-1, 1], [1, 1]),
        "b": ([-1, -0.5, 0.2, 0.9, 1], [0, 0.3, 0, 2, 40]),
        # (b) squeezed into [-0.8, 0.8], in front of it an interval without mass
        # ([-1, -0.8]: both values 0) and behind it a ramp to 0 and another one ([0.85, 1])
        "c": ([-1, -0.8, -0.4, 0.16, 0.72, 0.8, 0.85, 1], [0, 0, 0.3, 0, 2, 40, 0, 0]),
        "d": (cd, hg(0.85, cd)),
        "e": (ce, _mie_like(ce)),
        "f": (cf, hg(0.7, cf)),
    }
    return {k: (np.asarray(c, np.float64).astype(np.float32), np.asarray(v, np.float64).astype(np.float32))
            for k, (c, v) in t.items()}


TABLES = _tables()
assert np.diff(TABLES["e"][0].astype(np.float64)).min() < 1.6e-6   # the finest spacing, at the forward peak
