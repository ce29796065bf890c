"""The sets the tests of the exposure and order axes share (test_many_cases_host.py, test_gpu_many_exposures.py): observed
sets of 64, 65 and 130 exposures over the 800 pixels of test_gpu_moments -- a wave of exposures, a wave plus one, two waves
and a ragged third; 64 is a multiple of the filter kernels' 4 and of SYSREM's 8 exposures per trip, 65 one past both --, and
sets of 5 exposures over 64, 65 and 130 short segments.  Seeded numpy only; the pixel centres are the device tests' business.

Every set carries: data of order 1 (smooth trends in time and pixel plus seeded noise; the device tests multiply them by the
model's scale), weights in [0.5, 2] with 5 % exact zeros scattered over the segments of more than two pixels, one column
masked at every exposure, one exposure masked over a whole segment, gains in [0.5, 1.5], one shift per exposure (a velocity
ramp of +-40 km/s, the planet of ORBIT_KP), the orbit of that ramp, an exposure table with scale 0 at a few exposures and
smears with exact zeros among them, and a map of 3 x 4 cells over 11 lags in which exactly one cell leaves the lag grid, at
the last exposure only."""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from transit_amd import pixels, xcor
from transit_amd.exposures import Exposures

NEXPS = (64, 65, 130)
NSEGS = (64, 65, 130)
LENGTHS = [1, 63, 64, 65, 200, 0, 7, 400]        # test_gpu_moments' segments
OFF_GRID = {250: 2400.0, 700: 2700.0}            # and its two off-grid pixels: pixel -> centre (cm-1)
PATTERN = [3, 1, 0, 5, 2, 64, 1]                 # the many-orders sets' lengths, cycled
ORDERS_NEXP = 5
ORBIT_KP = 108.0                                 # km/s: velocity = ORBIT_KP * orbit
RAMP = 40.0                                      # km/s
LAG_KMS, LAGS = xcor.lag_grid(-15.0, 15.0, 3.0)  # 11 lags
KP, VSYS = np.array([10.0, 20.0, 32.6]), np.array([-2.0, 0.0, 1.5, 3.0])
OUTSIDE_CELL = (2, 3)                            # 32.6 * 40 / 108 + 3 = 15.07 > 15 at the last exposure, 14.94 at the most before
ZERO_SCALE = (3, 62, 63, 64, 70)                 # the table's scale is 0 at those of these exposures the set has
SYSREM_PAIRS = ((1, 1), (8, 10), (16, 10), (5, 64))      # (ncomp, niter) of the many-exposures sets
ORDERS_NCOMP = 2                                 # with 5 exposures and 5 % zero weights more components kill too many columns


@dataclass
class ManySet:
    name: str
    lengths: list
    data: np.ndarray                             # [nexp, npix], of order 1
    weight: np.ndarray                           # [nexp, npix]
    gain: np.ndarray                             # [npix]
    off_grid: dict                               # pixel -> centre (cm-1) outside the spectrum's grid
    masked_col: int                              # weight 0 at every exposure
    masked_exp: int                              # weight 0 over the whole of segment masked_seg ...
    masked_seg: int
    dead_seg: Optional[int] = None               # the many-orders sets: a segment with every weight 0
    seg_first: np.ndarray = field(init=False)
    velocity: np.ndarray = field(init=False)     # [nexp] km/s
    shifts: np.ndarray = field(init=False)
    orbit: np.ndarray = field(init=False)
    offset: np.ndarray = field(init=False)
    scale: np.ndarray = field(init=False)        # the exposure table
    smear: np.ndarray = field(init=False)

    def __post_init__(self):
        self.seg_first = xcor.segments(self.lengths)
        nexp = self.nexp
        self.velocity = np.linspace(-RAMP, RAMP, nexp)
        self.shifts = np.array([pixels.shift(v) for v in self.velocity])
        self.orbit = self.velocity / ORBIT_KP
        self.offset = 0.05 * np.cos(np.arange(nexp))
        rng = np.random.default_rng(900 + nexp + self.nseg)
        self.scale = rng.uniform(0.5, 1.5, nexp) * np.where(np.arange(nexp) % 7 == 5, -0.25, 1.0)
        self.scale[[v for v in ZERO_SCALE if v < nexp]] = 0.0
        self.smear = rng.uniform(1e-7, 1.3e-5, nexp)
        self.smear[::5] = 0.0

    @property
    def nexp(self) -> int:
        return int(self.data.shape[0])

    @property
    def npix(self) -> int:
        return int(self.data.shape[1])

    @property
    def nseg(self) -> int:
        return len(self.lengths)

    def observed(self, scale: float = 1.0, weighted: bool = True) -> xcor.Observed:
        return xcor.Observed(self.seg_first, scale * self.data, self.weight if weighted else None, self.gain)

    def the_map(self, stat: str = "ccf", **over) -> xcor.VelocityMap:
        kw = dict(lag_kms=LAG_KMS, kp=KP, vsys=VSYS, orbit=self.orbit, offset=self.offset, stat=stat, scale=0.9, a=1.1, b=0.2)
        kw.update(over)
        return xcor.VelocityMap(**kw)

    def table(self) -> Exposures:
        return Exposures(self.scale.copy(), self.smear.copy())

    def segment(self, s: int) -> slice:
        return slice(int(self.seg_first[s]), int(self.seg_first[s + 1]))

    def swapped(self, a: int, b: int) -> "ManySet":
        """the same set with the exposures a and b exchanged: data, weights, shifts, orbit, offset and table together"""
        perm = np.arange(self.nexp)
        perm[[a, b]] = perm[[b, a]]
        other = ManySet(self.name + ", %d and %d swapped" % (a, b), self.lengths, self.data[perm], self.weight[perm], self.gain, self.off_grid,
                        self.masked_col, int(perm[self.masked_exp]), self.masked_seg, self.dead_seg)
        for k in ("velocity", "shifts", "orbit", "offset", "scale", "smear"):
            setattr(other, k, np.ascontiguousarray(getattr(self, k)[perm]))
        return other


def data_set(nexp: int, npix: int, seed: int, noise: float = 0.01, nterms: int = 6) -> np.ndarray:
    """[nexp, npix]: sysrem_cases.data_set for any number of pixels -- a continuum of order 1 times (1 + a few smooth trends
    in time of falling size) plus noise"""
    rng = np.random.default_rng(seed)
    x, t = np.linspace(0.0, 1.0, npix), np.linspace(-1.0, 1.0, nexp)
    cont = 1.0 + 0.3 * np.sin(7.0 * x) + 0.1 * np.cos(31.0 * x)
    d = np.ones((nexp, npix))
    for k in range(nterms):
        d += 0.2 * 0.4 ** k * rng.uniform(-1.0, 1.0, nexp)[:, None] * np.cos((3.0 + 5.0 * k) * x + rng.uniform(0, 6.0))[None, :] * (1.0 + 0.2 * t[:, None])
    return cont[None, :] * d * (1.0 + 0.05 * t[:, None]) + noise * rng.standard_normal((nexp, npix))


def edge_weights(nexp: int, lengths, seed: int, masked_col: int, masked_exp: int, masked_seg: int, dead_seg=None) -> np.ndarray:
    """[nexp, npix]: weights in [0.5, 2) with 5 % single masked entries in the segments of more than two pixels (a shorter
    segment would lose whole rows to them), masked_col masked at every exposure, exposure masked_exp masked over the whole of
    segment masked_seg, and every weight of dead_seg 0"""
    seg = xcor.segments(lengths)
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.5, 2.0, (nexp, int(seg[-1])))
    zero = rng.random(w.shape) < 0.05
    for s, n in enumerate(lengths):
        if n <= 2:
            zero[:, seg[s]:seg[s + 1]] = False
    w[zero] = 0.0
    w[:, masked_col] = 0.0
    w[masked_exp, seg[masked_seg]:seg[masked_seg + 1]] = 0.0
    if dead_seg is not None:
        w[:, seg[dead_seg]:seg[dead_seg + 1]] = 0.0
    return w


_SETS = {}


def exposures_set(nexp: int) -> ManySet:
    """nexp exposures of test_gpu_moments' 800 pixels; the column 300 (of the 200-pixel segment) is masked at every exposure,
    and one exposure over the whole 65-pixel segment: exposure 64 of 65, 127 of 130 -- on a wave's second and on its last
    trip over the exposures -- and, where no exposure has an index of 64 or more, 61 of 64"""
    if ("exp", nexp) not in _SETS:
        npix = sum(LENGTHS)
        masked_col, masked_seg = 300, 3
        masked_exp = max(nexp - 3, 64) if nexp > 64 else nexp - 3
        w = edge_weights(nexp, LENGTHS, 200 + nexp, masked_col, masked_exp, masked_seg)
        gain = np.random.default_rng(300 + nexp).uniform(0.5, 1.5, npix)
        _SETS["exp", nexp] = ManySet("%d exposures" % nexp, list(LENGTHS), data_set(nexp, npix, 100 + nexp), w, gain, dict(OFF_GRID), masked_col, masked_exp, masked_seg)
    return _SETS["exp", nexp]


def orders_lengths(nseg: int):
    """PATTERN cycled: an empty segment at 2, 9, ..., 65, 72, ...; the segment min(64, nseg - 1) -- the dead one -- has 5
    pixels whatever the pattern gives it"""
    lengths = [PATTERN[s % len(PATTERN)] for s in range(nseg)]
    lengths[min(64, nseg - 1)] = 5
    return lengths


def orders_set(nseg: int) -> ManySet:
    """5 exposures of nseg short segments (at most 1411 pixels).  Segment 5 (64 pixels) holds the off-grid pixel and the masked
    column, exposure 2 is masked over segment 12 (64 pixels), and the segment min(64, nseg - 1) is dead: every weight 0"""
    if ("seg", nseg) not in _SETS:
        lengths = orders_lengths(nseg)
        seg = xcor.segments(lengths)
        npix, nexp = int(seg[-1]), ORDERS_NEXP
        dead = min(64, nseg - 1)
        masked_col = int(seg[5]) + 20
        w = edge_weights(nexp, lengths, 400 + nseg, masked_col, 2, 12, dead)
        gain = np.random.default_rng(500 + nseg).uniform(0.5, 1.5, npix)
        _SETS["seg", nseg] = ManySet("%d orders" % nseg, lengths, data_set(nexp, npix, 600 + nseg), w, gain, {int(seg[5]) + 10: 2400.0}, masked_col, 2, 12, dead)
    return _SETS["seg", nseg]


def all_sets():
    return [exposures_set(n) for n in NEXPS] + [orders_set(n) for n in NSEGS]


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a.view(np.int64)[~np.isnan(a)], b.view(np.int64)[~np.isnan(b)])
