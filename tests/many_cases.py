"""The sets the tests of the exposure, order and pixel axes share (test_many_cases_host.py, test_gpu_many_exposures.py,
test_gpu_long_orders.py): observed sets of 64, 65 and 130 exposures over the 800 pixels of xcor_checks -- a wave of
exposures, a wave plus one, two waves and a ragged third; 64 is a multiple of the filter kernels' 4 and of SYSREM's 8
exposures per trip, 65 one past both --, sets of 5 exposures over 64, 65 and 130 short segments, and long_set: 12 exposures
over orders of a detector's length, 1024, 1025 and 2049 pixels, with what it plants (see there).  Seeded numpy only; the pixel
centres are the device tests' business.

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
LENGTHS = [1, 63, 64, 65, 200, 0, 7, 400]        # xcor_checks' segments
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


def data_set(nexp: int, npix: int, seed: int, noise: float = 0.01, nterms: int = 6, trends: float = 1.0) -> np.ndarray:
    """[nexp, npix]: sysrem_cases.data_set for any number of pixels -- a continuum of order 1 times (1 + a few smooth trends
    in time of falling size) plus noise; trends scales every trend in time (1: sysrem_cases' own, to the bit)"""
    rng = np.random.default_rng(seed)
    x, t = np.linspace(0.0, 1.0, npix), np.linspace(-1.0, 1.0, nexp)
    cont = 1.0 + 0.3 * np.sin(7.0 * x) + 0.1 * np.cos(31.0 * x)
    d = np.ones((nexp, npix))
    for k in range(nterms):
        d += trends * 0.2 * 0.4 ** k * rng.uniform(-1.0, 1.0, nexp)[:, None] * np.cos((3.0 + 5.0 * k) * x + rng.uniform(0, 6.0))[None, :] * (1.0 + 0.2 * t[:, None])
    return cont[None, :] * d * (1.0 + trends * 0.05 * t[:, None]) + noise * rng.standard_normal((nexp, npix))


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
    """nexp exposures of xcor_checks.pixel_set's 800 pixels; the column 300 (of the 200-pixel segment) is masked at every exposure,
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


# ---- long orders -----------------------------------------------------------------------------------------------------
LONG_NEXP = 12
LONG_LENGTHS = [1024, 1025, 0, 2049, 7]          # 4105 pixels
LONG_SEGS = (0, 1, 3)                            # the long segments
LONG_TIE_SEGS = (1, 3)                           # the copy after the original in the first, before it in the second
LONG_TRENDS = 0.05                               # data_set's trends, about the size of its noise (see long_set)
SCAT_TRIP = 1024                                 # kScatLds: k_scatter_median stages a segment's variances this many at a time
HP_TILE = 512                                    # kHpTile
HP_NEAR = 5                                      # hpdata_cases.NEAR
LONG_HALVES = (0, 5, 70, 600)                    # the high-pass halves of the long set's tests; 600: more than kHpTile
LONG_NOISY = {0: (137, 640, 1023), 1: (255, 256, 1023), 3: (511, 1024, 1500, 2048)}      # segment -> pixels of the segment
LONG_MASKED_COL, LONG_MASKED_EXP, LONG_MASKED_SEG = 300, 9, 1
LONG_OFF_GRID = (3, 700, 2700.0)                 # (segment, pixel of the segment, centre in cm-1)


@dataclass
class Planted:
    """what long_set plants, in pixels of the whole set: the tie pairs (segment, median column, its copy), the noisy columns,
    and the masked entries (exposure, pixel, border) about the high-pass tiles' borders"""
    ties: list
    noisy: tuple
    near: list
    weighted: bool


def trip_of(seg_first, s: int, p: int) -> int:
    """the staging trip of k_scatter_median that holds pixel p of segment s"""
    return (int(p) - int(seg_first[s])) // SCAT_TRIP


def ranked(var, seg_first, s: int):
    """the live columns of segment s in the order of the definition: ascending var, ties by ascending pixel
    (scatter_cases.ranked over any segments)"""
    a, b = int(seg_first[s]), int(seg_first[s + 1])
    live = np.flatnonzero(var[a:b] > 0)
    return a + live[np.argsort(var[a:b][live], kind="stable")]


def hp_borders(lengths):
    """[(segment, pixel)]: the first pixel of every high-pass tile of the long segments but a segment's first"""
    seg = xcor.segments(lengths)
    return [(s, int(seg[s]) + k) for s in LONG_SEGS for k in range(HP_TILE, lengths[s], HP_TILE)]


def _plant_long_ties(data, weight, seg, weighted, taken):
    """Per LONG_TIE_SEGS segment, the column of the median rank copied -- data and weights -- onto a column of another staging
    trip: in the 1025-pixel segment onto its last pixel, the second trip's only value (the copy AFTER the original), in the
    2049-pixel segment onto a column of the first trip, the original in the second (the copy BEFORE it).  The original is the
    column that holds the median rank (m - 1) // 2 once the copy's own column is gone, so the two hold the ranks r and r + 1
    whatever the copy's column held before: scatter_cases.plant_ties' end (the median column copied onto the column of the
    next rank) for a copy's column of any variance.  Where the 2049-pixel segment's median column lies in the first trip it first changes places, data and weights,
    with the column 1024 pixels on: the variances, and so the ranks, stay."""
    w_rank = weight if weighted else None
    ties = []
    for s in LONG_TIE_SEGS:
        first, n = int(seg[s]), int(seg[s + 1] - seg[s])
        if n == SCAT_TRIP + 1:
            b = first + SCAT_TRIP
        else:
            b = first + 100
        assert b not in taken
        var = xcor.scatter_reference(data, w_rank, seg, xcor.SCATTER_MASK)[0]
        order = ranked(var, seg, s)
        order = order[order != b]
        a = int(order[order.size // 2])                        # (m' - 1) // 2 of m' = order.size + 1 live columns
        if n != SCAT_TRIP + 1 and trip_of(seg, s, a) == 0:
            other = a + SCAT_TRIP
            assert other not in taken and other != b and trip_of(seg, s, other) == 1
            data[:, [a, other]] = data[:, [other, a]]
            weight[:, [a, other]] = weight[:, [other, a]]
            a = other
        assert trip_of(seg, s, a) != trip_of(seg, s, b)
        data[:, b] = data[:, a]
        weight[:, b] = weight[:, a]
        ties.append((s, a, b))
    return ties


def long_set(weighted: bool = True):
    """(ManySet, Planted): 12 exposures of [1024, 1025, 0, 2049, 7] pixels, detector-length orders -- 1024 is one staging trip
    of k_scatter_median exactly and four whole scatter tiles of 256; 1025 a second trip of one value, a fifth scatter tile of
    one column and a third high-pass tile of one pixel; 2049 three trips, kNormCap + 1, eight full row steps of 256 plus one
    lane, and nine scatter tiles.  data_set and edge_weights as the other sets use them (column 300 masked at every exposure,
    exposure 9 over the whole 1025-pixel segment), one off-grid pixel inside the 2049-pixel segment, and planted:

      the noisy columns   LONG_NOISY: 10 x the noise, in every long segment, the last pixel of the 2049-pixel segment (the
                          one-column tile, the last trip's only value) and the columns at a 1023 | 1024 border among them.
                          A clip of 3 has to remove exactly these on the RAW data too, so the trends in time are data_set's
                          scaled by LONG_TRENDS = 0.05 -- about the size of the noise; at full size the raw columns' variances
                          are the trends' (a median of 0.003 to 0.03) and 10 x the noise (0.01) would not stand out
      the border entries  a masked entry within HP_NEAR pixels below every kHpTile border of the long segments and one above
                          it (not above where that is the segment's last pixel), at different exposures
      the ties            _plant_long_ties, against the ranking WITH the weights (weighted, the default) or without them: the
                          two sets differ in the tie columns alone, as scatter_cases.the_set(nexp, weighted) does"""
    if ("long", weighted) not in _SETS:
        lengths, nexp = list(LONG_LENGTHS), LONG_NEXP
        seg = xcor.segments(lengths)
        npix = int(seg[-1])
        masked_col = int(seg[0]) + LONG_MASKED_COL
        w = edge_weights(nexp, lengths, 700 + nexp, masked_col, LONG_MASKED_EXP, LONG_MASKED_SEG)
        data = data_set(nexp, npix, 800 + nexp, trends=LONG_TRENDS)
        smooth = data_set(nexp, npix, 800 + nexp, noise=0.0, trends=LONG_TRENDS)
        noisy = tuple(int(seg[s]) + p for s in LONG_SEGS for p in LONG_NOISY[s])
        for p in noisy:
            data[:, p] = smooth[:, p] + 10.0 * (data[:, p] - smooth[:, p])
        off = {int(seg[LONG_OFF_GRID[0]]) + LONG_OFF_GRID[1]: LONG_OFF_GRID[2]}
        near = []
        for i, (s, q) in enumerate(hp_borders(lengths)):
            sides = [q - 2 - i % 3] + ([q + i % (HP_NEAR + 1)] if q + 1 < int(seg[s + 1]) else [])
            for j, p in enumerate(sides):
                v = (2 * i + 5 * j + 1) % nexp
                assert p not in noisy and p != masked_col
                w[v, p] = 0.0
                near.append((v, int(p), q))
        taken = set(noisy) | {masked_col} | set(off) | {p for _, p, _ in near}
        ties = _plant_long_ties(data, w, seg, weighted, taken)
        gain = np.random.default_rng(750 + nexp).uniform(0.5, 1.5, npix)
        ms = ManySet("long orders" + ("" if weighted else ", ties without weights"), lengths, data, w, gain, off, masked_col, LONG_MASKED_EXP, LONG_MASKED_SEG)
        data.setflags(write=False)
        w.setflags(write=False)
        _SETS["long", weighted] = (ms, Planted(ties, noisy, near, weighted))
    return _SETS["long", weighted]

