"""The pixel-stage problem the device tests share: the synthetic cases, the band and pixel sets over their grids, variants
of a problem's atmosphere, and the accuracy rule of a pixel run.  A plain module: pytest collects nothing here, and no test
module imports another one for these.

make: 40 000 lines, 2500-2560 cm-1 in steps of 0.01 (6001 bins), 60 layers -- the case of the pixel, moment, trail and map
tests; make_band_case: 100 000 lines, 2500-2900 cm-1 (401 bins at an oversampling of 2160), 100 layers -- the case of the
band and contribution tests.

Tolerance of a pixel run's two accuracy checks (tolerance, check_close), per component, relative:
1e-12 + 2 * 2^-52 * nu_max / sigma_min.  1e-12 is the figure of test_gpu_bands for GAUSS bands (summation order and exp); the
second term bounds what a one-ulp difference in nu_i does to the weights: dx <= 2 ulp(nu) / sigma, and the Gaussian-weighted
mean of |x| is below 1."""
import ctypes as C
import os

import numpy as np

from transit_amd import _abi, bands, pixels, synth
from transit_amd.host import Problem


# ---- atmospheres ----------------------------------------------------------------------------------------------------
def atmospheres(P, k):
    """k variants of the problem's atmosphere: temperatures scaled by up to +-6 %, densities the other way
    (the arrays are kept alive by the returned list)."""
    a = P.atm
    L = P.layer_arrays()
    n = int(a.nlayer)
    keep, atms = [], []
    for j in range(k):
        f = 1.0 + 0.06 * np.sin(1.7 * j + 0.3)
        temp = np.ascontiguousarray(L["temp"] * f)
        dens = np.ascontiguousarray(L["density"] / f)
        keep += [temp, dens]
        b = _abi.TrxAtm()
        C.memmove(C.byref(b), C.byref(a), C.sizeof(_abi.TrxAtm))
        b.temp = temp.ctypes.data_as(_abi.c_double_p)
        b.density = dens.ctypes.data_as(_abi.c_double_p)
        atms.append(b)
    return atms, keep


# ---- the grid and the band sets -------------------------------------------------------------------------------------
def grid(P):
    st = P.static
    n = int(st.nwn)
    return float(st.wn_i), float(st.wn_d), n, st.wn_i + np.arange(n) * st.wn_d


def band_set(P, seed=0):
    """top-hats tiling the grid, overlapping filter curves, Gaussians at R = 300 and 3000 (one with its edges on
    grid points), a one-bin band, a whole-grid band, a band near the grid's start and a Gaussian off the grid"""
    wn_i, wn_d, n, wn = grid(P)
    rng = np.random.default_rng(seed)
    lo, hi = wn[0] - wn_d / 2, wn[-1] + wn_d / 2
    edges = np.linspace(lo, hi, 17)
    out = [bands.tophat(wn, edges[k], edges[k + 1]) for k in range(16)]
    for a, b in ((0.15, 0.55), (0.4, 0.8), (0.3, 0.95)):
        fw = np.sort(rng.uniform(wn[0] + a * (wn[-1] - wn[0]), wn[0] + b * (wn[-1] - wn[0]), 29))
        ft = np.sin(np.linspace(0.1, 3.0, fw.size)) ** 2 + 0.05
        out.append(bands.filter_curve(wn, fw, ft))
    span = wn[-1] - wn[0]
    out += bands.resolving_power(wn[0] + span * np.linspace(0.03, 0.97, 9) + 0.37 * wn_d, 300.0)
    out += bands.resolving_power(wn[0] + span * np.linspace(0.01, 0.99, 23) + 0.11 * wn_d, 3000.0)
    sig = 2.0 * wn_d                                   # 4 sigmas = 8 bins exactly: both edges on grid points
    out.append(bands.gauss(wn[n // 3], sig * bands.FWHM_PER_SIGMA, 4.0))
    out.append(bands.weights(n // 2, [0.7]))           # one bin
    out.append(bands.weights(0, 1.0 + 0.25 * np.sin(np.arange(n))))     # the whole grid
    out.append(bands.weights(2, [1.0, 2.0, 3.0]))      # outside every shard but the first
    out.append(bands.gauss(wn[0] - 50 * span, 1.0))    # no bin at all
    return out


def band_bins(P, b):
    """(global bins, weights) of a band by the header's rule"""
    wn_i, wn_d, n, wn = grid(P)
    if b.kind == _abi.BAND_WEIGHTS:
        return np.arange(b.first, b.first + b.weights.size), np.asarray(b.weights)
    a, z = bands.gauss_range(wn_i, wn_d, n, b.centre, b.fwhm, b.cut)
    i = np.arange(a, z)
    sigma = b.fwhm / bands.FWHM_PER_SIGMA
    x = ((wn_i + i * wn_d) - b.centre) / sigma
    return i, np.exp(-0.5 * (x * x))


def make_band_case(tmp_path, solution, **kw):
    d = str(tmp_path / solution)
    args = dict(nlines=100_000, wnlow=2500, wnhigh=2900, wndelt=1.0, wnosamp=2160, nlayers=100, solution=solution,
                toomuch=10.0, ethresh=1e-50, seed=41, ncia=2 if solution == "transit" else 1)
    args.update(kw)
    synth.make_case(d, **args)
    return Problem.from_cfg(os.path.join(d, "case.cfg"))


def thinner(P, f):
    """the problem's atmosphere with densities times f (f < 1: the rays go deeper)"""
    a = P.atm
    dens = np.ascontiguousarray(P.layer_arrays()["density"] * f)
    b = _abi.TrxAtm()
    C.memmove(C.byref(b), C.byref(a), C.sizeof(_abi.TrxAtm))
    b.density = dens.ctypes.data_as(_abi.c_double_p)
    return b, dens


# ---- the pixel sets and their shifts --------------------------------------------------------------------------------
V_KMS = (-150.0, -37.5, -3.1, 0.0, 3.1, 37.5, 150.0)
SHIFTS = np.array([1.0 - v / 299792.458 for v in V_KMS])


def make(tmp_path, solution, **kw):
    d = str(tmp_path / solution)
    args = dict(nlines=40_000, wnlow=2500, wnhigh=2560, wndelt=0.01, wnosamp=1, nlayers=60, solution=solution,
                toomuch=10.0, ethresh=1e-50, seed=41, ncia=2 if solution == "transit" else 1)
    args.update(kw)
    synth.make_case(d, **args)
    return Problem.from_cfg(os.path.join(d, "case.cfg"))


def set_a(P):
    """400 pixels at R = 20000: windows of 42-44 bins (a lane each)"""
    wn_d = float(P.static.wn_d)
    return pixels.resolving_power(np.linspace(2503, 2557, 400) + 0.37 * wn_d, 20000.0, 4.0)


def set_b(P):
    """the same centres at R = 3000: windows of 283-290 bins (a wave each)"""
    wn_d = float(P.static.wn_d)
    return pixels.resolving_power(np.linspace(2503, 2557, 400) + 0.37 * wn_d, 3000.0, 4.0)


def joined(*sets):
    return pixels.Pixels(np.concatenate([s.centre for s in sets]), np.concatenate([s.fwhm for s in sets]), sets[0].cut)


def window_lengths_and_margin(P, px, shifts):
    """the whole-grid window length of every pair, and the smallest distance (in bins) of a window edge from a grid
    point: a one-bin disagreement about a range cannot hide behind rounding when it is far above an ulp"""
    wn_i, wn_d, n, _ = grid(P)
    lens, margin = [], np.inf
    for b in pixels.as_bands(px, shifts):
        a, z = bands.gauss_range(wn_i, wn_d, n, b.centre, b.fwhm, b.cut)
        lens.append(z - a)
        sigma = b.fwhm / bands.FWHM_PER_SIGMA
        for edge in ((b.centre - b.cut * sigma - wn_i) / wn_d, (b.centre + b.cut * sigma - wn_i) / wn_d):
            margin = min(margin, abs(edge - round(edge)))
    return np.array(lens), margin


def tolerance(px, shifts):
    nu_max = float(np.max(px.centre)) / float(np.min(shifts))
    sigma_min = float(np.min(px.fwhm)) / float(np.max(shifts)) / bands.FWHM_PER_SIGMA
    return 1e-12 + 2.0 * 2.0 ** -52 * nu_max / sigma_min


def check_close(got, ref, tol, what=""):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    zero = ref == 0
    assert np.all(got[zero] == 0), (what, got[zero][got[zero] != 0][:4])
    err = np.abs(got[~zero] - ref[~zero]) / np.abs(ref[~zero])
    worst = float(err.max()) if err.size else 0.0
    print("%s: max rel err %.3e (tolerance %.3e)" % (what, worst, tol))
    assert worst <= tol, (what, worst, tol)


def check_accuracy(P, px, shifts, out, spec, tol, lo=0, what=""):
    wn_i, wn_d, n, _ = grid(P)
    check_close(out, pixels.reference(spec, wn_i, wn_d, n, px, shifts, lo=lo), tol, what)
