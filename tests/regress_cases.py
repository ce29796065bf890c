"""The vectors and the sets the regression tests share (test_regress_host.py, test_gpu_regress.py): the time basis of a smooth
synthetic airmass, given vectors of any count up to 16, vectors that differ from segment to segment -- which catch a kernel
that reads segment 0's everywhere --, planted singular columns, and a set whose trends in time are multiples of the airmass
powers plus noise, for the end-to-end chain.  The data and the weights are sysrem_cases' and many_cases'."""
import numpy as np

from transit_amd import xcor

NVECS = [1, 3, 4, 5, 8, 9, 16]                    # below, at and above the kernels' padded counts 4, 8 and 16
NEXP_16 = 17                                     # the exposures the sets of 16 vectors have: columns stay non-singular


def airmass(nexp: int) -> np.ndarray:
    """[nexp]: sec z of a target that rises, culminates at z = 20 deg two thirds through the night and sets again"""
    hour = np.linspace(-4.0, 2.0, nexp)
    z = np.radians(20.0) + np.radians(10.0) * np.abs(hour) ** 1.2
    return 1.0 / np.cos(z)


def airmass_vectors(nexp: int, degree: int = 2) -> np.ndarray:
    """[nexp, degree + 1]: xcor.time_basis of the airmass"""
    return xcor.time_basis(airmass(nexp), degree)


def given(nexp: int, nvec: int, seed: int = 0) -> np.ndarray:
    """[nexp, nvec] for all segments: 1, t and t^2 of the airmass as far as nvec goes, seeded normal vectors behind them"""
    out = np.random.default_rng(900 + 31 * nvec + nexp + seed).standard_normal((nexp, nvec))
    k = min(nvec, 3)
    out[:, :k] = airmass_vectors(nexp, 2)[:, :k]
    return out


def per_segment(nseg: int, nexp: int, nvec: int, seed: int = 0) -> np.ndarray:
    """[nseg, nexp, nvec]: different seeded vectors in every segment, a constant first"""
    out = np.random.default_rng(950 + 17 * nvec + nexp + seed).uniform(-1.0, 1.0, (nseg, nexp, nvec))
    out[:, :, 0] = 1.0
    return out


def with_duplicate(vec, seg: int) -> np.ndarray:
    """[nseg, nexp, nvec] from per-segment vectors of nvec >= 2: segment seg's last vector a copy of its first -- every one
    of its columns has a singular pivot"""
    out = np.array(vec)
    out[seg, :, -1] = out[seg, :, 0]
    return out


def starved_weights(w, col: int, nlive: int) -> np.ndarray:
    """the weights with column col live at its first nlive exposures alone"""
    out = np.array(w)
    out[:, col] = 0.0
    out[:nlive, col] = 1.0
    return out


# ---- the end-to-end set: trends in time that ARE the airmass powers ------------------------------------------
E2E_LENGTHS = [400, 400]
E2E_SEG = xcor.segments(E2E_LENGTHS)
E2E_NOISE = 1e-4


def trend_set(nexp: int, seed: int = 31, noise: float = E2E_NOISE):
    """(data [nexp, 800], weight, gain): a continuum of order 1 whose every column changes in time by its own multiples of
    t and t^2 of the airmass, plus seeded noise; weights in [0.5, 2) with 2 % single masked entries"""
    rng = np.random.default_rng(seed)
    npix = int(E2E_SEG[-1])
    x = np.linspace(0.0, 1.0, npix)
    T = airmass_vectors(nexp, 2)
    cont = 1.0 + 0.3 * np.sin(5.0 * x)
    c1, c2 = 0.1 * (1.0 + 0.5 * np.cos(3.0 * x)), 0.05 * np.cos(7.0 * x)
    data = cont[None, :] * (1.0 + T[:, 1:2] * c1[None, :] + T[:, 2:3] * c2[None, :]) + noise * rng.standard_normal((nexp, npix))
    w = rng.uniform(0.5, 2.0, (nexp, npix))
    w[rng.random((nexp, npix)) < 0.02] = 0.0
    return data, w, rng.uniform(0.5, 1.5, npix)
