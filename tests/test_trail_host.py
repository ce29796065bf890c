"""Host side of the trail runs (transit_amd.xcor: trail_reference, velocity_map, lag_grid) and the agreement of the
header's trail prototypes with transit_amd._abi -- no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from transit_amd import _abi, build, pixels, xcor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_set(seed=5, nlag=6, nexp=4, lengths=(1, 20, 0, 30)):
    rng = np.random.default_rng(seed)
    npix = int(sum(lengths))
    pairs = np.stack([rng.uniform(0.5, 1.5, (nlag, npix)), rng.uniform(1.0, 2.0, (nlag, npix))], axis=-1)
    pairs[2, 7] = (0.0, 0.0)                               # a pixel off the grid at one lag
    w = rng.uniform(0.5, 2.0, (nexp, npix))
    w[rng.random((nexp, npix)) < 0.1] = 0.0
    ob = xcor.Observed(xcor.segments(lengths), rng.standard_normal((nexp, npix)), w, rng.uniform(0.5, 1.5, npix))
    return pairs, ob


def test_trail_reference_is_the_moment_reference_lag_by_lag():
    pairs, ob = small_set()
    trail, scale = xcor.trail_reference(pairs, ob), xcor.trail_abs_reference(pairs, ob)
    assert trail.shape == scale.shape == (6, 4, 4, 7)
    for l in range(pairs.shape[0]):
        rep = np.repeat(pairs[l][None], ob.nexp, axis=0)
        assert np.array_equal(trail[l], xcor.reference(rep, ob)), l
        assert np.array_equal(scale[l], xcor.abs_reference(rep, ob)), l
    assert np.all(trail[:, :, 2] == 0)                     # the empty segment
    assert np.all(trail[2, :, 1, 0] == trail[3, :, 1, 0] - (ob.weight[:, 7] > 0))      # the dead pixel counts nowhere
    assert np.all(np.abs(trail[..., 1:]) <= scale[..., 1:])
    with pytest.raises(ValueError):
        xcor.trail_reference(pairs[:, :-1], ob)


def test_lag_grid_round_trips_through_the_shift():
    kms, lags = xcor.lag_grid(-50.0, 50.0, 2.5)
    assert kms.shape == lags.shape == (41,) and kms[0] == -50.0 and kms[-1] == 50.0 and kms[20] == 0.0
    assert np.array_equal(lags, [pixels.shift(v) for v in kms]) and lags[20] == 1.0
    assert np.all(np.diff(lags) < 0)                       # receding: redshifted
    beta = (1.0 - lags ** 2) / (1.0 + lags ** 2)
    assert np.max(np.abs(beta * pixels.C_KMS - kms)) < 1e-9
    assert xcor.lag_grid(0.0, 1.0, 0.3)[0].tolist() == pytest.approx([0.0, 0.3, 0.6, 0.9])
    assert xcor.lag_grid(3.0, 3.0, 1.0)[0].tolist() == [3.0]
    for bad in ((0.0, 1.0, 0.0), (1.0, 0.0, 0.5), (0.0, 1.0, -1.0)):
        with pytest.raises(ValueError):
            xcor.lag_grid(*bad)


def synthetic(kms, centres, width, nseg=2):
    """a trail whose WFG moment is a Gaussian in lag velocity around each exposure's centre (segment s: 1 + s times it)"""
    trail = np.zeros((kms.size, centres.size, nseg, 7))
    bump = np.exp(-0.5 * ((kms[:, None] - centres[None, :]) / width) ** 2)
    for s in range(nseg):
        trail[:, :, s, xcor.WFG] = (1.0 + s) * bump
    return trail


def wfg(trail):
    return np.asarray(trail)[..., xcor.WFG]


def test_velocity_map_peaks_at_the_injected_cell():
    kms, _ = xcor.lag_grid(-90.0, 90.0, 1.0)
    phase = np.linspace(-0.08, 0.08, 9)
    kp_true, vsys_true = 120.0, -7.0
    trail = synthetic(kms, vsys_true + kp_true * np.sin(2 * np.pi * phase), 2.0)
    kp, vsys = np.linspace(60.0, 180.0, 13), np.linspace(-25.0, 25.0, 51)
    assert kp[6] == kp_true and vsys[18] == vsys_true
    vp = vsys[None, :, None] + kp[:, None, None] * np.sin(2 * np.pi * phase)[None, None, :]
    m = xcor.velocity_map(trail, kms, vp, stat=wfg)
    assert m.shape == (13, 51)
    inside = np.all((vp >= kms[0]) & (vp <= kms[-1]), axis=-1)
    # NaN exactly where a velocity leaves the lag grid
    assert np.array_equal(np.isnan(m), ~inside) and inside.any() and (~inside).any()
    assert np.unravel_index(np.nanargmax(m), m.shape) == (6, 18)
    # (every exposure near its bump's top in both segments: what the linear interpolation of a Gaussian of 2 km/s on a
    # grid of 1 km/s loses is at most 1 - exp(-1/32), 3.1 %)
    assert 9 * 3.0 * np.exp(-1.0 / 32.0) <= m[6, 18] <= 9 * 3.0
    # one cell at a time gives the same number
    assert xcor.velocity_map(trail, kms, vp[6, 18], stat=wfg) == pytest.approx(m[6, 18], rel=1e-15)
    # the ends of the grid are inside it
    edge = np.array([[kms[0]] * 9, [kms[-1]] * 9, [kms[-1] + 1e-9] * 9])
    assert np.isnan(xcor.velocity_map(trail, kms, edge, stat=wfg)).tolist() == [False, False, True]


def test_velocity_map_interpolates_a_linear_statistic_exactly():
    kms = np.array([-10.0, -4.0, -1.0, 0.5, 3.0, 11.0])     # an uneven grid
    nexp, nseg = 5, 3
    rng = np.random.default_rng(8)
    a, b = rng.standard_normal((nexp, nseg)), rng.standard_normal((nexp, nseg))
    trail = np.zeros((kms.size, nexp, nseg, 7))
    trail[..., xcor.WFG] = a[None] + b[None] * kms[:, None, None]
    vp = rng.uniform(-10.0, 11.0, (4, 6, nexp))
    got = xcor.velocity_map(trail, kms, vp, stat=wfg)
    want = np.sum(a.sum(axis=1)[None, None, :] + b.sum(axis=1)[None, None, :] * vp, axis=-1)
    assert got.shape == (4, 6) and np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want))
    with pytest.raises(ValueError):
        xcor.velocity_map(trail, kms[::-1], vp, stat=wfg)
    with pytest.raises(ValueError):
        xcor.velocity_map(trail, kms, vp[..., :-1], stat=wfg)
    with pytest.raises(ValueError):
        xcor.velocity_map(trail[:-1], kms, vp, stat=wfg)


def test_velocity_map_skips_the_rows_the_statistic_leaves_undefined():
    pairs, ob = small_set(nlag=5)
    trail = xcor.trail_reference(pairs, ob)
    cc = xcor.ccf(trail)
    assert np.all(np.isnan(cc[:, :, 0])) and np.all(np.isnan(cc[:, :, 2])) and np.all(np.isfinite(cc[:, :, [1, 3]]))
    kms = np.arange(5.0)
    for k in range(5):                                     # on a lag: that lag's rows, the nan ones left out
        got = xcor.velocity_map(trail, kms, np.full(ob.nexp, kms[k]))
        assert got == pytest.approx(float(np.nansum(cc[k])), rel=1e-14)
    half = xcor.velocity_map(trail, kms, np.full(ob.nexp, 1.5))
    assert half == pytest.approx(0.5 * float(np.nansum(cc[1]) + np.nansum(cc[2])), rel=1e-13)


C_TYPES = {
    "trx_handle *": C.c_void_p, "trx_batch *": C.c_void_p,
    "const trx_atm *": C.POINTER(_abi.TrxAtm), "const trx_opts *": C.POINTER(_abi.TrxOpts), "trx_debug *": C.POINTER(_abi.TrxDebug),
    "double *": _abi.c_double_p, "const double *": _abi.c_double_p, "int32_t": C.c_int32,
    "const double *const *": C.POINTER(_abi.c_double_p), "double *const *": C.POINTER(_abi.c_double_p),
}


def prototype(name):
    """the ctypes of the parameters of `int name(...)` as include/transit_hip.h declares it"""
    txt = open(os.path.join(ROOT, "include", "transit_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, name
    norm = lambda t: re.sub(r"\s*\*\s*", "*", re.sub(r"\s+", " ", t)).strip()
    types = {norm(k): v for k, v in C_TYPES.items()}
    out = []
    for par in m.group(1).split(","):
        out.append(types[norm(re.sub(r"\b[A-Za-z_0-9]+\s*$", "", par.strip()))])
    return out


def test_header_prototypes_and_abi_signatures_agree():
    path = build.lib_path("libtransit_hip.so")
    if not os.path.exists(path):
        build.build_hip()
    lib = C.CDLL(path)
    for name in ("trx_run_trail", "trx_run_batch_trail"):
        assert hasattr(lib, name), name
    _abi.bind(lib, _abi.HIP_HEADER, "trx_")
    assert prototype("trx_run_moments") == list(lib.trx_run_trail.argtypes)      # (the parser, on a call bound before)
    for name in ("trx_run_trail", "trx_run_batch_trail"):
        f = getattr(lib, name)
        assert list(f.argtypes) == prototype(name), name
        assert f.restype is C.c_int
    assert len(lib.trx_run_trail.argtypes) == 8 and len(lib.trx_run_batch_trail.argtypes) == 7
    lib.trx_abi_version.restype = C.c_int
    assert lib.trx_abi_version() == 5
    # without a handle both refuse
    trail, lag = np.zeros((1, 1, 1, 7)), np.ones(1)
    assert lib.trx_run_trail(None, None, None, None, 1, lag.ctypes.data_as(_abi.c_double_p),
                             trail.ctypes.data_as(_abi.c_double_p), None) == -1
    assert lib.trx_run_batch_trail(None, 0, None, None, 1, None, None) == -1
    assert b"k_trail_moments" in open(path, "rb").read()
