"""The host side of the detector-pixel runs (transit_amd/pixels.py) against the band definition it restates, and the
library's new entry points as far as they go without a device (no GPU)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from transit_amd import _abi, bands, build, pixels

V_KMS = (-150.0, -37.5, -3.1, 0.0, 3.1, 37.5, 150.0)


def grid(n=6001, wn_i=2500.0, wn_d=0.01):
    return wn_i, wn_d, n, wn_i + np.arange(n) * wn_d


def test_shift_and_builders():
    assert pixels.shift(0) == 1.0
    assert pixels.shift(0.0) == 1.0
    for v in (3.1, 150.0, 3000.0):
        beta = v / 299792.458
        assert pixels.shift(v) < 1.0 < pixels.shift(-v)                  # receding: to lower wavenumbers
        assert pixels.shift(v) * pixels.shift(-v) == pytest.approx(1.0, rel=1e-15)
        assert pixels.shift(v) == pytest.approx(1.0 - beta + beta * beta / 2, rel=beta ** 3 + 1e-15)
    px = pixels.resolving_power([2000.0, 3000.0], 3000.0, cut=3.0)
    assert len(px) == 2 and px.cut == 3.0
    assert px.centre.tolist() == [2000.0, 3000.0] and px.fwhm.tolist() == [2000.0 / 3000.0, 1.0]
    assert pixels.Pixels([2500.0], [0.1]).cut == 4.0
    with pytest.raises(ValueError):
        pixels.Pixels([1.0, 2.0], [1.0])
    c = pixels.to_c(px)
    assert C.sizeof(_abi.TrxPixels) == 32
    assert (c.npix, c.centre[1], c.fwhm[0], c.cut) == (2, 3000.0, 2000.0 / 3000.0, 3.0)


def test_as_bands_is_the_shifted_gaussians_in_v_p_order():
    px = pixels.Pixels([2510.0, 2520.5, 2505.25], [0.1, 0.2, 0.3], cut=3.5)
    sh = [1.0, 0.9995, 1.0005]
    bs = pixels.as_bands(px, sh)
    assert len(bs) == 9
    for v, s in enumerate(sh):
        for p in range(3):
            b = bs[v * 3 + p]
            assert b.kind == _abi.BAND_GAUSS
            assert (b.centre, b.fwhm, b.cut) == (float(px.centre[p]) / s, float(px.fwhm[p]) / s, 3.5)
    assert [(b.centre, b.fwhm) for b in bs[:3]] == [(2510.0, 0.1), (2520.5, 0.2), (2505.25, 0.3)]    # at rest: the set itself


def test_reference_is_the_band_definition():
    wn_i, wn_d, n, wn = grid()
    rng = np.random.default_rng(11)
    S = 1.0 + rng.random(n)
    centres = np.concatenate([np.linspace(2503, 2557, 40) + 0.37 * wn_d, [2499.9, 2560.05, 2400.0, 2700.0]])   # and off both ends
    px = pixels.Pixels(np.concatenate([centres, centres]), np.concatenate([centres / 20000, centres / 3000]), 4.0)
    sh = [1.0 - v / 299792.458 for v in V_KMS]
    ref = pixels.reference(S, wn_i, wn_d, n, px, sh)
    assert ref.shape == (len(sh), len(px), 2)
    bs = pixels.as_bands(px, sh)
    lens = set()
    for k, b in enumerate(bs):
        v, p = divmod(k, len(px))
        a, z = bands.gauss_range(wn_i, wn_d, n, b.centre, b.fwhm, b.cut)
        lens.add(z - a)
        sigma = b.fwhm / bands.FWHM_PER_SIGMA
        ws = [math.exp(-0.5 * (((wn_i + i * wn_d) - b.centre) / sigma) ** 2) for i in range(a, z)]
        want = (math.fsum(w * S[i] for w, i in zip(ws, range(a, z))), math.fsum(ws))
        for c in range(2):
            assert ref[v, p, c] == pytest.approx(want[c], rel=1e-14, abs=0), (v, p, c)
        if z == a:
            assert ref[v, p, 0] == 0 and ref[v, p, 1] == 0
    assert 0 in lens and max(lens) >= 283 and {42, 43, 44} & lens
    # a shard sees its own bins only; the shards' pairs add up to the whole grid's
    cuts = [0, 1500, 3777, n]
    parts = [pixels.reference(S[cuts[r]:cuts[r + 1]], wn_i, wn_d, n, px, sh, lo=cuts[r]) for r in range(3)]
    got = pixels.combine(parts)
    nz = ref != 0
    assert np.all(got[~nz] == 0)
    assert np.max(np.abs(got[nz] - ref[nz]) / np.abs(ref[nz])) <= 1e-14
    assert np.any((parts[1][..., 1] == 0) & (ref[..., 1] != 0))            # some pairs have no bin in the middle shard
    assert np.allclose(pixels.value(ref[:, :40]), 1.5, atol=0.5)


def test_combine_adds_in_the_order_given():
    parts = [np.array([[[1e16, 1.0]]]), np.array([[[1.0, 2.0]]]), np.array([[[-1e16, 3.0]]])]
    assert pixels.combine(parts).tolist() == [[[((1e16 + 1.0) - 1e16), 6.0]]]
    assert pixels.value(np.array([[[3.0, 2.0], [1.0, 4.0]]])).tolist() == [[1.5, 0.25]]
    with pytest.raises(ValueError):
        pixels.combine([])


def test_library_exports_and_refuses_without_a_handle():
    path = build.lib_path("libtransit_hip.so")
    if not os.path.exists(path):
        build.build_hip()
    lib = C.CDLL(path)
    for name in ("trx_set_pixels", "trx_run_pixels", "trx_batch_set_pixels", "trx_run_batch_pixels"):
        assert hasattr(lib, name), name
    _abi.bind(lib, _abi.HIP_HEADER, "trx_")
    px = pixels.resolving_power([2510.0, 2520.0], 20000.0)
    assert lib.trx_set_pixels(None, C.byref(pixels.to_c(px))) == -1
    assert lib.trx_set_pixels(None, None) == -1
    assert lib.trx_batch_set_pixels(None, C.byref(pixels.to_c(px))) == -1
    out, sh = np.zeros((1, 2, 2)), np.ones(1)
    assert lib.trx_run_pixels(None, None, None, None, 1, sh.ctypes.data_as(_abi.c_double_p),
                              out.ctypes.data_as(_abi.c_double_p), None) == -1
    assert lib.trx_run_batch_pixels(None, 0, None, None, 1, None, None) == -1
    blob = open(path, "rb").read()
    assert b"k_pixel_pairs" in blob
