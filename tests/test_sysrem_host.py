"""Detrending the observed set without a device: the refusals, the tiles, the extents and the arithmetic of
transit_amd/csrc/trx_sysrem.h through tests/sysrem_check.cpp, a stand-alone program over exact-size heap arrays under
-fsanitize=address,undefined that walks a whole set the way the kernels do; its U, coef and residuals held bit for bit
against xcor.sysrem_reference, the numpy mirror; the mirror's own properties (weights None = weights 1, unit vectors, the
agreement with xcor.sysrem_basis, the injection's fixed points); and the ABI: the struct's size, the constant, the exported
symbol and the kernels in the code object."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from bits import same_bits
from host_check import build_check

import many_cases as mc
import sysrem_cases as sc
from transit_amd import _abi, build, xcor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return build_check("sysrem_check", tmp_path_factory.mktemp("sysrem_check"))


def test_refusals_extents_tiles_and_known_sets_under_sanitizers(check_exe):
    out = subprocess.run([check_exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stderr == ""                              # (no sanitizer report)
    lines = out.stdout.splitlines()
    last = lines[-1].split()
    assert last[0] == "ok" and int(last[1]) > 60, lines[-20:]
    assert not [line for line in lines if line.startswith("FAILED")]


_MIRROR = {}


def mirror(nexp, weighted, ncomp, niter):
    """(data, weight, (basis, coef, resid)) of the shared set, computed once per case"""
    key = (nexp, weighted, ncomp, niter)
    if key not in _MIRROR:
        data = sc.data_set(nexp, 40 + nexp)
        w = sc.edge_weights(nexp, 50 + nexp) if weighted else None
        _MIRROR[key] = (data, w, xcor.sysrem_reference(data, w, sc.SEG, ncomp, niter))
    return _MIRROR[key]


def program_is_the_mirror(check_exe, path, data, w, seg, ncomp, niter, want):
    """the program's U, coef and residuals of one set against the mirror's, bit for bit"""
    basis, coef, resid = want
    with open(path, "w") as f:
        f.write("%d %d %d %d %d\n%s\n" % (data.shape[0], ncomp, niter, len(seg) - 1, int(w is not None), " ".join(str(int(x)) for x in seg)))
        for arr in (data,) + ((w,) if w is not None else ()):
            f.write(" ".join(float(x).hex() for x in arr.reshape(-1)) + "\n")
    out = subprocess.run([check_exe, "set", str(path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout[-2000:] + out.stderr[-4000:]
    lines = {w_[0]: w_[1:] for w_ in (line.split() for line in out.stdout.splitlines())}
    assert "FAILED" not in lines
    got = {k: np.array([float.fromhex(x) for x in lines[k]]) for k in ("U", "coef", "r")}
    assert same_bits(got["U"].reshape(basis.shape), basis)
    assert same_bits(got["coef"].reshape(coef.shape), coef)
    assert same_bits(got["r"].reshape(resid.shape), resid)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ncomp,niter", [(3, 10), (16, 10)])
def test_the_programs_vectors_and_residuals_on_the_long_orders(check_exe, tmp_path, ncomp, niter, weighted):
    """many_cases.long_set: rows of 1024, 1025 and 2049 pixels -- four row steps of 256, four and one lane, eight and one lane --
    at the (ncomp, niter) of tests/test_gpu_long_orders.py"""
    ms = mc.long_set()[0]
    w = ms.weight if weighted else None
    want = xcor.sysrem_reference(ms.data, w, ms.seg_first, ncomp, niter)
    program_is_the_mirror(check_exe, tmp_path / "set.txt", ms.data, w, ms.seg_first, ncomp, niter, want)
    basis, coef, resid = want
    assert np.all(basis[2] == 0) and not np.signbit(basis[2]).any() and np.isfinite(basis).all() and np.isfinite(resid).all()
    assert np.all(np.any(basis[[0, 1, 3, 4], :, 0] != 0, axis=1))
    if weighted:
        k = ms.segment(ms.masked_seg)
        assert np.all(basis[ms.masked_seg, ms.masked_exp] == 0) and not np.signbit(basis[ms.masked_seg, ms.masked_exp]).any()
        assert np.array_equal(resid[ms.masked_exp, k], ms.data[ms.masked_exp, k])
        assert np.all(coef[:, ms.masked_col] == 0) and np.array_equal(resid[:, ms.masked_col], ms.data[:, ms.masked_col])


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("niter", [1, 2, 10])
@pytest.mark.parametrize("ncomp", [1, 3, 5])
@pytest.mark.parametrize("nexp", [7, 12])
def test_the_programs_vectors_and_residuals_are_the_mirrors_bit_for_bit(check_exe, tmp_path, nexp, ncomp, niter, weighted):
    data, w, (basis, coef, resid) = mirror(nexp, weighted, ncomp, niter)
    program_is_the_mirror(check_exe, tmp_path / "set.txt", data, w, sc.SEG, ncomp, niter, (basis, coef, resid))
    # the edges: the empty segment's vectors are zero; under the edge weights the masked exposure's a_v is +0 and its
    # residuals are the data, and the masked column keeps its data and a zero coefficient
    assert np.all(basis[5] == 0) and not np.signbit(basis[5]).any()
    assert np.isfinite(basis).all() and np.isfinite(resid).all()
    if weighted:
        k = slice(sc.SEG[sc.MASKED_SEG], sc.SEG[sc.MASKED_SEG + 1])
        assert np.all(basis[sc.MASKED_SEG, sc.MASKED_EXP] == 0) and not np.signbit(basis[sc.MASKED_SEG, sc.MASKED_EXP]).any()
        assert np.array_equal(resid[sc.MASKED_EXP, k], data[sc.MASKED_EXP, k])
        assert np.all(coef[:, sc.MASKED_COL] == 0) and np.array_equal(resid[:, sc.MASKED_COL], data[:, sc.MASKED_COL])
        assert np.count_nonzero(basis[sc.MASKED_SEG, :, 0]) == nexp - 1


@pytest.mark.parametrize("nexp,ncomp,niter", [(7, 3, 2), (12, 5, 10)])
def test_weights_none_are_weights_one(nexp, ncomp, niter):
    data, _, got = mirror(nexp, False, ncomp, niter)
    ones = xcor.sysrem_reference(data, np.ones_like(data), sc.SEG, ncomp, niter)
    for a, b in zip(got, ones):
        assert same_bits(a, b)


@pytest.mark.parametrize("weighted", [False, True])
def test_every_nonzero_vector_has_unit_length(weighted):
    """the tolerance of test_sysrem_basis_against_a_singular_vector"""
    for nexp, ncomp in ((7, 5), (12, 5)):
        basis = mirror(nexp, weighted, ncomp, 10)[2][0]
        norm = np.linalg.norm(basis, axis=1)                 # [nseg, ncomp]
        zero = np.all(basis == 0, axis=1)
        assert zero[5].all() and not zero[[1, 2, 3, 4, 6, 7]].any() and not zero[0, 0]
        assert np.all(np.abs(norm[~zero] - 1.0) < 1e-14)


def test_wave_sum_and_row_sum_orders():
    lanes = np.zeros(64)
    lanes[0], lanes[32], lanes[1] = 1.0, 2.0 ** 53, 1.0
    assert xcor.wave_sum(lanes) == 2.0 ** 53                 # (1 + 2^53 first: the partner is lane ^ 32)
    assert xcor.wave_sum(np.arange(64.0)) == 2016.0
    with pytest.raises(ValueError):
        xcor.wave_sum(np.zeros(63))
    # lane 0 adds the terms 0, 64, 128 in that order: (2^53 + 1) + 1 = 2^53, while 2^53 + (1 + 1) would be 2^53 + 2
    t = np.zeros(130)
    t[0], t[64], t[128] = 2.0 ** 53, 1.0, 1.0
    assert xcor.row_sum(t) == 2.0 ** 53
    t[0], t[128] = 1.0, 2.0 ** 53
    assert xcor.row_sum(t) == 2.0 ** 53 + 2.0
    assert xcor.row_sum(np.zeros(0)) == 0.0 and xcor.row_sum(np.ones((3, 200))).tolist() == [200.0] * 3


def prototype_set(seed=2, noise=1e-3, fall=0.3, npix=sc.NPIX):
    """7 exposures over the shared segments: six rank-one terms of falling size plus noise, 5 % masked entries"""
    rng = np.random.default_rng(seed)
    d = np.zeros((7, npix))
    for k in range(6):
        sign = 1 if k == 0 else rng.choice([-1, 1], npix)[None, :]
        d += fall ** k * rng.uniform(0.5, 1.5, 7)[:, None] * rng.uniform(0.5, 1.5, npix)[None, :] * sign
    d += noise * rng.standard_normal(d.shape)
    w = rng.uniform(0.5, 2.0, d.shape)
    w[rng.random(d.shape) < 0.05] = 0.0
    return d, w


@pytest.mark.parametrize("ncomp", [3, 5])
def test_the_mirror_against_sysrem_basis(ncomp):
    """The same algorithm in numpy's own summation order: the two differ by the rounding of the sums, amplified by the
    alternation.  On prototype_set() the largest difference over the segments of >= 7 pixels was measured at 2.3e-15
    (3 components) and 9.8e-15 (5 components); the bound 1e-11 leaves a factor above 1000 for another platform's
    summation order.  Left out: the empty segment, and the one-pixel segment from its second component on -- its residual
    there is rounding noise, and the two differ by order 1."""
    d, w = prototype_set()
    got = xcor.sysrem_reference(d, w, sc.SEG, ncomp, 10)[0]
    want = xcor.sysrem_basis(d, w, sc.SEG, ncomp, 10)
    diff = np.abs(got - want)
    worst = float(diff[[1, 2, 3, 4, 6, 7]].max())
    print("ncomp %d: largest |mirror - sysrem_basis| on the segments of >= 7 pixels %.2e, first component of the one-pixel segment %.2e"
          % (ncomp, worst, float(diff[0, :, 0].max())))
    assert worst < 1e-11
    assert float(diff[0, :, 0].max()) < 1e-11


@pytest.mark.parametrize("ncomp", [3, 5])
def test_the_mirror_against_sysrem_basis_on_the_long_orders(ncomp):
    """test_the_mirror_against_sysrem_basis' rule, 1e-11 on the segments of >= 7 pixels, at the lengths of many_cases.long_set:
    prototype_set's recipe over 4105 pixels in segments of 1024, 1025, 0, 2049 and 7.  The mirror's row sums take such a row
    in lanes of 17 and of 33 terms, numpy's pairwise: a mirror that dropped or doubled a row step would differ by order 1."""
    seg = xcor.segments(mc.LONG_LENGTHS)
    d, w = prototype_set(npix=int(seg[-1]))
    got = xcor.sysrem_reference(d, w, seg, ncomp, 10)[0]
    want = xcor.sysrem_basis(d, w, seg, ncomp, 10)
    diff = np.abs(got - want)
    worst = float(diff[[0, 1, 3, 4]].max())
    print("long orders, ncomp %d: largest |mirror - sysrem_basis| on the segments of >= 7 pixels %.2e" % (ncomp, worst))
    assert np.all(got[2] == 0) and np.all(want[2] == 0)
    assert worst < 1e-11


def test_injection_fixed_points():
    rng = np.random.default_rng(9)
    nexp, npix = 5, 40
    F = rng.standard_normal((nexp, npix))
    obs = xcor.Observed(xcor.segments([npix]), F, None, rng.uniform(0.5, 1.5, npix))
    pairs = np.stack([rng.uniform(0.5, 1.5, (nexp, npix)), rng.uniform(0.5, 1.5, (nexp, npix))], axis=-1)
    pairs[1, 3] = (0.0, 0.0)
    pairs[2, 7] = (1.0, 0.0)
    pairs[4, :5, 1] = 0.0
    out = xcor.inject_reference(pairs, obs, 1e-2, 1.0)
    dead = pairs[..., 1] <= 0
    assert dead.sum() == 7 and same_bits(out[dead], F[dead])
    assert np.all(out[~dead] != F[~dead])
    # p0 = 0, p1 = 1: m = 0 g + 1 = 1, F * 1 = F
    assert same_bits(xcor.inject_reference(pairs, obs, 0.0, 1.0), F)
    # the operations, one at a time
    g = obs.gain[None, :] * (pairs[..., 0] / np.where(dead, 1.0, pairs[..., 1]))
    m = 1e-2 * g
    m = m + 1.0
    assert same_bits(out[~dead], (F * m)[~dead])


def test_abi_struct_constant_symbol_and_kernels():
    assert ctypes.sizeof(_abi.TrxDetrend) == 32
    assert _abi.SYSREM_MAX_ITER == 64
    txt = open(os.path.join(ROOT, "include", "transit_hip.h")).read()
    assert "#define TRX_SYSREM_MAX_ITER 64" in txt
    path = build.lib_path("libtransit_hip.so")
    if not os.path.exists(path):
        build.build_hip()
    lib = ctypes.CDLL(path)
    assert hasattr(lib, "trx_detrend_observed")
    lib.trx_abi_version.restype = ctypes.c_int
    assert lib.trx_abi_version() == 5
    blob = open(path, "rb").read()
    for k in (b"k_sysrem_inject", b"k_sysrem_cols", b"k_sysrem_rows", b"k_sysrem_close", b"k_sysrem_subtract"):
        assert k in blob, k
    # refused without a handle, before anything is touched
    _abi.bind(lib, _abi.HIP_HEADER, "trx_")
    assert lib.trx_detrend_observed(None, None, None, None, 0, None, None, None, None, None, None, None) == -1
