"""The principal-component detrend of the observed set without a device: the refusals, the extents, the tournament
schedule, the Gram tiles and the arithmetic of transit_amd/csrc/trx_pca.h through tests/pca_check.cpp, a stand-alone program
over exact-size heap arrays under -fsanitize=address,undefined that walks a whole set the way the kernels do; its U, coef,
residuals, eigenvalues, offdiag and nwhole held bit for bit against xcor.pca_reference, the numpy mirror; the mirror's own
properties (the schedule, weights None = weights 1, orthonormal vectors, descending eigenvalues, convergence, the agreement
with xcor.svd_basis); and the ABI: the struct's size, the constants, the exported symbol and the kernels in the code
object."""
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
    return build_check("pca_check", tmp_path_factory.mktemp("pca_check"))


def test_refusals_extents_schedule_and_known_sets_under_sanitizers(check_exe):
    out = subprocess.run([check_exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stderr == ""                              # (no sanitizer report)
    lines = out.stdout.splitlines()
    last = lines[-1].split()
    assert last[0] == "ok" and int(last[1]) > 90, lines[-20:]
    assert not [line for line in lines if line.startswith("FAILED")]


@pytest.mark.parametrize("nexp", list(range(1, 14)) + [64, 65, 127, 128])
def test_the_schedule(nexp):
    rounds = xcor.jacobi_rounds(nexp)
    m = nexp + (nexp & 1)
    assert len(rounds) == m - 1
    seen = []
    for pairs in rounds:
        flat = [x for pq in pairs for x in pq]
        assert len(set(flat)) == len(flat)               # the pairs of a round are disjoint
        assert all(0 <= p < q < nexp for p, q in pairs)
        assert len(pairs) == (m // 2 if nexp == m else m // 2 - 1)
        seen += pairs
    assert sorted(seen) == [(p, q) for p in range(nexp) for q in range(p + 1, nexp)]      # every pair once a sweep


_MIRROR = {}


def mirror(nexp, weighted, ncomp, nsweep):
    """(data, weight, pca_reference's six) of the shared set, computed once per case"""
    key = (nexp, weighted, ncomp, nsweep)
    if key not in _MIRROR:
        data = sc.data_set(nexp, 40 + nexp)
        w = sc.edge_weights(nexp, 50 + nexp) if weighted else None
        _MIRROR[key] = (data, w, xcor.pca_reference(data, w, sc.SEG, ncomp, nsweep))
    return _MIRROR[key]


def run_program(check_exe, path, nexp, ncomp, nsweep, seg, data, w):
    with open(path, "w") as f:
        f.write("%d %d %d %d %d\n%s\n" % (nexp, ncomp, nsweep, len(seg) - 1, int(w is not None), " ".join(str(int(x)) for x in seg)))
        for arr in (data,) + ((w,) if w is not None else ()):
            f.write(" ".join(float(x).hex() for x in arr.reshape(-1)) + "\n")
    out = subprocess.run([check_exe, "set", str(path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout[-2000:] + out.stderr[-4000:]
    lines = {w_[0]: w_[1:] for w_ in (line.split() for line in out.stdout.splitlines())}
    assert "FAILED" not in lines
    got = {k: np.array([float.fromhex(x) for x in lines[k]]) for k in ("U", "coef", "r", "eigen", "offdiag")}
    got["nwhole"] = np.array([int(x) for x in lines["nwhole"]], dtype=np.int64)
    return got


def same_as_mirror(got, want):
    basis, coef, resid, eigen, offdiag, nwhole = want
    assert same_bits(got["U"].reshape(basis.shape), basis)
    assert same_bits(got["coef"].reshape(coef.shape), coef)
    assert same_bits(got["r"].reshape(resid.shape), resid)
    assert same_bits(got["eigen"].reshape(eigen.shape), eigen)
    assert same_bits(got["offdiag"], offdiag)
    assert np.array_equal(got["nwhole"], nwhole)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nsweep", [1, 2, 8])
@pytest.mark.parametrize("ncomp", [1, 3, 5])
@pytest.mark.parametrize("nexp", [7, 12])
def test_the_programs_results_are_the_mirrors_bit_for_bit(check_exe, tmp_path, nexp, ncomp, nsweep, weighted):
    data, w, want = mirror(nexp, weighted, ncomp, nsweep)
    same_as_mirror(run_program(check_exe, tmp_path / "set.txt", nexp, ncomp, nsweep, sc.SEG, data, w), want)
    basis, coef, resid, eigen, offdiag, nwhole = want
    # the edges: the empty segment's vectors are +0; under the edge weights the masked exposure has a +0 row in every vector
    # and its residuals are its data, and the masked column has zero coefficients
    assert np.all(basis[5] == 0) and not np.signbit(basis[5]).any() and np.all(eigen[5] == 0) and nwhole[5] == 0 and offdiag[5] == 0
    assert np.isfinite(basis).all() and np.isfinite(resid).all() and np.isfinite(coef).all()
    if weighted:
        k = slice(sc.SEG[sc.MASKED_SEG], sc.SEG[sc.MASKED_SEG + 1])
        assert np.all(basis[sc.MASKED_SEG, sc.MASKED_EXP] == 0) and not np.signbit(basis[sc.MASKED_SEG, sc.MASKED_EXP]).any()
        assert np.array_equal(resid[sc.MASKED_EXP, k], data[sc.MASKED_EXP, k])
        assert np.all(coef[:, sc.MASKED_COL] == 0) and np.array_equal(resid[:, sc.MASKED_COL], data[:, sc.MASKED_COL])
        on = w > 0
        for s in range(len(sc.LENGTHS)):
            a, b = sc.SEG[s], sc.SEG[s + 1]
            live = on[:, a:b].any(axis=1)
            assert nwhole[s] == np.count_nonzero(on[live, a:b].all(axis=0) & live.any())
        assert 0 < nwhole[7] < 400 and np.any(basis[7, :, 0] != 0)
    else:
        assert np.array_equal(nwhole, sc.LENGTHS) and np.all(np.any(basis[[0, 1, 2, 3, 4, 6, 7], :, 0] != 0, axis=1))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ncomp", [3, 5])
def test_the_programs_results_on_the_long_orders(check_exe, tmp_path, ncomp, weighted):
    """many_cases.long_set at the (ncomp, nsweep) of tests/test_gpu_long_orders.py: Gram rows and live counts over 1024, 1025
    and 2049 pixels"""
    ms = mc.long_set()[0]
    w = ms.weight if weighted else None
    want = xcor.pca_reference(ms.data, w, ms.seg_first, ncomp, 8)
    same_as_mirror(run_program(check_exe, tmp_path / "set.txt", ms.nexp, ncomp, 8, ms.seg_first, ms.data, w), want)
    basis, coef, resid, eigen, offdiag, nwhole = want
    assert np.all(basis[2] == 0) and not np.signbit(basis[2]).any() and np.all(eigen[2] == 0) and nwhole[2] == 0 and offdiag[2] == 0
    assert np.isfinite(basis).all() and np.isfinite(resid).all() and np.isfinite(coef).all()
    if weighted:
        k = ms.segment(ms.masked_seg)
        assert np.all(basis[ms.masked_seg, ms.masked_exp] == 0) and not np.signbit(basis[ms.masked_seg, ms.masked_exp]).any()
        assert np.array_equal(resid[ms.masked_exp, k], ms.data[ms.masked_exp, k])
        for s in mc.LONG_SEGS:
            assert 0 < nwhole[s] < ms.lengths[s] and np.any(basis[s, :, 0] != 0)
    else:
        assert np.array_equal(nwhole, ms.lengths) and np.all(np.any(basis[[0, 1, 3, 4], :, 0] != 0, axis=1))


def test_a_set_whose_every_column_has_a_hole(check_exe, tmp_path):
    nexp = 7
    data = sc.data_set(nexp, 3)
    w = np.ones_like(data)
    w[np.arange(sc.NPIX) % nexp, np.arange(sc.NPIX)] = 0.0          # one hole per column
    want = xcor.pca_reference(data, w, sc.SEG, 3, 2)
    basis, coef, resid, eigen, offdiag, nwhole = want
    # (the one-pixel segment apart: the exposure of its hole is not live there, so its column is whole)
    rest = [1, 2, 3, 4, 5, 6, 7]
    assert nwhole[0] == 1 and np.all(nwhole[rest] == 0) and np.all(basis[rest] == 0) and not np.signbit(basis[rest]).any() and np.all(eigen[rest] == 0)
    assert np.all(coef[:, 1:] == 0) and np.array_equal(resid[:, 1:], data[:, 1:])
    same_as_mirror(run_program(check_exe, tmp_path / "set.txt", nexp, 3, 2, sc.SEG, data, w), want)


@pytest.mark.parametrize("nexp,ncomp,nsweep", [(7, 3, 2), (12, 5, 8)])
def test_weights_none_are_weights_one(nexp, ncomp, nsweep):
    data, _, got = mirror(nexp, False, ncomp, nsweep)
    ones = xcor.pca_reference(data, np.ones_like(data), sc.SEG, ncomp, nsweep)
    for a, b in zip(got, ones):
        assert same_bits(a, b)


def prototype_set(nexp=7, seed=2, noise=1e-3, fall=0.3, npix=sc.NPIX):
    """test_sysrem_host.prototype_set's recipe without its weights: six rank-one terms of falling size plus noise"""
    rng = np.random.default_rng(seed)
    d = np.zeros((nexp, npix))
    for k in range(6):
        sign = 1 if k == 0 else rng.choice([-1, 1], npix)[None, :]
        d += fall ** k * rng.uniform(0.5, 1.5, nexp)[:, None] * rng.uniform(0.5, 1.5, npix)[None, :] * sign
    d += noise * rng.standard_normal(d.shape)
    return d


def signed(basis):
    """the sign rule of trx_pca_observed applied to vectors [nseg, nexp, ncomp]"""
    out = basis.copy()
    for s in range(out.shape[0]):
        for i in range(out.shape[2]):
            col = out[s, :, i]
            if col[int(np.argmax(np.abs(col)))] < 0:
                out[s, :, i] = 0.0 - col
    return out


_TEN = {}


def ten_sweeps(nexp):
    """offdiag / eigen[:, 0] per segment of prototype_set(nexp) after 10 sweeps (they do not depend on ncomp), computed once"""
    if nexp not in _TEN:
        _, _, _, eigen, offdiag, _ = xcor.pca_reference(prototype_set(nexp), None, sc.SEG, 1, 10)
        _TEN[nexp] = offdiag / np.where(eigen[:, 0] > 0, eigen[:, 0], 1.0)
    return _TEN[nexp]


SVD_BOUND = {1: 2e-12, 3: 1e-10, 5: 4e-8}
ONE_PIXEL_BOUND = 2.5e-13


@pytest.mark.parametrize("nexp", [7, 12, 101])
@pytest.mark.parametrize("ncomp", [1, 3, 5])
def test_the_mirror_against_svd_basis(nexp, ncomp):
    """The Gram route after 8 sweeps against numpy's SVD of the same unweighted data, both under the sign rule.  The error of
    component k grows as (sigma_1 / sigma_k)^2 eps.  On prototype_set() at 7, 12 and 101 exposures the largest difference
    over the segments of >= 7 pixels was measured on the CPU at 2.0e-15 (1 component), 1.2e-13 (3 components) and 3.8e-11
    (5 components), and at 2.2e-16 on the first component of the one-pixel segment; the bounds 2e-12, 1e-10, 4e-8 and
    2.5e-13 leave a factor of about 1000 for another platform's LAPACK.  Left out: the empty segment, and the one-pixel
    segment beyond its first component (it has one singular vector).

    Convergence, asserted on EVERY segment of every case.  After 8 sweeps offdiag <= 1e-12 eigen[:, 0] holds and is
    asserted at 7 and 12 exposures on all segments (measured: <= 1e-19) and at 101 exposures on the segments of 1, 0, 7, 200
    and 400 pixels (1e-21, 0, 2e-19, 3.0e-14, 2.1e-15).  The three segments of 63, 64 and 65 pixels at 101 exposures do
    not: 8 sweeps leave 9.0e-13, 3.4e-11 and 1.2e-12 of eigen[:, 0] there (the first meets 1e-12 by a tenth only and is
    held with its two neighbours).  The cause is a crowded spectrum -- dozens of noise
    eigenvalues close together (beside the nexp - npix null ones here; on the device a full-rank 40 x 2048 set of 100
    exposures with 95 close noise eigenvalues leaves 1.4e-11 likewise), which delays the quadratic phase of the leading
    block against them.  Those three are asserted at 3.4e-8, the measured 3.4e-11 with the same factor of 1000 as the
    bounds above, and every segment of every case is asserted at the issue's 1e-12 after 10 sweeps, where the measured
    worst is 3e-16 (5e-18, 3e-16 and 3e-18 on the three)."""
    d = prototype_set(nexp)
    got, _, _, eigen, offdiag, _ = xcor.pca_reference(d, None, sc.SEG, ncomp, 8)
    want = signed(xcor.svd_basis(d, sc.SEG, ncomp))
    diff = np.abs(got - want)
    big = [1, 2, 3, 4, 6, 7]
    worst = float(diff[big].max())
    print("nexp %d, ncomp %d: largest |mirror - svd_basis| on the segments of >= 7 pixels %.2e, first component of the one-pixel segment %.2e"
          % (nexp, ncomp, worst, float(diff[0, :, 0].max())))
    assert worst < SVD_BOUND[ncomp]
    assert float(diff[0, :, 0].max()) < ONE_PIXEL_BOUND
    # 8 sweeps have converged; the vectors are orthonormal; the eigenvalues descend
    rel = offdiag / np.where(eigen[:, 0] > 0, eigen[:, 0], 1.0)
    crowded = np.array([nexp == 101 and n in (63, 64, 65) for n in sc.LENGTHS])
    rel10 = ten_sweeps(nexp)
    print("nexp %d: offdiag / eigen[:, 0] per segment after 8 sweeps: %s\n          after 10 sweeps: %s"
          % (nexp, np.array2string(rel, precision=2), np.array2string(rel10, precision=2)))
    assert np.all(rel[~crowded] <= 1e-12) and np.all(rel[crowded] <= 3.4e-8)
    assert np.all(rel10 <= 1e-12)
    for s in range(len(sc.LENGTHS)):
        u = got[s][:, np.any(got[s] != 0, axis=0)]               # the non-zero vectors (all of them on the segments of >= 7 pixels)
        assert u.shape[1] == ncomp or s not in big
        assert u.shape[1] == 0 or np.max(np.abs(u.T @ u - np.eye(u.shape[1]))) < 1e-13
    assert np.all(np.diff(eigen, axis=1) <= 0)


@pytest.mark.parametrize("nexp", [7, 12])
@pytest.mark.parametrize("ncomp", [1, 3, 5])
def test_the_mirror_against_svd_basis_on_the_long_orders(nexp, ncomp):
    """test_the_mirror_against_svd_basis' rules -- SVD_BOUND on the segments of >= 7 pixels, offdiag <= 1e-12 eigen[:, 0] after
    8 sweeps, orthonormal vectors, descending eigenvalues -- at the lengths of many_cases.long_set: prototype_set's recipe
    over 4105 pixels in segments of 1024, 1025, 0, 2049 and 7.  The Gram matrix's row sums take such a row in lanes of 17 and
    of 33 terms; numpy's SVD knows nothing of either."""
    seg = xcor.segments(mc.LONG_LENGTHS)
    d = prototype_set(nexp, npix=int(seg[-1]))
    got, _, _, eigen, offdiag, nwhole = xcor.pca_reference(d, None, seg, ncomp, 8)
    want = signed(xcor.svd_basis(d, seg, ncomp))
    big = [0, 1, 3, 4]
    worst = float(np.abs(got - want)[big].max())
    rel = offdiag / np.where(eigen[:, 0] > 0, eigen[:, 0], 1.0)
    print("long orders, nexp %d, ncomp %d: largest |mirror - svd_basis| %.2e; offdiag / eigen[:, 0] per segment after 8 sweeps: %s"
          % (nexp, ncomp, worst, np.array2string(rel, precision=2)))
    assert np.array_equal(nwhole, mc.LONG_LENGTHS) and np.all(got[2] == 0)
    assert worst < SVD_BOUND[ncomp]
    assert np.all(rel <= 1e-12)
    for s in big:
        u = got[s]
        assert np.all(np.any(u != 0, axis=0)) and np.max(np.abs(u.T @ u - np.eye(ncomp))) < 1e-13
    assert np.all(np.diff(eigen, axis=1) <= 0)


def test_abi_struct_constants_symbol_and_kernels():
    assert ctypes.sizeof(_abi.TrxPca) == 32
    assert _abi.PCA_MAX_SWEEP == 32 and _abi.PCA_MAX_EXP == 128
    txt = open(os.path.join(ROOT, "include", "transit_hip.h")).read()
    assert "#define TRX_PCA_MAX_SWEEP 32" in txt and "#define TRX_PCA_MAX_EXP   128" in txt
    path = build.lib_path("libtransit_hip.so")
    if not os.path.exists(path):
        build.build_hip()
    lib = ctypes.CDLL(path)
    assert hasattr(lib, "trx_pca_observed")
    lib.trx_abi_version.restype = ctypes.c_int
    assert lib.trx_abi_version() == 5
    blob = open(path, "rb").read()
    for k in (b"k_pca_live", b"k_pca_whole", b"k_pca_gram", b"k_pca_jacobi", b"k_pca_project"):
        assert k in blob, k
    # refused without a handle, before anything is touched
    _abi.bind(lib, _abi.HIP_HEADER, "trx_")
    assert lib.trx_pca_observed(None, None, None, None, 0, None, None, None, None, None, None, None, None, None, None) == -1
