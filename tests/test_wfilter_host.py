"""The weighted detrending filter without a device: the refusals, the layout, the extents and the per-column arithmetic of
transit_amd/csrc/trx_wfilter.h through tests/wfilter_check.cpp, a stand-alone program over exact-size heap arrays under
-fsanitize=address,undefined that walks a whole set the way the kernels do; its factors, flags and values held bit for bit
against xcor.weighted_factor and xcor.weighted_filter_reference, the numpy mirror; the mirror held against the same
projection in long double within xcor.weighted_filter_bound (derived in its docstring); the SYSREM basis against a singular
vector; and the ABI: the struct's size, the pivot constant and the exported symbols."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from bits import same_bits
from host_check import build_check

import wfilter_cases as wc
from transit_amd import _abi, build, xcor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = [1, 65, 0, 30]                         # a tile of one lane, 64 + 1, an empty segment, an ordinary one
MASKED, SHORT, EXACT = 70, 75, 80                # edge columns, in the last segment


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return build_check("wfilter_check", tmp_path_factory.mktemp("wfilter_check"))


def test_refusals_extents_layout_and_known_columns_under_sanitizers(check_exe):
    out = subprocess.run([check_exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stderr == ""                              # (no sanitizer report)
    lines = out.stdout.splitlines()
    last = lines[-1].split()
    assert last[0] == "ok" and int(last[1]) > 100, lines[-20:]
    assert not [line for line in lines if line.startswith("FAILED")]


def the_set(nexp, ncomp, seed):
    """(obs, wf, pairs): a gain-free observed set over LENGTHS with the edge weights, a random basis, and pairs (g, 1)"""
    rng = np.random.default_rng(seed)
    npix = sum(LENGTHS)
    g = 1.0 + 0.1 * rng.standard_normal((nexp, npix))
    w = wc.edge_weights(nexp, npix, ncomp, MASKED, SHORT, EXACT, seed + 1, scattered=0.2)
    obs = xcor.Observed(xcor.segments(LENGTHS), rng.standard_normal((nexp, npix)), w)
    wf = xcor.WeightedFilter(wc.random_basis(obs.nseg, nexp, ncomp, seed + 2))
    return obs, wf, np.stack([g, np.ones_like(g)], axis=-1)


@pytest.mark.parametrize("nexp,ncomp", [(7, 1), (7, 3), (7, 5), (7, 9), (12, 4), (12, 8), (12, 9), (20, 16)])
def test_the_programs_factor_and_values_are_the_mirrors_bit_for_bit(check_exe, tmp_path, nexp, ncomp):
    """every padding the program runs (the layout's and the wider ones) agrees with itself there; here its narrowest
    one against numpy: the live flags, L and D of the live columns and of the dead ones up to the singular pivot's
    row (nan for nan beyond), and the values with their NaN pattern"""
    obs, wf, pairs = the_set(nexp, ncomp, 100 * nexp + ncomp)
    live = wc.decisive(obs, wf)
    path = tmp_path / "set.txt"
    with open(path, "w") as f:
        f.write("%d %d %d\n%s\n" % (nexp, ncomp, obs.nseg, " ".join(str(int(x)) for x in obs.seg_first)))
        for arr in (wf.basis, obs.weight, pairs[..., 0]):
            f.write(" ".join(float(x).hex() for x in arr.reshape(-1)) + "\n")
    out = subprocess.run([check_exe, "set", str(path)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout[-2000:] + out.stderr[-4000:]
    lines = [line.split() for line in out.stdout.splitlines()]
    assert not [w for w in lines if w[0] == "FAILED"]
    rows = [w for w in lines if w[0] == "col"]
    nfac = ncomp * (ncomp + 1) // 2
    assert len(rows) == obs.npix and all(len(w) == 3 + nfac + nexp for w in rows)
    got_live = np.array([int(w[2]) for w in rows], dtype=bool)
    got_fac = np.array([[float.fromhex(x) for x in w[3:3 + nfac]] for w in rows])
    got_val = np.array([[float.fromhex(x) for x in w[3 + nfac:]] for w in rows]).T
    L, D, _ = xcor.weighted_factor(obs, wf)
    want_fac = np.zeros((obs.npix, nfac))
    for j in range(ncomp):
        for k in range(j + 1):
            want_fac[:, j * (j + 1) // 2 + k] = D[:, j] if k == j else L[:, j, k]
    assert np.array_equal(got_live, live)
    assert same_bits(got_fac, want_fac)
    ref = xcor.weighted_filter_reference(pairs, obs, wf)
    assert same_bits(got_val, ref)
    assert np.array_equal(np.isnan(ref).all(axis=0), ~live) and not np.isnan(ref[:, live]).any()
    # the edge columns
    assert not live[MASKED] and not live[SHORT] and bool(live[EXACT]) == (ncomp <= nexp)
    if ncomp <= nexp:
        assert np.count_nonzero(live) >= obs.npix - 6 and live[0] and live[65]
        assert np.count_nonzero((obs.weight == 0)[:, live]) > 5      # masked entries in live columns
    else:
        assert not live.any()


@pytest.mark.parametrize("nexp,ncomp", [(7, 1), (7, 3), (7, 5), (40, 1), (40, 3), (40, 5), (40, 9), (40, 16)])
def test_the_mirror_against_long_double(nexp, ncomp):
    """orthonormal bases from svd_basis, weights that vary by a factor of 100 along every column: |mirror - exact| within
    weighted_filter_bound, element by element"""
    rng = np.random.default_rng(7 * nexp + ncomp)
    lengths = [40, 100, 25]
    npix = sum(lengths)
    seg = xcor.segments(lengths)
    data = rng.standard_normal((nexp, npix)) + np.linspace(0.5, 1.5, nexp)[:, None] * np.linspace(1.0, 2.0, npix)[None, :]
    w = 10.0 ** rng.uniform(-1.0, 1.0, (nexp, npix))
    for p in range(npix):
        a, z = rng.permutation(nexp)[:2]
        w[a, p], w[z, p] = 0.1, 10.0
    assert np.all(w.max(axis=0) / w.min(axis=0) == 100.0)
    obs = xcor.Observed(seg, data, w, rng.uniform(0.5, 1.5, npix))
    basis = xcor.svd_basis(data, seg, ncomp)
    for s in range(3):
        assert np.max(np.abs(basis[s].T @ basis[s] - np.eye(ncomp))) < 1e-13
    wf = xcor.WeightedFilter(basis)
    a = 1.0 + 0.05 * rng.standard_normal((nexp, npix))
    pairs = np.stack([a * 3.0, np.full_like(a, 3.0)], axis=-1)
    live = wc.decisive(obs, wf)
    assert live.all()
    mirror, exact, bound = (f(pairs, obs, wf) for f in (xcor.weighted_filter_reference, xcor.weighted_filter_exact, xcor.weighted_filter_bound))
    assert not np.isnan(mirror).any() and not np.isnan(exact).any() and np.all(bound > 0)
    g = obs.gain[None, :] * (pairs[..., 0] / pairs[..., 1])
    err = np.abs(mirror - exact)
    rel = float(np.max(err / np.max(np.abs(g), axis=0)[None, :]))
    print("nexp %d, ncomp %d: largest |mirror - exact| %.3e of the column's max |g| (%.2f * 2^-52), %.4f of the bound"
          % (nexp, ncomp, rel, rel / 2.0 ** -52, float(np.max(err / bound))))
    assert np.all(err <= bound)
    # and the projection is one: the filtered values are orthogonal to the basis under the column's weights
    for s in range(3):
        k = slice(seg[s], seg[s + 1])
        resid = np.einsum("vj,vp->jp", basis[s], w[:, k] * mirror[:, k])
        scale = np.einsum("vj,vp->jp", np.abs(basis[s]), w[:, k] * np.abs(g[:, k]))
        assert np.max(np.abs(resid) / scale) < 1e-13


def test_equal_weights_are_the_plain_filter():
    """with all weights equal and an orthonormal basis the projector is U U^T: the plain filter of svd_filter"""
    rng = np.random.default_rng(5)
    seg = xcor.segments([30, 50])
    data = rng.standard_normal((9, 80))
    obs = xcor.Observed(seg, data, np.full((9, 80), 0.75))
    F = xcor.svd_filter(data, seg, 3)
    wf = xcor.WeightedFilter(xcor.svd_basis(data, seg, 3))
    assert np.array_equal(wf.basis, F.back)
    g = 1.0 + 0.1 * rng.standard_normal((9, 80))
    pairs = np.stack([g, np.ones_like(g)], axis=-1)
    plain, weighted = xcor.filter_reference(pairs, obs, F), xcor.weighted_filter_reference(pairs, obs, wf)
    tol = xcor.weighted_filter_bound(pairs, obs, wf) + (9 + 3 + 8) * 2.0 ** -52 * xcor.filter_abs_reference(pairs, obs, F)
    assert np.all(np.abs(plain - weighted) <= tol)
    # one masked entry: that column's values move, by far more than rounding; the others keep their bits
    w = obs.weight.copy()
    w[4, 17] = 0.0
    masked = xcor.weighted_filter_reference(pairs, xcor.Observed(seg, data, w), wf)
    assert np.all(np.abs(masked[:, 17] - weighted[:, 17]) > 1e-6)
    keep = np.arange(80) != 17
    assert np.array_equal(masked[:, keep], weighted[:, keep])


def test_sysrem_basis_against_a_singular_vector():
    """unit weights, one component, a matrix with a clear singular-value gap: the leading left singular vector up to sign"""
    rng = np.random.default_rng(3)
    nexp, lengths = 12, [60, 0, 45]
    seg = xcor.segments(lengths)
    data = np.zeros((nexp, sum(lengths)))
    for s in (0, 2):
        a, c = rng.uniform(0.5, 1.5, nexp), rng.uniform(0.5, 1.5, lengths[s])
        data[:, seg[s]:seg[s + 1]] = 10.0 * a[:, None] * c[None, :] + 0.01 * rng.standard_normal((nexp, lengths[s]))
    got = xcor.sysrem_basis(data, None, seg, 1, niter=20)
    assert got.shape == (3, nexp, 1) and np.all(got[1] == 0)
    for s in (0, 2):
        u, sv, _ = np.linalg.svd(data[:, seg[s]:seg[s + 1]], full_matrices=False)
        assert sv[0] > 100 * sv[1]
        sign = np.sign(u[:, 0] @ got[s, :, 0])
        assert abs(np.linalg.norm(got[s, :, 0]) - 1.0) < 1e-14
        assert np.max(np.abs(sign * u[:, 0] - got[s, :, 0])) < 1e-12
    assert np.array_equal(xcor.sysrem_basis(data, np.ones_like(data), seg, 1, niter=20), got)
    # several components under weights with masked entries: unit vectors that a weighted filter can take
    w = rng.uniform(0.5, 2.0, data.shape)
    w[rng.random(data.shape) < 0.05] = 0.0
    two = xcor.sysrem_basis(data, w, seg, 2, niter=10)
    assert np.allclose(np.linalg.norm(two[[0, 2]], axis=1), 1.0, atol=1e-14)
    obs = xcor.Observed(xcor.segments([60, 45]), data, w)
    L, D, live = xcor.weighted_factor(obs, xcor.WeightedFilter(two[[0, 2]]))
    assert live.all()


def test_abi_struct_constant_and_symbols():
    assert ctypes.sizeof(_abi.TrxWfilter) == 16
    assert _abi.WFILTER_PIVOT == 2 ** -26
    txt = open(os.path.join(ROOT, "include", "transit_hip.h")).read()
    assert "#define TRX_WFILTER_PIVOT 0x1p-26" in txt
    path = build.lib_path("libtransit_hip.so")
    if not os.path.exists(path):
        build.build_hip()
    lib = ctypes.CDLL(path)
    for name in ("trx_set_weighted_filter", "trx_batch_set_weighted_filter"):
        assert hasattr(lib, name), name
    lib.trx_abi_version.restype = ctypes.c_int
    assert lib.trx_abi_version() == 5
    assert ctypes.sizeof(_abi.TrxFilter) == 24
    blob = open(path, "rb").read()
    for k in (b"k_wfilter_factor", b"k_pixel_wfilter", b"k_cell_wfilter"):
        assert k in blob, k
    # refused without a handle, before anything is touched
    _abi.bind(lib, _abi.HIP_HEADER, "trx_")
    assert lib.trx_set_weighted_filter(None, None, None) == -1
    assert lib.trx_batch_set_weighted_filter(None, None) == -1
