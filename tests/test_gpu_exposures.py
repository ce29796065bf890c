"""The exposure table on the device (trx_set_exposures / trx_run_exposed and the batch forms, include/transit_hip.h): a
scale and a Doppler-smear half-width per exposure, applied in the pixel stage, against transit_amd.exposures, the numpy
statement of the same definition.

The case is pixel_cases.make's (6001 bins, 60 layers), the exposures its seven shifts, the pixels three sets of 400: its
set A (lane windows of 42-44 bins), its set B (wave windows of 283-290 bins) and a set C at R = 4575 whose plain windows are
186-190 bins, so that the smear carries some exposures over kPixWaveFrom = 192 bins and others not; three segments, one
per set.  smear = [0, 2e-9, 1e-6, 3e-6, 1.3e-5, 0, 1e-5], scale = [1, 0.5, 0, -0.25, 1, 3, 1e-3].

Tolerance of the accuracy checks, per component, relative: pixel_cases.tolerance + E * n_max * wn_d / (4 d_min) over the
rows with eta > 0: the sum of the weights is about 4 d / wn_d, each of the n_max weights carries an absolute error of at
most E = 2^-50 -- the host's and the device's erf within 2^-51 each (the host's is within 1.5 ulp(1) of 40-digit
arithmetic; the device's is what test_the_weight_itself measures)."""
import ctypes as C

import numpy as np
import pytest

import pixel_cases as pc
import xcor_checks as xc
from transit_amd import _abi, bands, exposures, pixels, xcor
from transit_amd.engine import Batch, Engine, EngineError

pytestmark = pytest.mark.gpu

SHIFTS = pc.SHIFTS
LENGTHS = [400, 400, 400]
WAVE_FROM = 192                                  # kPixWaveFrom
E_ERF = 2.0 ** -50
EPS = 2.0 ** -52


def table():
    return exposures.Exposures(xc.SCALE, xc.SMEAR)


def set_c(P):
    """400 pixels at R = 4575: plain windows of 186-190 bins, below kPixWaveFrom until the smear widens them"""
    wn_d = float(P.static.wn_d)
    return pixels.resolving_power(np.linspace(2510, 2550, 400) + 0.37 * wn_d, 4575.0, 4.0)


def pixel_set(P):
    return pc.joined(pc.set_a(P), pc.set_b(P), set_c(P))


def windows(P, px, shifts, ex):
    """[nexp, npix] whole-grid window lengths by exposures.exposed_range, and the smallest distance (in bins) of a window
    edge from a grid point"""
    wn_i, wn_d, n, _ = pc.grid(P)
    lens, margin = np.zeros((len(shifts), len(px)), dtype=np.int64), np.inf
    for v, s in enumerate(shifts):
        eta = ex.eta(v)
        for p in range(len(px)):
            centre, fwhm = float(px.centre[p]) / float(s), float(px.fwhm[p]) / float(s)
            a, z = exposures.exposed_range(wn_i, wn_d, n, centre, fwhm, px.cut, eta)
            lens[v, p] = z - a
            r = px.cut * (fwhm / bands.FWHM_PER_SIGMA) + (centre * eta if eta > 0 else 0.0)
            for edge in ((centre - r - wn_i) / wn_d, (centre + r - wn_i) / wn_d):
                margin = min(margin, abs(edge - round(edge)))
    return lens, margin


def tolerance(P, px, shifts, ex, lens):
    wn_d = float(P.static.wn_d)
    smeared = [v for v in range(len(shifts)) if ex.eta(v) > 0]
    d_min = min(float(np.min(px.centre)) / float(shifts[v]) * ex.eta(v) for v in smeared)
    return pc.tolerance(px, shifts) + E_ERF * int(lens[smeared].max()) * wn_d / (4.0 * d_min)


def check_sums(mom, ref, scale, ob, what=""):
    """moments against the reference's and the sums of its absolute terms, with xcor_checks.check_moments' bound: the count exactly,
    every other moment within (n_max + 16) * 2^-52 of the scale (exactly where the scale is 0)"""
    assert mom.shape == ref.shape == scale.shape
    assert np.array_equal(mom[..., 0], ref[..., 0]), what
    tol = (int(np.max(np.diff(ob.seg_first))) + 16) * EPS
    err, size = np.abs(mom - ref)[..., 1:], scale[..., 1:]
    worst = float(np.max(err[size > 0] / size[size > 0]))
    print("%s: worst |mom - ref| / abs_ref %.3e = %.2f * 2^-52 (tolerance %.3e); %d sums of scale 0" % (what, worst, worst / EPS, tol, np.count_nonzero(size == 0)))
    assert np.all(err <= tol * size), (what, worst, tol)


def handle(P, px, ob=None, ex=None):
    E = Engine(P.static)
    E.set_pixels(px)
    if ob is not None:
        E.set_observed(ob)
    if ex is not None:
        E.set_exposures(ex)
    return E


class Case:
    pass


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """the eclipse case at 20 000 lines, the 1200 pixels, the observed set of 7 exposures by 3 segments, the table, the
    window lengths, and -- made once, shared and left unchanged -- the spectrum, the plain pairs and the exposed pairs"""
    c = Case()
    c.P = pc.make(tmp_path_factory.mktemp("exposures"), "eclipse", nlines=20_000)
    c.px, c.ex = pixel_set(c.P), table()
    c.lens, c.margin = windows(c.P, c.px, SHIFTS, c.ex)
    plain = Engine(c.P.static)
    c.spec = plain.run(c.P.atm, c.P.opts)["spectrum"]
    plain.close()
    c.ob = xc.observed(len(c.px), float(np.mean(c.spec)), lengths=LENGTHS)
    E = handle(c.P, c.px, c.ob)
    c.plain = E.run_pixels(c.P.atm, c.P.opts, SHIFTS)
    E.set_exposures(c.ex)
    c.pairs = E.run_exposed(c.P.atm, c.P.opts, SHIFTS)
    E.close()
    for a in (c.spec, c.plain, c.pairs):
        a.flags.writeable = False
    return c


def test_the_three_sets_take_both_forms_in_one_call(case):
    P, px = case.P, case.px
    plain_lens, plain_margin = windows(P, px, SHIFTS, exposures.Exposures(smear=np.zeros(7)))
    a, b, c = plain_lens[:, :400], plain_lens[:, 400:800], plain_lens[:, 800:]
    assert 42 <= a.min() and a.max() <= 44 and 283 <= b.min() and b.max() <= 290 and 186 <= c.min() and c.max() <= 190
    assert np.array_equal(plain_lens, np.array(pc.window_lengths_and_margin(P, px, SHIFTS)[0]).reshape(7, -1))
    assert min(case.margin, plain_margin) >= 1e-6, (case.margin, plain_margin)
    lens = case.lens
    # set C: lanes without smear, the wave at eta = 1.3e-5, and both forms in the one row at eta = 1e-5
    assert np.all(lens[[0, 1, 2, 3, 5], 800:] < WAVE_FROM) and np.all(lens[4, 800:] >= WAVE_FROM)
    assert np.any(lens[6, 800:] < WAVE_FROM) and np.any(lens[6, 800:] >= WAVE_FROM)
    assert np.all(lens[:, :400] < WAVE_FROM) and np.all(lens[:, 400:800] >= WAVE_FROM)
    assert np.all(lens[[4, 6]] > plain_lens[[4, 6]]) and np.array_equal(lens[[0, 5]], plain_lens[[0, 5]])


# ---- 1. accuracy -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solution", ["eclipse", "transit"])
def test_exposed_pairs_are_the_definition(tmp_path, solution):
    P = pc.make(tmp_path, solution)
    assert P.nwn == 6001
    wn_i, wn_d, n, _ = pc.grid(P)
    px, ex = pixel_set(P), table()
    lens, margin = windows(P, px, SHIFTS, ex)
    assert margin >= 1e-6
    tol = tolerance(P, px, SHIFTS, ex, lens)
    assert pc.tolerance(px, SHIFTS) < tol < 2e-10
    plain = Engine(P.static)
    ob = xc.observed(len(px), 1.0, lengths=LENGTHS)
    E = handle(P, px, ob, ex)
    deep, keep = pc.thinner(P, 1e-3)
    refs = {}
    for k, atm in enumerate((P.atm, P.atm, deep, P.atm)):      # fresh, hinted, resuming deeper, hinted again
        what = "%s run %d" % (solution, k)
        out, spec = E.run_exposed(atm, P.opts, SHIFTS, spectrum=True)
        assert out.shape == (7, len(px), 2)
        assert np.array_equal(spec, plain.run(atm, P.opts)["spectrum"]), what      # 2c. the spectrum is run()'s
        key = spec.tobytes()
        if key not in refs:
            refs[key] = exposures.reference(spec, wn_i, wn_d, n, px, SHIFTS, ex)
        pc.check_close(out, refs[key], tol, what + " vs reference")
        assert np.all(out[..., 1] > 0) and np.all(out[2, :, 0] == 0)
    assert len(refs) == 2
    plain.close(); E.close()


# ---- 2. bit identities ------------------------------------------------------------------------------------------
def test_rows_without_smear_are_the_plain_rows(case):
    P, px = case.P, case.px
    # eta == 0 and scale 1 (exposure 0), and every row of a table of zeros and ones
    assert np.array_equal(case.pairs[0], case.plain[0])
    E = handle(P, px, case.ob)
    for ex in (exposures.Exposures(np.ones(7), np.zeros(7)), exposures.Exposures(smear=np.zeros(7)), exposures.Exposures(scale=np.ones(7))):
        E.set_exposures(ex)
        assert np.array_equal(E.run_exposed(P.atm, P.opts, SHIFTS), case.plain)
    # smear = NULL: b is the plain b, a the one product
    E.set_exposures(exposures.Exposures(scale=xc.SCALE))
    got, spec = E.run_exposed(P.atm, P.opts, SHIFTS, spectrum=True)
    assert np.array_equal(got[..., 1], case.plain[..., 1])
    assert np.array_equal(got[..., 0], xc.SCALE[:, None] * case.plain[..., 0])
    assert np.array_equal(spec, case.spec)
    # eta == 0 with a scale (exposure 5): the same
    assert np.array_equal(case.pairs[5, :, 1], case.plain[5, :, 1]) and np.array_equal(case.pairs[5, :, 0], 3.0 * case.plain[5, :, 0])
    # eta > 0 moves the bits, b included
    for v in (1, 2, 3, 4, 6):
        assert np.all(case.pairs[v, :, 1] != case.plain[v, :, 1]), v
    E.close()


# ---- 3. the weight itself ---------------------------------------------------------------------------------------
def test_the_weight_itself(case):
    """One-bin windows: cut = 6 and sigma = 0.9 wn_d / 12, centres 0 to 0.45 bins off a grid point, d <= 0.04 wn_d, so that b
    is the weight W of that bin and a its one product with S_i.  |b - W_host| must be within E = 2^-50; measured on an
    MI355X: 2.22e-16 = 1.0 * 2^-52 at the worst (1.5 * 2^-52 with the farthest centres at 0.44 bins and an exposure
    without smear), so E stands as derived.
    (a == b * S_i in the same bits: a is that one product, rounded once.  a / b is S_i to an ulp, not always in the same
    bits: a quotient of a rounded product by its factor need not return the other factor.)"""
    P = case.P
    wn_i, wn_d, n, wn = pc.grid(P)
    sigma = 0.9 * wn_d / 12.0
    bins = np.arange(300, 5700, 27)
    off = np.linspace(0.0, 0.45, bins.size) * np.where(np.arange(bins.size) % 2, -1.0, 1.0)
    px = pixels.Pixels(wn[bins] + off * wn_d, np.full(bins.size, sigma * bands.FWHM_PER_SIGMA), 6.0)
    etas = np.array([1e-9, 3e-9, 1e-8, 3e-8, 6e-8, 1e-7, 1.5e-7])      # (all above 0: at eta == 0 the farthest centre's edge is a grid point)
    assert float(np.max(px.centre)) * etas.max() <= 0.04 * wn_d
    ex = exposures.Exposures(smear=etas)
    shifts = np.ones(7)
    lens, margin = windows(P, px, shifts, ex)
    assert np.all(lens == 1) and margin >= 1e-6
    ob = xcor.Observed(xcor.segments([len(px)]), np.ones((7, len(px))))
    E = handle(P, px, ob, ex)
    out = E.run_exposed(P.atm, P.opts, shifts)
    E.close()
    S = case.spec[bins]
    q = (px.fwhm / bands.FWHM_PER_SIGMA) * exposures.SQRT2      # (sigma as the device makes it: fwhm' / (2 sqrt(2 ln 2)))
    worst = 0.0
    for v in range(7):
        x = wn[bins] - px.centre
        d = px.centre * etas[v]
        W = exposures._erf((x + d) / q) - exposures._erf((x - d) / q)
        worst = max(worst, float(np.max(np.abs(out[v, :, 1] - W))))
        assert np.all(out[v, :, 1] > 0)
    print("worst |b - W_host| %.3e = %.3f * 2^-52 (E = 2^-50 = %.3e)" % (worst, worst / EPS, E_ERF))
    assert worst <= E_ERF
    assert np.array_equal(out[..., 0], out[..., 1] * S[None, :])
    assert np.max(np.abs(out[..., 0] / out[..., 1] - S[None, :]) / S[None, :]) <= EPS


# ---- 4. downstream ----------------------------------------------------------------------------------------------
def test_moments_filter_and_highpass_take_the_exposed_pairs(case):
    P, px, ob, pairs = case.P, case.px, case.ob, case.pairs
    E = handle(P, px, ob, case.ex)
    mom = E.run_moments(P.atm, P.opts, SHIFTS)
    check_sums(mom, xcor.reference(pairs, ob), xcor.abs_reference(pairs, ob), ob, "moments of the exposed pairs")
    bare = handle(P, px, ob)
    assert not np.array_equal(mom, bare.run_moments(P.atm, P.opts, SHIFTS))
    # the exposure with scale 0: the model is 0 there, and no pixel is dead
    for c in (xcor.WG, xcor.WGG, xcor.WFG):
        assert np.all(mom[2, :, c] == 0), c
    assert np.all(mom[2, :, xcor.N] > 0) and np.all(mom[:, :, xcor.WGG][[0, 1, 3, 4, 5, 6]] > 0)
    # the filter behind them
    F = xcor.svd_filter(ob.data, ob.seg_first, 3)
    E.set_filter(F)
    fmom, fval = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    xc.check_values(fval, pairs, ob, F, "filter behind the exposed pairs")
    xc.check_filtered_moments(fmom, fval, ob, "filtered moments of the exposed pairs")
    assert np.array_equal(E.run_moments(P.atm, P.opts, SHIFTS), mom)
    # with a high-pass as well: its definition over the exposed pairs, then the same two
    hp = xcor.gaussian_highpass(12.0)
    E.set_highpass(hp)
    hval = xcor.highpass_reference(pairs, ob, hp)
    assert not np.any(np.isnan(hval))
    hmom = E.run_moments(P.atm, P.opts, SHIFTS)
    check_sums(hmom, xcor.reference_values(hval, ob), xcor.abs_reference_values(hval, ob), ob, "high-passed moments of the exposed pairs")
    gain_free = xcor.Observed(ob.seg_first, ob.data, ob.weight, None)
    hfmom, hfval = E.run_filtered_moments(P.atm, P.opts, SHIFTS, values=True)
    xc.check_values(hfval, xcor.highpass_pairs(hval), gain_free, F, "filter behind the high-pass of the exposed pairs")
    xc.check_filtered_moments(hfmom, hfval, ob, "filtered high-passed moments of the exposed pairs")
    assert not np.array_equal(hmom, mom) and not np.array_equal(hfmom, fmom)
    E.close(); bare.close()


# ---- 5. independence --------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_rest_of_the_call(case):
    P, px, ob, first = case.P, case.px, case.ob, case.pairs
    E = handle(P, px, ob, case.ex)
    for _ in range(2):
        assert np.array_equal(E.run_exposed(P.atm, P.opts, SHIFTS), first)
    assert np.array_equal(E.run_exposed(P.atm, P.opts, SHIFTS, spectrum=True)[0], first)
    # the other rows' smear and scale change: rows 1 and 4 keep theirs
    smear, scale = xc.SMEAR[::-1].copy(), (xc.SCALE * -2.0 + 0.125)[::-1].copy()
    for v in (1, 4):
        smear[v], scale[v] = xc.SMEAR[v], xc.SCALE[v]
    E.set_exposures(exposures.Exposures(scale, smear))
    got = E.run_exposed(P.atm, P.opts, SHIFTS)
    assert np.array_equal(got[[1, 4]], first[[1, 4]])
    assert all(not np.array_equal(got[v], first[v]) for v in (0, 2, 3, 5, 6))
    # the exposures permuted, with their shifts
    perm = [4, 0, 6, 2, 5, 1, 3]
    E.set_exposures(exposures.Exposures(xc.SCALE[perm], xc.SMEAR[perm]))
    assert np.array_equal(E.run_exposed(P.atm, P.opts, SHIFTS[perm]), first[perm])
    E.close()


def test_batch_pairs_are_the_single_handle_pairs(case):
    P, px, ob = case.P, case.px, case.ob
    K = 4
    atms, keep = pc.atmospheres(P, K)
    shifts = np.stack([np.roll(SHIFTS, j) * (1.0 + 1e-6 * j) for j in range(K)])
    tables = [exposures.Exposures(np.roll(xc.SCALE, j) + 0.25 * j, np.roll(xc.SMEAR, 2 * j)) for j in range(K)]
    one = handle(P, px, ob)
    ref, ref1, mom = [], [], []
    for j in range(K):
        one.set_exposures(tables[j])
        ref.append(one.run_exposed(atms[j], P.opts, shifts[j]))
        mom.append(one.run_moments(atms[j], P.opts, shifts[j]))
        one.set_exposures(tables[1])
        ref1.append(one.run_exposed(atms[j], P.opts, shifts[j]))
    one.set_exposures(None)
    bare = np.stack([one.run_moments(atms[j], P.opts, shifts[j]) for j in range(K)])
    one.close()
    ref, ref1, mom = np.stack(ref), np.stack(ref1), np.stack(mom)
    assert len({ref[j].tobytes() for j in range(K)}) == K
    B = Batch(P.static, ways=3)
    B.set_pixels(px)
    B.set_observed(ob)
    with pytest.raises(EngineError) as ei:              # no table installed
        B.run_exposed(atms, P.opts, shifts)
    assert ei.value.code == -1 and "exposure table" in str(ei.value)
    assert np.array_equal(B.run_moments(atms, P.opts, shifts), bare)
    B.set_exposures(tables)                             # n = k
    for rep in range(2):
        assert np.array_equal(B.run_exposed(atms, P.opts, shifts), ref), rep
    assert np.array_equal(B.run_moments(atms, P.opts, shifts), mom)
    B.set_exposures(tables[1])                          # n = 1
    assert np.array_equal(B.run_exposed(atms, P.opts, shifts), ref1)
    # n not in {1, k}
    B.set_exposures(tables[:3])
    for run in (B.run_exposed, B.run_moments):
        with pytest.raises(EngineError) as ei:
            run(atms, P.opts, shifts)
        assert ei.value.code == -1 and "3 exposure tables" in str(ei.value)
    assert np.array_equal(B.run_exposed(atms[:3], P.opts, shifts[:3]), ref[:3])
    # all entries are checked before any is kept
    with pytest.raises(EngineError) as ei:
        B.set_exposures([tables[0], exposures.Exposures(xc.SCALE, np.where(np.arange(7) == 4, 0.5, xc.SMEAR))])
    assert ei.value.code == -1 and "entry 1" in str(ei.value) and "exposure 4" in str(ei.value)
    assert np.array_equal(B.run_exposed(atms[:3], P.opts, shifts[:3]), ref[:3])
    B.set_exposures(None)                               # cleared: the plain moments again
    assert np.array_equal(B.run_moments(atms, P.opts, shifts), bare)
    B.set_exposures(tables[1])
    B.set_observed(ob)                                  # drops the tables
    with pytest.raises(EngineError):
        B.run_exposed(atms, P.opts, shifts)
    B.close()


# ---- 6. ignored where rows are not exposures ----------------------------------------------------------------------
def test_the_other_runs_do_not_know_of_the_table(case):
    P, px, ob = case.P, case.px, case.ob
    E, bare = handle(P, px, ob, case.ex), handle(P, px, ob)
    hp, F, vm = xcor.gaussian_highpass(12.0), xcor.svd_filter(ob.data, ob.seg_first, 3), xc.the_map("ccf")
    bs = pixels.as_bands(pixels.Pixels(px.centre[::100], px.fwhm[::100], px.cut), SHIFTS[:2])
    for X in (E, bare):
        X.set_highpass(hp)
        X.set_filter(F)
        X.set_bands(bs)
        X.set_broadening(None)
    lags = SHIFTS[[1, 4, 1]]
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)
    assert same(E.run_pixels(P.atm, P.opts, SHIFTS), case.plain)
    assert same(E.run_highpassed(P.atm, P.opts, SHIFTS), bare.run_highpassed(P.atm, P.opts, SHIFTS))
    assert same(E.run_trail(P.atm, P.opts, lags), bare.run_trail(P.atm, P.opts, lags))
    assert same(E.run_velocity_map(P.atm, P.opts, vm), bare.run_velocity_map(P.atm, P.opts, vm))
    assert same(E.run_filtered_map(P.atm, P.opts, vm), bare.run_filtered_map(P.atm, P.opts, vm))
    assert same(E.run(P.atm, P.opts)["spectrum"], case.spec)
    assert same(E.run_bands(P.atm, P.opts), bare.run_bands(P.atm, P.opts))
    from transit_amd import broaden
    for X in (E, bare):
        X.set_broadening(broaden.Rotation(8.0, 0.4))
    assert same(E.run_broadened(P.atm, P.opts), bare.run_broadened(P.atm, P.opts))
    # ... and the table is still in force behind them, over the broadened spectrum now
    got = E.run_exposed(P.atm, P.opts, SHIFTS)
    assert not np.array_equal(got, case.pairs) and np.array_equal(got[0], bare.run_pixels(P.atm, P.opts, SHIFTS)[0])
    E.close(); bare.close()


# ---- 7. lifetime and refusals -------------------------------------------------------------------------------------
def test_refusals_and_lifetimes(case):
    P, px, ob = case.P, case.px, case.ob
    E = Engine(P.static)
    lib, dp = E._lib, _abi.c_double_p
    E.set_pixels(px)
    with pytest.raises(EngineError) as ei:             # no observed set
        E.set_exposures(case.ex)
    assert ei.value.code == -1 and "no observed set" in str(ei.value)
    with pytest.raises(EngineError) as ei:
        E.run_exposed(P.atm, P.opts, SHIFTS)
    assert ei.value.code == -1 and "no observed set" in str(ei.value)
    E.set_observed(ob)
    with pytest.raises(EngineError) as ei:             # no table
        E.run_exposed(P.atm, P.opts, SHIFTS)
    assert ei.value.code == -1 and "no exposure table" in str(ei.value)
    E.set_exposures(case.ex)
    assert np.array_equal(E.run_exposed(P.atm, P.opts, SHIFTS), case.pairs)

    def with_exposure_3(scale=-0.25, smear=3e-6):
        sc, sm = xc.SCALE.copy(), xc.SMEAR.copy()
        sc[3], sm[3] = scale, smear
        return exposures.Exposures(sc, sm)

    bad = {"scale nan": with_exposure_3(scale=np.nan), "scale inf": with_exposure_3(scale=np.inf), "scale -inf": with_exposure_3(scale=-np.inf),
           "smear nan": with_exposure_3(smear=np.nan), "smear inf": with_exposure_3(smear=np.inf), "smear < 0": with_exposure_3(smear=-1e-9),
           "smear above the cap": with_exposure_3(smear=np.nextafter(exposures.SMEAR_MAX, 1.0))}
    for what, ex in bad.items():
        with pytest.raises(EngineError) as ei:
            E.set_exposures(ex)
        assert ei.value.code == -1 and "exposure 3" in str(ei.value) and what.split()[0] in str(ei.value), what
        assert np.array_equal(E.run_exposed(P.atm, P.opts, SHIFTS), case.pairs), what      # the previous table acts
    E.set_exposures(with_exposure_3(smear=exposures.SMEAR_MAX))                            # the cap itself is taken
    E.set_exposures(case.ex)
    for what, ex in (("6", exposures.Exposures(xc.SCALE[:6], xc.SMEAR[:6])), ("8", exposures.Exposures(np.ones(8)))):
        with pytest.raises(EngineError) as ei:
            E.set_exposures(ex)
        assert ei.value.code == -1 and "nexp " + what in str(ei.value) and "nexp 7" in str(ei.value)
    c = case.ex.to_c()
    c.nexp = -7
    assert lib.trx_set_exposures(E._h, C.byref(c)) == -1 and b"nexp < 0" in lib.trx_last_error(E._h)
    c = case.ex.to_c()
    c.scale, c.smear = None, None
    assert lib.trx_set_exposures(E._h, C.byref(c)) == -1 and b"NULL" in lib.trx_last_error(E._h)
    assert np.array_equal(E.run_exposed(P.atm, P.opts, SHIFTS), case.pairs)
    # the run's own refusals: counts and NULLs as run_moments, out in place of mom; the shifts
    out, sh = np.zeros_like(case.pairs), np.ascontiguousarray(SHIFTS)

    def run(nshift, shift, dest):
        return lib.trx_run_exposed(E._h, C.byref(P.atm), C.byref(P.opts), None, nshift, shift.ctypes.data_as(dp) if shift is not None else None,
                                   dest.ctypes.data_as(dp) if dest is not None else None, None)

    for nshift in (0, -3, 6, 8):
        assert run(nshift, sh, out) == -1 and b"nexp 7" in lib.trx_last_error(E._h), nshift
    assert run(7, None, out) == -1 and b"shift is NULL" in lib.trx_last_error(E._h)
    assert run(7, sh, None) == -1 and b"out is NULL" in lib.trx_last_error(E._h)
    for what, v in (("nan", np.nan), ("inf", np.inf), ("0", 0.0), ("< 0", -1.0)):
        s = sh.copy()
        s[4] = v
        assert run(7, s, out) == -1 and b"shift 4" in lib.trx_last_error(E._h), what
    assert np.all(out == 0)
    assert run(7, sh, out) == 0 and np.array_equal(out, case.pairs)
    # the filter and the high-pass come and go without the table
    mom = E.run_moments(P.atm, P.opts, SHIFTS)
    E.set_filter(xcor.svd_filter(ob.data, ob.seg_first, 2))
    E.set_highpass(xcor.boxcar_highpass(9))
    assert np.array_equal(E.run_exposed(P.atm, P.opts, SHIFTS), case.pairs)
    E.set_filter(None)
    E.set_highpass(None)
    assert np.array_equal(E.run_moments(P.atm, P.opts, SHIFTS), mom)
    # a refused observed set keeps the table, a successful one drops it -- a clearing one too; so does set_pixels
    with pytest.raises(EngineError):
        E.set_observed(xcor.Observed(np.array([0, 500, 400, 1200]), ob.data))
    assert np.array_equal(E.run_exposed(P.atm, P.opts, SHIFTS), case.pairs)
    E.set_observed(ob)
    with pytest.raises(EngineError) as ei:
        E.run_exposed(P.atm, P.opts, SHIFTS)
    assert ei.value.code == -1 and "no exposure table" in str(ei.value)
    bare = E.run_moments(P.atm, P.opts, SHIFTS)
    assert not np.array_equal(bare, mom)
    E.set_exposures(case.ex)
    E.set_pixels(px)
    E.set_observed(ob)
    with pytest.raises(EngineError) as ei:
        E.run_exposed(P.atm, P.opts, SHIFTS)
    assert ei.value.code == -1 and "no exposure table" in str(ei.value)
    E.set_exposures(case.ex)
    E.set_exposures(None)                              # cleared; an empty table clears too
    assert np.array_equal(E.run_moments(P.atm, P.opts, SHIFTS), bare)
    E.set_exposures(case.ex)
    E.set_exposures(exposures.Exposures())
    with pytest.raises(EngineError):
        E.run_exposed(P.atm, P.opts, SHIFTS)
    E.close()


# ---- 8. shards ----------------------------------------------------------------------------------------------------
def test_shards_combined_in_rank_order(case):
    P, px, ob, ex = case.P, case.px, case.ob, case.ex
    wn_i, wn_d, n, _ = pc.grid(P)
    tol = tolerance(P, px, SHIFTS, ex, case.lens)
    ref = exposures.reference(case.spec, wn_i, wn_d, n, px, SHIFTS, ex)
    pc.check_close(np.array(case.pairs), ref, tol, "whole grid")
    cuts = [0, 1500, 3777, n]
    parts, empties, negative = [], 0, 0
    try:
        for r in range(3):
            P.set_shard(cuts[r], cuts[r + 1])
            E = handle(P, px, ob, ex)
            s, sp = E.run_exposed(P.atm, P.opts, SHIFTS, spectrum=True)
            with pytest.raises(EngineError) as ei:      # the moment runs stay unsupported on a shard
                E.run_moments(P.atm, P.opts, SHIFTS)
            assert ei.value.code == -6
            E.close()
            assert sp.shape == (cuts[r + 1] - cuts[r],)
            pc.check_close(s, exposures.reference(sp, wn_i, wn_d, n, px, SHIFTS, ex, lo=cuts[r]), tol, "shard %d" % r)
            for v in range(7):
                for p in range(len(px)):
                    a, z = exposures.exposed_range(wn_i, wn_d, n, float(px.centre[p]) / float(SHIFTS[v]), float(px.fwhm[p]) / float(SHIFTS[v]), px.cut, ex.eta(v))
                    if max(a, cuts[r]) >= min(z, cuts[r + 1]):
                        empties += 1
                        negative += xc.SCALE[v] < 0
                        assert s[v, p, 0] == 0 and s[v, p, 1] == 0 and not np.signbit(s[v, p, 0]) and not np.signbit(s[v, p, 1]), (r, v, p)
            parts.append(s)
    finally:
        P.set_shard(0, n)
    assert empties > 1000 and negative > 100
    pc.check_close(pixels.combine(parts), ref, tol, "shards added in rank order")
