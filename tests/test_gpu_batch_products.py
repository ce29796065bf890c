"""Every product of a batch through ONE batch of handles, and what the batch forms refuse.

The per-product files check one batch form's happy path each; this one runs them all behind one another on the same
two handles (K = 3 atmospheres: one handle serves two of them), under per-atmosphere broadenings and under one for all,
lets an atmosphere fail inside every kind of product call, and pins the code and the exact text of every refusal of the
trx_run_batch_* family -- and of the single-handle observed runs (moments, filtered moments, trail) they deal to.

Shapes (the smallest that take every product's batch path, the per-atmosphere broadening and the handle-reuse path):
the 101-bin eclipse case of test_batch_reports_the_failing_atmosphere, 40 pixels, 3 exposures in segments of 13 and 27
pixels, a filter of 2 components, 5 lags, a map of 3 x 4 cells, 3 bands, broadenings of 1, 2 and 5 bins."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

import pixel_cases as pc
import xcor_checks as xc
from transit_amd import _abi, bands, broaden, pixels, synth, xcor
from transit_amd.engine import Batch, Engine, EngineError
from transit_amd.host import Problem

pytestmark = pytest.mark.gpu

K = 3
NEXP, NLAG, NPIX, NBANDS = 3, 5, 40, 3
LENGTHS = [13, 27]
BETAS = (4.1e-4, 1.037e-3, 2.1e-3)              # half-widths 1, 2 and 5 bins at the grid's last bin
PRODUCTS = ("bands", "contrib", "pixels", "moments", "filtered", "trail", "map", "broadened")
WANT_BROADENING = ("pixels", "moments", "filtered", "trail", "map", "broadened")
ARG, UNSUPPORTED = -1, -6
dp = _abi.c_double_p


def single(E, what, c, j):
    """product `what` of atmosphere j on the single handle, as a tuple of arrays"""
    a, o = c.atms[j], c.P.opts
    if what == "bands":
        return (E.run_bands(a, o),)
    if what == "contrib":
        return E.run_contrib(a, o)
    if what == "pixels":
        return (E.run_pixels(a, o, c.shifts[j]),)
    if what == "moments":
        return (E.run_moments(a, o, c.shifts[j]),)
    if what == "filtered":
        return (E.run_filtered_moments(a, o, c.shifts[j]),)
    if what == "trail":
        return (E.run_trail(a, o, c.lags[j]),)
    if what == "map":
        return E.run_velocity_map(a, o, c.vm, per=True)
    return (E.run_broadened(a, o),)


def batch(B, what, c):
    """product `what` of all atmospheres on the batch, as a tuple of arrays [K, ...]"""
    o = c.P.opts
    if what == "bands":
        return (B.run_bands(c.atms, o),)
    if what == "contrib":
        return B.run_contrib(c.atms, o)
    if what == "pixels":
        return (B.run_pixels(c.atms, o, c.shifts),)
    if what == "moments":
        return (B.run_moments(c.atms, o, c.shifts),)
    if what == "filtered":
        return (B.run_filtered_moments(c.atms, o, c.shifts),)
    if what == "trail":
        return (B.run_trail(c.atms, o, c.lags),)
    if what == "map":
        return B.run_velocity_map(c.atms, o, c.vm, per=True)
    return (B.run_broadened(c.atms, o),)


def install(X, c):
    X.set_bands(c.bands)
    X.set_pixels(c.px)
    X.set_observed(c.ob)
    X.set_filter(c.F)


@pytest.fixture(scope="module")
def ctx(tmp_path_factory):
    """the case, its K atmospheres, the sets, one Batch(ways=2) and one Engine with all of them installed, and the
    single handle's results: ref[mode][what][j], mode "own" (atmosphere j under broadening j) or "same" (all under the
    first), and plain[j] -- computed once, never changed"""
    d = str(tmp_path_factory.mktemp("batch_products") / "c")
    synth.make_case(d, nlines=20_000, wnlow=2500, wnhigh=2600, wndelt=1.0, wnosamp=2160, nlayers=60,
                    solution="eclipse", toomuch=10.0, ethresh=1e-50, seed=5)
    P = Problem.from_cfg(os.path.join(d, "case.cfg"))
    wn_i, wn_d, n, wn = pc.grid(P)
    c = SimpleNamespace(P=P, nwn=n, nl=int(P.atm.nlayer))
    c.atms, c.keep = pc.atmospheres(P, K)
    centres = np.linspace(2510.0, 2590.0, NPIX // 2) + 0.37 * wn_d
    c.px = pc.joined(pixels.resolving_power(centres, 1500.0, 4.0), pixels.resolving_power(centres, 400.0, 4.0))
    c.bands = [bands.tophat(wn, 2520.0, 2540.0), bands.gauss(2555.3, 6.0, 4.0), bands.weights(7, [1.0, 2.0, 3.0])]
    c.bl = [broaden.Rotation.from_beta(beta, limb) for beta, limb in zip(BETAS, (0.6, 0.0, 1.0))]
    halves = [int(broaden.half_widths(wn_i, wn_d, n, b.beta)[-1]) for b in c.bl]
    assert halves == [1, 2, 5] and max(halves) < _abi.BROADEN_MAX_HALF
    c.shifts = np.stack([np.roll(pc.SHIFTS, j)[:NEXP] * (1.0 + 1e-6 * j) for j in range(K)])
    lag_kms, lags = xcor.lag_grid(-6.0, 6.0, 3.0)
    c.lags = np.stack([lags * (1.0 + 1e-6 * j) for j in range(K)])
    c.vm = xc.the_map("loglike_bl19", lag_kms=lag_kms, kp=[10.0, 20.0, 30.0], vsys=[-2.0, -1.0, 0.0, 1.0],
                      orbit=np.sin(2 * np.pi * np.array([-0.02, 0.0, 0.02])), offset=[0.1, -0.2, 0.3])
    assert len(c.px) == NPIX and len(c.bands) == NBANDS and c.lags.shape == (K, NLAG) and (c.vm.nkp, c.vm.nvsys) == (3, 4)
    c.E = Engine(P.static)
    scale = float(np.mean(c.E.run(P.atm, P.opts)["spectrum"]))
    c.ob = xc.observed(NPIX, scale, lengths=LENGTHS, nexp=NEXP)
    c.F = xcor.svd_filter(c.ob.data, c.ob.seg_first, 2)
    install(c.E, c)
    c.ref = {}
    for mode in ("own", "same"):
        c.ref[mode] = {what: [] for what in PRODUCTS}
        for j in range(K):
            c.E.set_broadening(c.bl[j] if mode == "own" else c.bl[0])
            for what in PRODUCTS:
                c.ref[mode][what].append(single(c.E, what, c, j))
    c.E.set_broadening(None)
    c.plain = [c.E.run(c.atms[j], P.opts)["spectrum"].copy() for j in range(K)]
    c.B = Batch(P.static, ways=2)
    install(c.B, c)
    c.B.set_broadening(None)
    yield c
    c.B.close()
    c.E.close()


def check(got, ref, what):
    assert len(got) == len(ref[0]), what
    for j in range(K):
        for part, (g, r) in enumerate(zip(got, ref[j])):
            assert g[j].shape == r.shape and np.array_equal(g[j], r, equal_nan=True), (what, j, part)


def test_every_product_through_one_batch(ctx):
    c, B = ctx, ctx.B
    for what in WANT_BROADENING:                   # the broadening reaches the product: the modes are different references
        assert c.ref["own"][what][1][0].tobytes() != c.ref["same"][what][1][0].tobytes(), what
    for what in PRODUCTS:                          # the atmospheres differ, so do their products
        assert len({c.ref["own"][what][j][0].tobytes() for j in range(K)}) == K, what
    assert np.isfinite(c.ref["own"]["map"][0][0]).any()
    for mode, given in (("own", c.bl), ("same", c.bl[0]), ("own", c.bl)):
        B.set_broadening(given)
        for what in PRODUCTS:
            check(batch(B, what, c), c.ref[mode][what], (mode, what))
        # no product field leaks into the next call
        assert np.array_equal(B.run(c.atms, c.P.opts), np.stack(c.plain)), mode
    for what in reversed(PRODUCTS):                # and in another order of the calls
        check(batch(B, what, c), c.ref["own"][what], ("reversed", what))
    B.set_broadening(None)
    assert np.array_equal(B.run(c.atms, c.P.opts), np.stack(c.plain))


def test_a_failing_atmosphere_inside_a_product_call(ctx):
    c, B = ctx, ctx.B
    B.set_broadening(c.bl)
    try:
        for what in ("bands", "pixels", "moments", "trail", "map", "broadened"):
            c.atms[1].nlayer = 0                   # run_check refuses this one
            with pytest.raises(EngineError) as ei:
                batch(B, what, c)
            assert ei.value.code == ARG, what
            assert B._err() == "atmosphere 1: at least three layers are needed", (what, B._err())
            assert str(ei.value).endswith(" atmosphere 1: at least three layers are needed"), what
            c.atms[1].nlayer = c.nl                # the same call succeeds once the atmosphere is restored
            check(batch(B, what, c), c.ref["own"][what], ("restored", what))
    finally:
        c.atms[1].nlayer = c.nl
        B.set_broadening(None)


# the batch forms: the row arrays in the order each function checks them, and the call
FORMS = {
    "trx_run_batch_bands": (("sums",), lambda lib, b, k, a, o, r, c: lib.trx_run_batch_bands(b, k, a, o, r["sums"])),
    "trx_run_batch_contrib": (("sums", "contrib"), lambda lib, b, k, a, o, r, c: lib.trx_run_batch_contrib(b, k, a, o, r["sums"], r["contrib"])),
    "trx_run_batch_broadened": (("broadened",), lambda lib, b, k, a, o, r, c: lib.trx_run_batch_broadened(b, k, a, o, r["broadened"])),
    "trx_run_batch_pixels": (("shift", "out"), lambda lib, b, k, a, o, r, c: lib.trx_run_batch_pixels(b, k, a, o, c.get("n", NEXP), r["shift"], r["out"])),
    "trx_run_batch_moments": (("shift", "mom"), lambda lib, b, k, a, o, r, c: lib.trx_run_batch_moments(b, k, a, o, c.get("n", NEXP), r["shift"], r["mom"])),
    "trx_run_batch_filtered_moments": (("shift", "mom"), lambda lib, b, k, a, o, r, c: lib.trx_run_batch_filtered_moments(b, k, a, o, c.get("n", NEXP), r["shift"], r["mom"])),
    "trx_run_batch_trail": (("lag", "trail"), lambda lib, b, k, a, o, r, c: lib.trx_run_batch_trail(b, k, a, o, c.get("n", NLAG), r["lag"], r["trail"])),
    "trx_run_batch_velocity_map": (("map", "per"), lambda lib, b, k, a, o, r, c: lib.trx_run_batch_velocity_map(b, k, a, o, c["vm"], r["map"], r["per"])),
}
FITS = [f for f in FORMS if f not in ("trx_run_batch_bands", "trx_run_batch_contrib")]
NEEDS = {"trx_run_batch_bands": "band", "trx_run_batch_contrib": "band", "trx_run_batch_pixels": "pixel",
         "trx_run_batch_moments": "observed", "trx_run_batch_filtered_moments": "observed", "trx_run_batch_trail": "observed",
         "trx_run_batch_velocity_map": "observed"}
SETTER = {"band": "trx_batch_set_bands", "pixel": "trx_batch_set_pixels", "observed": "trx_batch_set_observed"}


def test_the_refusal_table(ctx):
    c, B, lib = ctx, ctx.B, ctx.B._lib
    arr = (_abi.TrxAtm * K)(*c.atms)
    opts = C.byref(c.P.opts)
    outs = {"sums": (K, NBANDS, 2), "contrib": (K, NBANDS, c.nl), "broadened": (K, c.nwn), "out": (K, NEXP, NPIX, 2),
            "mom": (K, NEXP, len(LENGTHS), 7), "trail": (K, NLAG, NEXP, len(LENGTHS), 7), "map": (K, 3, 4), "per": (K, NLAG, NEXP),
            "spectra": (K, c.nwn)}
    buf = {name: np.full(shape, -7.0) for name, shape in outs.items()}
    buf["shift"], buf["lag"] = c.shifts.copy(), c.lags.copy()

    def rows(name, null=()):
        return (dp * K)(*[None if j in null else buf[name][j].ctypes.data_as(dp) for j in range(K)])

    def call(fn, null=None, k=K, atm=arr, **extra):
        """(code, trx_last_error(NULL)) of a call with row j of array `name` NULL for every (name, j) of `null`"""
        names, f = FORMS[fn]
        null = null or {}
        r = {name: rows(name, null.get(name, ())) for name in names}
        rc = f(lib, B._b, k, atm, opts, r, dict({"vm": C.byref(c.vm.to_c())}, **extra))
        for name in outs:
            assert np.all(buf[name] == -7.0), (fn, name)      # a refusal touches no output
        return rc, B._err()

    # two broadenings installed for three atmospheres: what every broadened or pixel form refuses LAST
    B.set_broadening(c.bl[:2])
    try:
        for fn, (names, _) in FORMS.items():
            # a NULL row, in each array in turn
            for name in names:
                assert call(fn, {name: (1,)}) == (ARG, "%s: %s[1] is NULL" % (fn, name)), (fn, name)
            if len(names) == 2:                        # by atmosphere first, then in the order of the arrays
                assert call(fn, {names[0]: (1,), names[1]: (1,)}) == (ARG, "%s: %s[1] is NULL" % (fn, names[0])), fn
                assert call(fn, {names[0]: (1,), names[1]: (0,)}) == (ARG, "%s: %s[0] is NULL" % (fn, names[1])), fn
            assert call(fn, atm=None) == (ARG, fn + ": bad argument"), fn
            assert call(fn, k=-1) == (ARG, fn + ": bad argument"), fn
            if fn in FITS:
                want = (ARG, fn + ": 2 broadenings installed (trx_batch_set_broadening) for 3 atmospheres")
                assert call(fn) == want, fn
                assert call(fn, k=0) == (0, ""), fn       # no atmosphere fits any number of them
        assert call("trx_run_batch_velocity_map", vm=None) == (ARG, "trx_run_batch_velocity_map: vm is NULL")
        # the counts
        for n in (0, -3):
            assert call("trx_run_batch_pixels", n=n) == (ARG, "trx_run_batch_pixels: nshift < 1")
            assert call("trx_run_batch_trail", n=n) == (ARG, "trx_run_batch_trail: nlag < 1")
            assert call("trx_run_batch_pixels", {"shift": (1,)}, n=n) == (ARG, "trx_run_batch_pixels: nshift < 1")
            assert call("trx_run_batch_trail", {"lag": (1,)}, n=n) == (ARG, "trx_run_batch_trail: nlag < 1")
        # plain trx_run_batch: a code and no text
        assert lib.trx_run_batch(B._b, K, arr, opts, rows("spectra", (1,))) == ARG and B._err() == ""
        assert np.all(buf["spectra"] == -7.0)
        # nothing installed: the set's refusal comes before the rows', the filter's after the observed set's
        B.set_broadening(None)
        assert call("trx_run_batch_broadened") == (ARG, "trx_run_batch_broadened: no broadening installed (trx_batch_set_broadening)")
        assert call("trx_run_batch_broadened", {"broadened": (1,)}) == (ARG, "trx_run_batch_broadened: no broadening installed (trx_batch_set_broadening)")
        B.set_broadening(c.bl[:2])
        B.set_filter(None)
        assert call("trx_run_batch_filtered_moments", {"mom": (1,)}) == (ARG, "trx_run_batch_filtered_moments: no filter installed (trx_batch_set_filter)")
        B.set_bands([])
        B.set_pixels(None)                             # (the observed set goes with it)
        for fn, kind in NEEDS.items():
            want = (ARG, "%s: no %s set installed (%s)" % (fn, kind, SETTER[kind]))
            assert call(fn) == want and call(fn, {FORMS[fn][0][0]: (1,)}) == want, fn
        B.set_pixels(c.px)
        for fn, kind in NEEDS.items():
            if kind == "observed":
                assert call(fn) == (ARG, "%s: no observed set installed (trx_batch_set_observed)" % fn), fn
    finally:
        install(B, c)
        B.set_broadening(None)
    # what the single-handle call refuses comes back under its atmosphere's number, a count that is not nexp for one
    # (both handles start on a refused atmosphere: whichever reports first)
    B.set_broadening(c.bl)
    rc, msg = call("trx_run_batch_moments", n=2)
    assert rc == ARG and msg in ["atmosphere %d: trx_run_moments: nshift 2 is not the observed set's nexp 3" % j for j in (0, 1)], msg
    # and the batch computes what it did before
    for what in PRODUCTS:
        check(batch(B, what, c), c.ref["own"][what], ("after the refusals", what))
    B.set_broadening(None)
    assert np.array_equal(B.run(c.atms, c.P.opts), np.stack(c.plain))


WINDOWED = "%s: this handle's shard is not the whole grid; take trx_run_pixels, add the ranks' pairs (trx_gather_host) and %s them on the host"


def test_observed_run_refusals_of_a_single_handle(ctx):
    c, lib = ctx, ctx.E._lib
    atm, opts = C.byref(c.atms[0]), C.byref(c.P.opts)
    sh, lg = np.ascontiguousarray(c.shifts[0]), np.ascontiguousarray(c.lags[0])
    mom, trail = np.full((NEXP, len(LENGTHS), 7), -7.0), np.full((NLAG, NEXP, len(LENGTHS), 7), -7.0)
    p = lambda x: x.ctypes.data_as(dp) if x is not None else None

    def moments(h, n=NEXP, s=sh, m=mom):
        return lib.trx_run_moments(h, atm, opts, None, n, p(s), p(m), None), (lib.trx_last_error(h) or b"").decode()

    def filtered(h, n=NEXP, s=sh, m=mom):
        return lib.trx_run_filtered_moments(h, atm, opts, None, n, p(s), None, p(m), None), (lib.trx_last_error(h) or b"").decode()

    def a_trail(h, n=NLAG, s=lg, m=trail):
        return lib.trx_run_trail(h, atm, opts, None, n, p(s), p(m), None), (lib.trx_last_error(h) or b"").decode()

    runs = (("trx_run_moments", moments, "shift", "mom"), ("trx_run_filtered_moments", filtered, "shift", "mom"),
            ("trx_run_trail", a_trail, "lag", "trail"))
    # a shard of the grid: refused first, whatever is installed (here: nothing) and whatever else is wrong
    n = c.P.nwn
    try:
        c.P.set_shard(10, 90)
        S = Engine(c.P.static)
    finally:
        c.P.set_shard(0, n)
    try:
        for who, run, _, _ in runs:
            want = (UNSUPPORTED, WINDOWED % (who, "filter and reduce" if who == "trx_run_filtered_moments" else "reduce"))
            assert run(S._h) == want and run(S._h, n=0, s=None, m=None) == want, who
    finally:
        S.close()
    # the whole grid
    E, h = c.E, c.E._h
    try:
        for who, run, in_name, out_name in runs:
            count = "nlag < 1" if who == "trx_run_trail" else "nshift 0 is not the observed set's nexp 3"
            assert run(h, n=0) == (ARG, "%s: %s" % (who, count)), who
            assert run(h, n=0, s=None, m=None) == (ARG, "%s: %s" % (who, count)), who
            assert run(h, s=None, m=None) == (ARG, "%s: %s is NULL" % (who, in_name)), who
            assert run(h, m=None) == (ARG, "%s: %s is NULL" % (who, out_name)), who
        assert moments(h, n=4) == (ARG, "trx_run_moments: nshift 4 is not the observed set's nexp 3")
        E.set_filter(None)
        assert filtered(h, n=0, s=None, m=None) == (ARG, "trx_run_filtered_moments: no filter installed (trx_set_filter)")
        E.set_observed(None)
        for who, run, _, _ in runs:
            assert run(h, n=0, s=None, m=None) == (ARG, who + ": no observed set installed (trx_set_observed)"), who
        E.set_pixels(None)
        for who, run, _, _ in runs:
            assert run(h) == (ARG, who + ": no observed set installed (trx_set_observed)"), who
        assert np.all(mom == -7.0) and np.all(trail == -7.0)
    finally:
        install(E, c)
    E.set_broadening(c.bl[0])
    for what in ("moments", "filtered", "trail"):
        got = single(E, what, c, 0)
        assert np.array_equal(got[0], c.ref["same"][what][0][0]), what
    E.set_broadening(None)
