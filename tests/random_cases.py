"""Seeded random problems shared by the random sweeps (test_gpu_random.py: HIP path against the
CPU oracle; test_random_reference.py: the oracle against the compiled reference).

random_case(seed) returns the keyword arguments of synth.make_case for one problem, the same for
the same seed.  The space reaches the edges where the kernels change form:

* layers on both sides of the walk step (kWalkLayers = 64) and the ray tail's limit
  (kTailLayers = 128), with thresholds under which some rays sweep more than 128 layers
  (plans of three and more steps, no tail);
* 1-3 line databases with 2..256 isotopes between them (the window's kWalkSegs = 16 isotope
  blocks, the tail's 64-block mask, kMaxIso = 256), some isotopes without lines;
* 1, 5, 8, 9 or 16 emission angles (k_ray_tail<8> against k_ray_tail<kMaxAngles>);
* the cloud models and the scattering options of test_gpu_properties.

At most 5000 lines per problem."""
import numpy as np

from transit_amd import synth

LAYERS = [3, 4, 9, 30, 63, 64, 65, 70, 127, 128, 129, 150, 200]
ISOTOPES = [2, 15, 16, 17, 63, 64, 65, 130, 256]
ANGLES = [1, 5, 8, 9, 16]
# the five parametrisations of test_gpu_properties.test_cloud_models_against_oracle
CLOUDS = ["ext,1e-9,-3.0,0.5", "opa,1e-3,-3.0,0.5", "B17,1e-7,-3.0,0.5,-1.5",
          "F18,1e-7,-3.0,0.5,2.0,0.8,1e-5", "P19,1e-9,-3.0,0.5,-2.0,1e-22,3000.0"]
SCATTERING = ["1.5", "polar"]
MOLECULES = ["CH4", "H2O", "CO", "CO2"]
_MASS = {m[1]: m[2] for m in synth.MOLECULE_TABLE}


def _split(rng, total, parts):
    """`total` as `parts` random positive integers."""
    cuts = np.sort(rng.choice(np.arange(1, total), parts - 1, replace=False))
    return [int(v) for v in np.diff(np.concatenate([[0], cuts, [total]]))]


def _linedbs(rng, nlines, lo, hi, empty_db=False):
    """empty_db: the last of at least two databases has no line at all."""
    niso = int(rng.choice(ISOTOPES))
    ndb = min(int(rng.integers(1, 4)), niso)
    if empty_db:
        ndb = max(ndb, 2)
    per_db = _split(rng, niso, ndb)
    mols = list(rng.choice(MOLECULES, ndb, replace=False))
    # lines per isotope: a random share, a quarter of the isotopes (never all of a database) without any
    w = rng.random(niso) * (rng.random(niso) >= 0.25)
    k0 = 0
    for n in per_db:
        if not w[k0:k0 + n].any():
            w[k0] = 1.0
        k0 += n
    if empty_db:
        w[niso - per_db[-1]:] = 0.0
    counts = rng.multinomial(nlines, w / w.sum())
    dbs, k0 = [], 0
    for j, (mol, n) in enumerate(zip(mols, per_db)):
        c = counts[k0:k0 + n]
        ratios = 0.5 ** np.arange(1, n + 1)
        ratios[0] += 1.0 - ratios.sum()
        nl = int(c.sum())
        dbs.append(synth.synth_linedb(nl, lo, hi, seed=int(rng.integers(1, 10**6)),
                                      name="synthetic %s, %d isotopes" % (mol, n), molname=str(mol),
                                      iso_names=tuple("%d%03d" % (j + 1, i) for i in range(n)),
                                      iso_masses=tuple(_MASS[mol] + 0.37 * i for i in range(n)),
                                      iso_ratios=tuple(float(r) for r in ratios),
                                      iso_split=tuple(float(v) / nl for v in c) if nl else (1.0,) + (0.0,) * (n - 1),
                                      z_scale=float(rng.choice([107.0, 170.0, 590.0])),
                                      log_gf=[(-12.0, -5.0), (-16.0, -11.0)][int(rng.integers(0, 2))]))
        k0 += n
    return dbs


def random_case(seed):
    rng = np.random.default_rng(1000 + seed)
    solution = "eclipse" if rng.random() < 0.6 else "transit"
    wnlow = float(rng.choice([400.0, 2500.0, 4000.0, 9000.0]))
    width = float(rng.choice([2.0, 7.0, 20.0, 40.0]))
    wndelt = float(rng.choice([1.0, 0.5, 0.1, 0.02]))
    osamp = int(rng.choice([1, 2, 7, 60, 2160])) if wndelt >= 0.5 else int(rng.choice([1, 2, 5]))
    nlines = int(rng.choice([17, 300, 2000, 5000]))          # (empty and one-line lists: test_gpu_properties.py)
    nlayers = int(rng.choice(LAYERS))
    line_margin = float(rng.choice([0.0, 1.5]))
    toomuch = float(rng.choice([0.5, 5.0, 10.0, 50.0]))
    ethresh = float(rng.choice([1e-50, 1e-8, 1e-5, 1e-3]))
    if nlayers > 128 and rng.random() < 0.6:
        # deep rays: a high toomuch over weak lines -- more than 128 layers swept, no ray tail
        toomuch, ethresh = float(rng.choice([1e3, 1e5])), 1e-50
    ncia = int(rng.integers(0, 3))
    nang = int(rng.choice(ANGLES))
    extra = {}
    if rng.random() < 0.3:
        extra["cloud"] = str(rng.choice(CLOUDS))
    if rng.random() < 0.3:
        extra["scattering"] = str(rng.choice(SCATTERING))
    dbs = _linedbs(rng, nlines, wnlow - line_margin, wnlow + width + line_margin)
    return dict(wnlow=wnlow, wnhigh=wnlow + width, wndelt=wndelt, wnosamp=osamp, nlayers=nlayers,
                solution=solution, toomuch=toomuch, ethresh=ethresh, ncia=ncia, line_margin=line_margin,
                raygrid=" ".join("%.4g" % a for a in np.linspace(0.0, 80.0, nang)) if nang > 1 else "0",
                dbs=dbs, extra=extra)


def summary(kw):
    """The case in one line (assertion messages): everything but the line lists, which are told by size."""
    d = {k: v for k, v in kw.items() if k not in ("dbs", "atm")}
    d["isotopes"] = [len(db.isotopes) for db in kw["dbs"]]
    d["lines"] = sum(len(w) for db in kw["dbs"] for w in db.wl)
    return d


def fill_empty_isotopes(kw):
    """The case with one weak line in the middle of the band for every isotope that has none.  The
    reference reads an isotope without lines past the end of its line arrays (datafileBS over zero
    records, readlineinfo.c:496-524: one or two records of the next isotope, or beyond the file's),
    so it is compared on this twin; the host side skips such an isotope, and the kernels meet the
    empty blocks in test_gpu_random.py."""
    import copy
    kw = dict(kw, dbs=copy.deepcopy(kw["dbs"]))
    wl = 1e4 / (0.5 * (kw["wnlow"] + kw["wnhigh"]))
    for db in kw["dbs"]:
        for k in range(len(db.isotopes)):
            if len(db.wl[k]) == 0:
                db.wl[k], db.elow[k], db.gf[k] = np.array([wl]), np.array([1000.0]), np.array([1e-12])
    return kw


def empty_isotopes(kw):
    return sum(len(w) == 0 for db in kw["dbs"] for w in db.wl)


def reference_binary(kw):
    """The compiled reference that gives defined output for the case: cloud models 2-5 read tau.c's
    uninitialised mean density, defined only in the build with zero-initialised locals (oracle/Makefile)."""
    cloud = kw.get("extra", {}).get("cloud", "")
    return "transit_zinit" if cloud and not cloud.startswith("ext") else "transit"


# ---- opacity-grid problems (test_gpu_grid_random.py, test_random_grid_reference.py) ---------------------
# The per-molecule sweep (trx_sweep_permol) walks nv = nlayer x ntemp states in steps of up to 64 walking or 12
# two-kernel states, in the order v = layer * ntemp + temperature, from the last state down.  The short forms
# run only on a short step: k_line_walk_packed for <= 10 states, k_line_walk_lanes for <= 32 with 8+-bin
# frames on a dense list.  Each seed draws one class of state counts (GRID_NV_CLASSES); one state colder
# than kWalkMinTemp (~387 K) sends the whole sweep to the two-kernel form.
GRID_NV_CLASSES = ["around64", "mod64_1_10", "mod64_11_32", "around128", "mod64_11_32", "mod64_1_10", "around64", "over2000"]


def _grid_shape(rng, cls):
    """(nlayer, ntemp) with nlayer in 3..70 and ntemp in 2..30 whose product falls in the class."""
    ok = {"around64": lambda nv: nv in (63, 64, 65), "around128": lambda nv: nv in (128, 129),
          "mod64_1_10": lambda nv: nv > 64 and 1 <= nv % 64 <= 10,
          "mod64_11_32": lambda nv: nv > 64 and 11 <= nv % 64 <= 32,
          "over2000": lambda nv: nv >= 2000}[cls]
    pairs = [(nl, nt) for nl in range(3, 71) for nt in range(2, 31) if ok(nl * nt)]
    nl, nt = pairs[int(rng.integers(0, len(pairs)))]
    return nl, nt


def random_grid_case(seed):
    """synth.make_case keywords of one opacity-grid problem (extra: opacityfile, tlow, thigh, tempdelt): the
    grid spans 70..3000 K (the synthetic TLI's range), the atmosphere lies inside it.  One whole molecule slot
    without lines in the band on every seed == 3 (mod 8)."""
    rng = np.random.default_rng(5000 + seed)
    cls = GRID_NV_CLASSES[seed % len(GRID_NV_CLASSES)]
    nlayers, ntemp = _grid_shape(rng, cls)
    # grid temperatures: integer nodes, so that tlow + k * tempdelt is exact and ends on thigh
    cold = rng.random() < 0.25                       # a grid reaching below kWalkMinTemp: no state walks
    lo_min = 70 if cold else 390
    tempdelt = int(rng.integers(1, max(2, (3000 - lo_min) // (ntemp - 1)) + 1))
    tlow = int(rng.integers(lo_min, 3000 - (ntemp - 1) * tempdelt + 1))
    if cold:
        tlow = int(rng.integers(70, 381))
        tempdelt = min(tempdelt, (3000 - tlow) // (ntemp - 1))
    thigh = tlow + (ntemp - 1) * tempdelt
    # the atmosphere: inside [tlow, thigh), and inside the CIA tables where it has any (from 400 K, with
    # the second table from 800 K: synth.make_case)
    a_lo, a_hi = tlow + 0.05 * (thigh - tlow), thigh - 0.05 * (thigh - tlow)
    ncia = int(rng.integers(0, 3))
    cia_lo = [0.0, 400.0, 800.0][ncia]
    if a_lo < cia_lo:
        if a_hi > cia_lo + 20.0 and rng.random() < 0.5:
            a_lo = cia_lo + 1.0
        else:
            ncia = 0
    t_top, t_bottom = (float(v) for v in rng.uniform(a_lo, a_hi, 2))
    atm = synth.demo_atmosphere(nlayers, p_bottom=float(rng.choice([100.0, 10.0])), t_bottom=t_bottom, t_top=t_top)
    dense = rng.random() < 0.3                       # ngroups >= 8 nwn: k_line_walk_lanes runs unforced
    wnlow = float(rng.choice([400.0, 2500.0, 4000.0, 9000.0]))
    width = 2.0 if dense else float(rng.choice([2.0, 7.0, 20.0, 40.0]))
    wndelt = float(rng.choice([1.0, 0.5])) if dense else float(rng.choice([1.0, 0.5, 0.1, 0.02]))
    osamp = int(rng.choice([1, 2, 7, 60, 2160])) if wndelt >= 0.5 else int(rng.choice([1, 2, 5]))
    nlines = 5000 if dense else int(rng.choice([17, 300, 2000, 5000]))
    if cls == "over2000":                            # (the oracle sweeps every state: keep the band short)
        width, wndelt = min(width, 7.0), max(wndelt, 0.1)
        osamp = min(osamp, 60) if wndelt < 0.5 else osamp
    line_margin = float(rng.choice([0.0, 1.5]))
    ethresh = float(rng.choice([1e-50, 1e-8, 1e-5, 1e-3]))
    dbs = _linedbs(rng, nlines, wnlow - line_margin, wnlow + width + line_margin, empty_db=seed % 8 == 3)
    extra = {"opacityfile": "opac.dat", "tlow": tlow, "thigh": thigh, "tempdelt": tempdelt}
    return dict(wnlow=wnlow, wnhigh=wnlow + width, wndelt=wndelt, wnosamp=osamp, nlayers=nlayers,
                solution="eclipse" if rng.random() < 0.6 else "transit", toomuch=float(rng.choice([0.5, 10.0])),
                ethresh=ethresh, ncia=ncia, line_margin=line_margin, atm=atm, dbs=dbs, extra=extra)
