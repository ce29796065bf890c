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


def _linedbs(rng, nlines, lo, hi):
    niso = int(rng.choice(ISOTOPES))
    ndb = min(int(rng.integers(1, 4)), niso)
    per_db = _split(rng, niso, ndb)
    mols = list(rng.choice(MOLECULES, ndb, replace=False))
    # lines per isotope: a random share, a quarter of the isotopes (never all of a database) without any
    w = rng.random(niso) * (rng.random(niso) >= 0.25)
    k0 = 0
    for n in per_db:
        if not w[k0:k0 + n].any():
            w[k0] = 1.0
        k0 += n
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
    d = {k: v for k, v in kw.items() if k != "dbs"}
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
