"""Golden cases: inputs + what the compiled reference wrote for them."""
import os

import numpy as np

import oracle_lib as ol
from transit_amd.host import Problem

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ["eclipse_small", "transit_small", "coadd_thresh", "cloud_scatter", "transit_modm1",
         "highres_fine", "midres_os4", "multi_species", "scat_polar", "qscale_eclipse", "dumps_transit",
         "resample_radius", "resample_transit", "many_isotopes", "saveext_transit",
         "cloud_opa", "cloud_b17", "cloud_f18", "cloud_p19"]


class Golden:
    def __init__(self, name):
        self.name = name
        self.dir = os.path.join(GOLDEN, name)
        self.problem = Problem.from_cfg(os.path.join(self.dir, "case.cfg"))
        self.spectrum = ol.read_spectrum(os.path.join(self.dir, "spectrum.dat"))[:, 1]
        _, self.tau = ol.read_rows_dump(os.path.join(self.dir, "tau.dat"), "wavenumber")      # [wn][height]
        _, self.e = ol.read_rows_dump(os.path.join(self.dir, "mol_extion.dat"), "radius")     # [layer][wn]
        _, cia = ol.read_rows_dump(os.path.join(self.dir, "CIA.dat"), "wavenumber")           # [wn][layer]
        self.e_cs = cia.T
        self.swept = (self.e != 0).any(axis=1)          # layers the reference's lazy sweep reached


_cache = {}


def golden(name):
    if name not in _cache:
        _cache[name] = Golden(name)
    return _cache[name]


def rel_err(a, b, floor=1e-300):
    a, b = np.asarray(a, float), np.asarray(b, float)
    m = np.abs(b) > floor
    if not m.any():
        return 0.0
    return float(np.max(np.abs(a[m] - b[m]) / np.abs(b[m])))


def free_port():
    """A TCP port that is free right now (rendezvous of multi-process tests)."""
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


SAVEFILES = (("tau.dat", "wavenumber"), ("CIA.dat", "wavenumber"), ("mol_extion.dat", "radius"),
             ("total_extion.dat", "wavenumber"), ("cloud_extion.dat", "wavenumber"), ("scatt_extion.dat", "wavenumber"))


def check_savefiles(got_dir, case, tol):
    """The six dumps of `savefiles yes` against the reference's own: same text skeleton (header,
    row keys, line count), same zeros (layers the reference's lazy sweep never reached; heights
    past the toomuch cut), values to `tol`."""
    for name, key in SAVEFILES:
        ref_path = os.path.join(GOLDEN, case, name)
        got_lines, ref_lines = open(os.path.join(got_dir, name)).read().split("\n"), open(ref_path).read().split("\n")
        assert got_lines[:4] == ref_lines[:4], (name, got_lines[:4], ref_lines[:4])
        assert len(got_lines) == len(ref_lines), (name, len(got_lines), len(ref_lines))
        gk, gv = ol.read_rows_dump(os.path.join(got_dir, name), key)
        rk, rv = ol.read_rows_dump(ref_path, key)
        assert np.array_equal(gk, rk), (name, "row keys", gk.shape, rk.shape)
        assert np.array_equal(gv == 0, rv == 0), (name, "zeros differ at", np.argwhere((gv == 0) != (rv == 0))[:4].tolist())
        assert rel_err(gv, rv) < tol, (name, rel_err(gv, rv), tol)
