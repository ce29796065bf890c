"""The spectrum engine: thin ctypes binding of the C ABI in include/transit_hip.h.

`Engine` is the MI355X product path (libtransit_hip.so, hand-written HIP).  It
never falls back to anything else: if the HIP library is missing or no gfx950
device is usable it raises.  `CEngine` is the ABI-shaped binding itself and
serves any library exporting the same create/run/destroy family.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np

from . import _abi
from . import bands as _bands
from . import broaden as _broaden
from . import pixels as _pixels
from .build import lib_path


class EngineError(RuntimeError):
    def __init__(self, code: int, where: str, detail: str = ""):
        super().__init__("%s failed: %s (%d) %s" % (where, _abi.STATUS.get(code, "?"), code, detail))
        self.code = code


class CEngine:
    """create/run/destroy over one handle of an ABI-shaped library."""

    def __init__(self, lib, prefix: str, static: _abi.TrxStatic):
        self._lib, self._p = lib, prefix
        self._h = C.c_void_p()
        self.nwn_total = int(static.nwn)
        self.lo, self.hi = int(static.wn_lo), int(static.wn_hi)
        self.ndop, self.nlor = int(static.ndop), int(static.nlor)
        rc = self._f("create")(C.byref(static), C.byref(self._h))
        if rc != 0:
            self._h = None
            raise EngineError(rc, prefix + "create", self._last_error())

    def _f(self, name):
        return getattr(self._lib, self._p + name)

    def _call(self, name, *args):
        """<prefix>name(handle, *args), a non-zero status raised with the handle's last error"""
        rc = self._f(name)(self._h, *args)
        if rc != 0:
            raise EngineError(rc, self._p + name, self._last_error())

    def _last_error(self) -> str:
        fn = getattr(self._lib, self._p + "last_error", None)
        if fn is None or not self._h:
            return ""
        v = fn(self._h)
        return v.decode(errors="replace") if v else ""

    def close(self):
        if getattr(self, "_h", None):
            self._f("destroy")(self._h)
            self._h = None

    __del__ = close

    @property
    def nwn(self) -> int:
        return self.hi - self.lo if self.hi > self.lo else self.nwn_total

    def run(self, atm: _abi.TrxAtm, opts: _abi.TrxOpts, debug=False,
            n_out: Optional[int] = None) -> Dict[str, np.ndarray]:
        """trx_run.  debug=True also returns every intermediate of trx_debug; a tuple of
        names ("e", "e_cs", "tau", "last", "intens", "computed") returns just those."""
        n = n_out if n_out is not None else self.nwn
        nl, na = int(atm.nlayer), max(int(opts.nangles), 1)
        out = {"spectrum": np.zeros(n)}
        dbg = None
        if debug:
            want = ("e", "e_cs", "tau", "last", "intens", "computed") if debug is True else tuple(debug)
            make = {"e": lambda: np.zeros((nl, n)), "e_cs": lambda: np.zeros((nl, n)),
                    "er": lambda: np.zeros((nl, n)), "e_scat": lambda: np.zeros((nl, n)), "e_cloud": lambda: np.zeros((nl, n)),
                    "tau": lambda: np.zeros((n, nl)), "last": lambda: np.zeros(n, dtype=np.int64),
                    "intens": lambda: np.zeros((na, n)), "computed": lambda: np.zeros(nl, dtype=np.uint8)}
            types = {"last": _abi.c_int64_p, "computed": _abi.c_uint8_p}
            for k in want:
                out[k] = make[k]()
            ptr = lambda k: out[k].ctypes.data_as(types.get(k, _abi.c_double_p)) if k in out else None
            dbg = _abi.TrxDebug(ptr("e"), ptr("e_cs"), ptr("tau"), ptr("last"), ptr("intens"), ptr("computed"),
                                ptr("er"), ptr("e_scat"), ptr("e_cloud"))
        self._call("run", C.byref(atm), C.byref(opts), _dp(out["spectrum"]), C.byref(dbg) if dbg is not None else None)
        return out

    def run_into(self, atm: _abi.TrxAtm, opts: _abi.TrxOpts, spectrum: np.ndarray) -> None:
        """trx_run into a caller's float64 array of this handle's shard size: no allocation per call
        (retrieval loops, bench.py's timed step)."""
        if spectrum.dtype != np.float64 or not spectrum.flags.c_contiguous or spectrum.size < self.nwn:
            raise ValueError("spectrum: a C-contiguous float64 array of at least %d elements" % self.nwn)
        self._call("run", C.byref(atm), C.byref(opts), _dp(spectrum), None)

    def sweep_permol(self, nv, temp, density, zpart, ethresh, nslot, iso_slot) -> np.ndarray:
        """computemolext(permol=1) for nv states: returns o[nv][nslot][nwn]."""
        out = np.zeros((nv, nslot, self.nwn))
        self._call("sweep_permol", nv, temp, density, zpart, float(ethresh), nslot, iso_slot, _dp(out))
        return out

    def build_opacity_grid(self, problem) -> np.ndarray:
        """calcopacity(): sweep the (layer x temperature) states of `problem`, let the
        host side write the file and switch the problem to grid mode."""
        nv, t, d, z, nslot, sl = problem.grid_request()
        o = self.sweep_permol(nv, t, d, z, problem.opts.ethresh, nslot, sl)
        problem.install_opacity(o)
        return o

    def restore_extinction(self, e: Optional[np.ndarray], computed: Optional[np.ndarray] = None):
        """trx_restore_extinction: e [nlayer][nwn_shard] and one flag per layer (None: forget them)."""
        if e is None:
            self._call("restore_extinction", 0, None, None)
        else:
            e = np.ascontiguousarray(e, dtype=np.float64); c = np.ascontiguousarray(computed, dtype=np.uint8)
            self._call("restore_extinction", e.shape[0], _dp(e), c.ctypes.data_as(_abi.c_uint8_p))

    def stats(self) -> Dict[str, float]:
        s = _abi.TrxStats()
        self._call("get_stats", C.byref(s))
        return s.as_dict()

    def table(self):
        """(profsize[ndop,nlor], offset[ndop,nlor], floats[total])"""
        n = self.ndop * self.nlor
        ps, off = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        tot = C.c_int64()
        self._call("table_info", ps.ctypes.data_as(_abi.c_int64_p), off.ctypes.data_as(_abi.c_int64_p), C.byref(tot))
        tab = np.zeros(tot.value, dtype=np.float32)
        self._call("table_copy", tab.ctypes.data_as(_abi.c_float_p))
        return ps.reshape(self.ndop, self.nlor), off.reshape(self.ndop, self.nlor), tab

    def width_grids(self):
        d, l = np.zeros(self.ndop), np.zeros(self.nlor)
        self._call("width_grids", _dp(d), _dp(l))
        return d, l


_hip = None
HIP_VERSIONS = None


def _one_hip_runtime():
    """A process must hold ONE HIP/HSA runtime.  PyTorch-ROCm wheels bundle their own
    libamdhip64.so (same soname as /opt/rocm's, but loaded by path): if our library came first
    and bound /opt/rocm's copy, a later `import torch` would map a second runtime, and RCCL
    (torch's librccl.so) would then find its HSA uninitialised ("no ROCm-capable device").  So
    when a torch wheel with a bundled runtime is installed, map that copy first -- ours then
    binds to it by soname, whichever import order the caller uses.  torch itself is not imported."""
    import importlib.util
    import sys
    # three busy queues per handle: see INTEGRATION.md section 4 (only effective while the HIP
    # runtime has not initialised yet; multi-GPU launchers should export it themselves)
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    if "torch" in sys.modules or os.environ.get("TRANSIT_AMD_OWN_HIP_RUNTIME"):
        return                                   # torch's runtime is mapped already / the caller wants /opt/rocm's
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    bundled = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(bundled):
        C.CDLL(bundled, mode=C.RTLD_GLOBAL)


def hip_library():
    """Load libtransit_hip.so or raise -- there is no CPU fallback."""
    global _hip
    if _hip is None:
        path = os.environ.get("TRANSIT_HIP_LIB") or lib_path("libtransit_hip.so")   # override: A/B builds
        if not os.path.exists(path):
            raise RuntimeError("HIP extension %s is missing; build it with "
                               "`python -m transit_amd.build` (hipcc --offload-arch=gfx950)" % path)
        _one_hip_runtime()
        lib = C.CDLL(path)
        _abi.bind(lib, _abi.HIP_HEADER, "trx_")
        if lib.trx_abi_version() != _abi.ABI_VERSION:
            raise RuntimeError("libtransit_hip.so ABI %d != binding %d" % (lib.trx_abi_version(), _abi.ABI_VERSION))
        # the runtime in this process may be the copy a PyTorch wheel bundles, not the toolchain's the
        # library was compiled against: a different MAJOR version is refused, a different minor one told
        built, running = C.c_int(0), C.c_int(0)
        if lib.trx_hip_versions(C.byref(built), C.byref(running)) == 0 and built.value and running.value:
            if built.value // 10000000 != running.value // 10000000:
                raise RuntimeError("libtransit_hip.so was built with HIP %d but runs on runtime %d (set "
                                   "TRANSIT_AMD_OWN_HIP_RUNTIME=1 to keep torch's bundled runtime out)" % (built.value, running.value))
            global HIP_VERSIONS                  # (built, running): 7.2 against the 7.0 of torch's wheel on this image -- same major
            HIP_VERSIONS = (built.value, running.value)
        _hip = lib
    return _hip


def _dp(x):
    """the double pointer of an array, or None for None (an output the caller does not want)"""
    return x.ctypes.data_as(_abi.c_double_p) if x is not None else None


def _vec(x) -> np.ndarray:
    """x (shifts, lags) as a flat C-contiguous double array"""
    return np.ascontiguousarray(x, dtype=np.float64).reshape(-1)


def _zeros(give, *shapes):
    """one zeroed double array per shape, or one None per shape where the caller does not want the outputs"""
    return [np.zeros(shape) if give else None for shape in shapes]


def _some(*pairs):
    """(value, wanted) pairs: the wanted values as a tuple, or the only one by itself"""
    out = tuple(v for v, wanted in pairs if wanted)
    return out if len(out) > 1 else out[0]


@dataclass(eq=False)
class Detrended:
    """What Engine.detrend_observed returns: basis [nseg, nexp, ncomp] the fitted time vectors U, coef [ncomp, npix] their
    column vectors, data [nexp, npix] the residuals now installed as the observed data (None after the undo), nsingular the
    columns the installed weighted filter's pivot rule makes dead, spectrum the injection run's spectrum (None without).
    Engine.pca_observed returns one with three more: eigen [nseg, ncomp] the components' eigenvalues of the Gram matrix,
    offdiag [nseg] the largest off-diagonal entry the sweeps left, nwhole [nseg] the columns that took part in the fit
    (None from detrend_observed, after the undo and with outputs=False).  Engine.regress_observed returns one with
    nsingular_fit, the columns whose fit of the given vectors had a singular pivot (None from the other two calls); its basis
    [nseg, nexp, nvec + nfit] holds the given vectors ahead of the fitted ones, its coef [nvec + nfit, npix] likewise."""

    basis: Optional[np.ndarray]
    coef: Optional[np.ndarray]
    data: Optional[np.ndarray]
    nsingular: int
    spectrum: Optional[np.ndarray] = None
    eigen: Optional[np.ndarray] = None
    offdiag: Optional[np.ndarray] = None
    nwhole: Optional[np.ndarray] = None
    nsingular_fit: Optional[int] = None


@dataclass(eq=False)
class Weighed:
    """What Engine.weigh_observed returns: variance [npix] every column's variance in time (+0: a dead column), median [nseg]
    every segment's median variance, weight [nexp, npix] the weights now in force (all three None after the undo or with
    outputs=False), nmasked the live columns the clip removed, nsingular the columns the installed weighted filter's pivot
    rule makes dead under the new weights (0 without a weighted filter)."""

    variance: Optional[np.ndarray]
    median: Optional[np.ndarray]
    weight: Optional[np.ndarray]
    nmasked: int
    nsingular: int


@dataclass(eq=False)
class Highpassed:
    """What Engine.highpass_observed returns: data [nexp, npix] the high-passed data now installed (+0 at the dead entries;
    None after the undo or with outputs=False), ndead the entries whose weight as set_observed installed it is not > 0."""

    data: Optional[np.ndarray]
    ndead: int


@dataclass(eq=False)
class Normalised:
    """What Engine.normalise_observed returns: data [nexp, npix] the normalised data now installed (+0 at the dead entries and
    in bad rows and columns), rowscale [nexp, nseg] every row's scale (+0: a bad row), centre [npix] every column's mean in
    time (+0: a bad column) -- the three None with outputs=False --, nclipped the entries the clip replaced, nbad the live
    entries that got +0, spectrum the injection run's spectrum (None without)."""

    data: Optional[np.ndarray]
    rowscale: Optional[np.ndarray]
    centre: Optional[np.ndarray]
    nclipped: int
    nbad: int
    spectrum: Optional[np.ndarray] = None


class Engine(CEngine):
    """MI355X engine: one handle = one GPU = one wavenumber shard."""

    def __init__(self, static: _abi.TrxStatic):
        self.nbands, self.npix, self.mom_shape = 0, 0, (0, 0)       # of the sets installed: none yet
        super().__init__(hip_library(), "trx_", static)

    def run_device(self, atm, opts, d_spectrum_ptr: int):
        self._call("run_device", C.byref(atm), C.byref(opts), C.c_void_p(d_spectrum_ptr), None)

    def _run_at(self, name, atm, opts, sh, out, spectrum: bool):
        """the run `name` at the shifts (or lags) sh into out: out, or (out, spectrum) with spectrum=True"""
        spec = np.zeros(self.nwn) if spectrum else None
        self._call(name, C.byref(atm), C.byref(opts), _dp(spec), int(sh.size), _dp(sh), _dp(out), None)
        return (out, spec) if spectrum else out

    def _inject(self, inject):
        """inject=(atm, opts, shifts, p0, p1) of an observed-set call, or None: the five leading arguments of its C
        signature (atm, opts, spectrum, nshift, shift), the flag, p0, p1 and the spectrum's buffer (None without)"""
        if inject is None:
            return (None, None, None, 0, None), 0, 0.0, 0.0, None
        atm, opts, shifts, p0, p1 = inject
        sh, spec = _vec(shifts), np.zeros(self.nwn)
        return (C.byref(atm), C.byref(opts), _dp(spec), int(sh.size), _dp(sh)), 1, float(p0), float(p1), spec

    def set_bands(self, bands):
        """trx_set_bands: install a band set (a list of transit_amd.bands.Band; empty: clear it)."""
        arr = _bands.to_c(bands)
        self._call("set_bands", len(bands), arr)
        self.nbands = len(bands)

    def run_bands(self, atm, opts, spectrum: bool = False):
        """trx_run_bands: the band sums [nbands, 2] of this shard -- and, with spectrum=True, (sums, spectrum),
        the spectrum bit for bit what run() gives."""
        sums = np.zeros((self.nbands, 2))
        spec = np.zeros(self.nwn) if spectrum else None
        self._call("run_bands", C.byref(atm), C.byref(opts), _dp(spec), _dp(sums), None)
        return (sums, spec) if spectrum else sums

    def run_contrib(self, atm, opts, spectrum: bool = False):
        """trx_run_contrib: (sums [nbands, 2], contrib [nbands, nlayer]) of this shard -- the band sums run_bands gives
        and the contribution function (eclipse) or transmittance profile (transit) of every band, rows in the
        atmosphere's layer order; with spectrum=True, (sums, contrib, spectrum)."""
        nb = self.nbands
        sums = np.zeros((nb, 2))
        contrib = np.zeros((nb, int(atm.nlayer)))
        spec = np.zeros(self.nwn) if spectrum else None
        self._call("run_contrib", C.byref(atm), C.byref(opts), _dp(spec), _dp(sums), _dp(contrib), None)
        return (sums, contrib, spec) if spectrum else (sums, contrib)

    def set_pixels(self, pixels):
        """trx_set_pixels: install a detector (a transit_amd.pixels.Pixels; None or an empty one: clear it)."""
        n = len(pixels) if pixels is not None else 0
        self._call("set_pixels", C.byref(_pixels.to_c(pixels)) if n else None)
        self.npix = n
        self.mom_shape = (0, 0)

    def run_pixels(self, atm, opts, shifts, spectrum: bool = False):
        """trx_run_pixels: the pairs [nshift, npix, 2] of this shard at the Doppler shifts given (nu_observed / nu_rest)
        -- and, with spectrum=True, (pairs, spectrum), the spectrum bit for bit what run() gives."""
        sh = _vec(shifts)
        return self._run_at("run_pixels", atm, opts, sh, np.zeros((sh.size, self.npix, 2)), spectrum)

    def set_observed(self, observed):
        """trx_set_observed: install the observed exposures (a transit_amd.xcor.Observed; None: clear them) over the
        pixel set in force.  set_pixels drops them."""
        self._call("set_observed", C.byref(observed.to_c()) if observed is not None else None)
        self.mom_shape = (observed.nexp, observed.nseg) if observed is not None else (0, 0)

    def run_moments(self, atm, opts, shifts, spectrum: bool = False):
        """trx_run_moments: the moments [nexp, nseg, 7] of the pixels at the exposures' Doppler shifts against the
        observed set (transit_amd.xcor) -- and, with spectrum=True, (moments, spectrum), the spectrum bit for bit what
        run() gives.  The pixel pairs stay on the device."""
        return self._run_at("run_moments", atm, opts, _vec(shifts), np.zeros(self.mom_shape + (_abi.NMOMENT,)), spectrum)

    def run_trail(self, atm, opts, lags, spectrum: bool = False):
        """trx_run_trail: the trail [nlag, nexp, nseg, 7] -- the moments of every exposure of the observed set against
        the model at every lag (nu_observed / nu_rest, as shifts are; transit_amd.xcor.lag_grid), row l bit for bit
        run_moments(atm, opts, [lags[l]] * nexp) -- and, with spectrum=True, (trail, spectrum), the spectrum bit for bit
        what run() gives.  An installed filter takes no part; the pixel pairs stay on the device."""
        lg = _vec(lags)
        return self._run_at("run_trail", atm, opts, lg, np.zeros((lg.size,) + self.mom_shape + (_abi.NMOMENT,)), spectrum)

    def run_velocity_map(self, atm, opts, vm, per: bool = False, spectrum: bool = False):
        """trx_run_velocity_map: the Kp-Vsys map [nkp, nvsys] of a transit_amd.xcor.VelocityMap -- run_trail at vm.lag and,
        on the device, xcor.trail_statistic and xcor.map_from_per of it; the trail stays there.  With per=True and/or
        spectrum=True a tuple (map[, per][, spectrum]): per [nlag, nexp] the statistic the map was made from (the map is
        xcor.map_from_per(per, vm) bit for bit), the spectrum bit for bit what run() gives."""
        m = np.zeros((vm.nkp, vm.nvsys))
        pr = np.zeros((vm.nlag, self.mom_shape[0])) if per else None
        spec = np.zeros(self.nwn) if spectrum else None
        self._call("run_velocity_map", C.byref(atm), C.byref(opts), _dp(spec), C.byref(vm.to_c()), _dp(m), _dp(pr), None)
        return _some((m, True), (pr, per), (spec, spectrum))

    def set_filter(self, filt):
        """trx_set_filter: install a detrending filter (a transit_amd.xcor.Filter; None: clear it) over the observed
        set in force.  set_observed and set_pixels drop it."""
        self._call("set_filter", C.byref(filt.to_c()) if filt is not None else None)

    def set_weighted_filter(self, wf) -> int:
        """trx_set_weighted_filter: install a weighted detrending filter (a transit_amd.xcor.WeightedFilter; None: clear
        the slot) over the observed set in force, in the slot set_filter fills: every pixel column is projected by least
        squares under its own weights.  Returns the number of columns the pivot rule makes dead.  run_filtered_moments
        and run_filtered_map then take it where they took the plain filter."""
        nsing = C.c_int64(0)
        self._call("set_weighted_filter", C.byref(wf.to_c()) if wf is not None else None, C.byref(nsing))
        return int(nsing.value)

    def run_filtered_moments(self, atm, opts, shifts, spectrum: bool = False, values: bool = False):
        """trx_run_filtered_moments: the moments [nexp, nseg, 7] of the FILTERED pixels (transit_amd.xcor) against the
        observed set; with spectrum=True and/or values=True a tuple (moments[, spectrum][, values]) -- the spectrum
        bit for bit what run() gives, the values [nexp, npix] the filtered model g' (NaN in dead columns).  Without
        values=True neither the pairs nor the values leave the device."""
        sh = _vec(shifts)
        mom = np.zeros(self.mom_shape + (_abi.NMOMENT,))
        spec = np.zeros(self.nwn) if spectrum else None
        val = np.zeros((mom.shape[0], self.npix)) if values else None
        self._call("run_filtered_moments", C.byref(atm), C.byref(opts), _dp(spec), int(sh.size), _dp(sh), _dp(val), _dp(mom), None)
        return _some((mom, True), (spec, spectrum), (val, values))

    def run_filtered_map(self, atm, opts, vm, lag_index: bool = False, spectrum: bool = False):
        """trx_run_filtered_map: the Kp-Vsys map [nkp, nvsys] of a transit_amd.xcor.VelocityMap with the installed filter
        applied to every cell's own model matrix -- the cell takes at every exposure the lag nearest to its velocity
        (xcor.nearest_lags), and its value is xcor.cell_value of run_filtered_moments at those lags; a cell with a
        velocity outside the lag grid is NaN.  With lag_index=True and/or spectrum=True a tuple
        (map[, lag_index][, spectrum]): lag_index [nkp, nvsys, nexp] int32 the lags taken (-1: outside), the spectrum
        bit for bit what run() gives.  One spectrum and one pixel pass, whatever the number of cells."""
        m = np.zeros((vm.nkp, vm.nvsys))
        idx = np.zeros((vm.nkp, vm.nvsys, self.mom_shape[0]), dtype=np.int32) if lag_index else None
        spec = np.zeros(self.nwn) if spectrum else None
        self._call("run_filtered_map", C.byref(atm), C.byref(opts), _dp(spec), C.byref(vm.to_c()), _dp(m),
                   idx.ctypes.data_as(_abi.c_int32_p) if lag_index else None, None)
        return _some((m, True), (idx, lag_index), (spec, spectrum))

    def set_highpass(self, hp):
        """trx_set_highpass: install a high-pass along the pixel axis (a transit_amd.xcor.HighPass; None: clear it) over
        the observed set in force.  run_moments, run_filtered_moments, run_trail and run_velocity_map then take the
        high-passed model; set_observed and set_pixels drop it."""
        self._call("set_highpass", C.byref(hp.to_c()) if hp is not None else None)

    def run_highpassed(self, atm, opts, shifts, spectrum: bool = False):
        """trx_run_highpassed: the high-passed model values [nshift, npix] (transit_amd.xcor.highpass_reference of
        run_pixels' pairs, bit for bit; NaN where the pixel is dead) at any number of shifts -- and, with
        spectrum=True, (values, spectrum), the spectrum bit for bit what run() gives."""
        sh = _vec(shifts)
        return self._run_at("run_highpassed", atm, opts, sh, np.zeros((sh.size, self.npix)), spectrum)

    def set_broadening(self, b):
        """trx_set_broadening: install a rotational broadening (a transit_amd.broaden.Rotation; None: clear it).  The
        pixel, moment and filtered-moment runs then sample the broadened spectrum; set_pixels does not drop it."""
        self._call("set_broadening", C.byref(_broaden.to_c(b)) if b is not None else None)

    def run_broadened(self, atm, opts, spectrum: bool = False):
        """trx_run_broadened: the broadened spectrum [nwn] -- and, with spectrum=True, (broadened, spectrum), the
        spectrum bit for bit what run() gives (never the broadened one)."""
        out = np.zeros(self.nwn)
        spec = np.zeros(self.nwn) if spectrum else None
        self._call("run_broadened", C.byref(atm), C.byref(opts), _dp(spec), _dp(out), None)
        return (out, spec) if spectrum else out

    def set_exposures(self, ex):
        """trx_set_exposures: install an exposure table (a transit_amd.exposures.Exposures; None or an empty one: clear
        it) over the observed set in force: a scale and a Doppler-smear half-width per exposure.  run_exposed, run_moments,
        run_filtered_moments and run_exposed_map then take it; set_observed and set_pixels drop it.  No device work: cheap per likelihood
        call."""
        n = len(ex) if ex is not None else 0
        self._call("set_exposures", C.byref(ex.to_c()) if n else None)

    def run_exposed(self, atm, opts, shifts, spectrum: bool = False):
        """trx_run_exposed: the pairs [nexp, npix, 2] of this shard at the exposures' Doppler shifts with the installed
        exposure table (transit_amd.exposures.reference) -- and, with spectrum=True, (pairs, spectrum), the spectrum bit
        for bit what run() gives."""
        sh = _vec(shifts)
        return self._run_at("run_exposed", atm, opts, sh, np.zeros((sh.size, self.npix, 2)), spectrum)

    def run_exposed_map(self, atm, opts, vm, lag_index: bool = False, nrows: bool = False, spectrum: bool = False):
        """trx_run_exposed_map: run_filtered_map UNDER the installed exposure table -- the model of exposure v scaled and
        smeared before the filter.  The Kp-Vsys map [nkp, nvsys] of a transit_amd.xcor.VelocityMap: a cell's value is
        xcor.cell_value of run_filtered_moments (table installed) at the lags nearest to its velocity; a cell with a
        velocity outside the lag grid is NaN.  With lag_index=True, nrows=True and/or spectrum=True a tuple
        (map[, lag_index][, nrows][, spectrum]): lag_index [nkp, nvsys, nexp] int32 the lags taken (-1: outside), nrows
        the (lag, exposure) pixel rows the call made (xcor.exposed_map_rows(vm)[3]), the spectrum bit for bit what run()
        gives.  One spectrum and one pixel pass, whatever the number of cells."""
        m = np.zeros((vm.nkp, vm.nvsys))
        idx = np.zeros((vm.nkp, vm.nvsys, self.mom_shape[0]), dtype=np.int32) if lag_index else None
        spec = np.zeros(self.nwn) if spectrum else None
        nr = C.c_int64(-1)
        self._call("run_exposed_map", C.byref(atm), C.byref(opts), _dp(spec), C.byref(vm.to_c()), _dp(m),
                   idx.ctypes.data_as(_abi.c_int32_p) if lag_index else None, C.byref(nr), None)
        return _some((m, True), (idx, lag_index), (int(nr.value), nrows), (spec, spectrum))

    def detrend_observed(self, ncomp: int, niter: int = 10, inject=None, outputs: bool = True) -> "Detrended":
        """trx_detrend_observed: SYSREM on the observed exposures themselves, on the device, always from the RAW data of
        set_observed -- ncomp components of niter alternations per segment (xcor.sysrem_reference, bit for bit).  inject:
        None, or (atm, opts, shifts, p0, p1): the model of this handle's pixel stage at the exposures' shifts is multiplied
        into the raw data first, f0 = F * (p0 g + p1) (xcor.inject_reference of run_exposed's pairs, or run_pixels' without
        a table).  The residuals become the observed data and the weighted filter of the fitted basis the filter;
        run_filtered_moments, run_filtered_map and run_exposed_map then are the recovery.  ncomp = 0 is the undo: the raw
        data back, the filter slot cleared.  Returns a Detrended: basis [nseg, nexp, ncomp], coef [ncomp, npix], data
        [nexp, npix] (the residuals now installed), nsingular, and spectrum (None without an injection).  outputs=False
        leaves basis, coef and data on the device (None in the result): the loop of an injection-recovery test needs
        only the map that follows."""
        (nexp, nseg), npix = self.mom_shape, self.npix
        run, flag, p0, p1, spec = self._inject(inject)
        dt = _abi.TrxDetrend(int(ncomp), int(niter), flag, 0, p0, p1)
        n = max(int(ncomp), 0) if outputs else 0
        basis, coef, data = _zeros(n, (nseg, nexp, n), (n, npix), (nexp, npix))
        nsing = C.c_int64(0)
        self._call("detrend_observed", *run, C.byref(dt), _dp(basis), _dp(coef), _dp(data), C.byref(nsing), None)
        return Detrended(basis, coef, data, int(nsing.value), spec)

    def pca_observed(self, ncomp: int, nsweep: int = 8, inject=None, outputs: bool = True) -> "Detrended":
        """trx_pca_observed: detrend_observed with a principal-component analysis in time in SYSREM's place, on the device,
        always from the RAW data of set_observed -- per segment the ncomp leading eigenvectors of the Gram matrix of the
        whole columns (those no live exposure masks) by nsweep Jacobi sweeps in a fixed order (xcor.pca_reference, bit for
        bit), removed from every column.  inject, the outcome, outputs=False and the undo (ncomp = 0) are
        detrend_observed's; either call undoes either.  Scattered masks keep a column out of the fit: SYSREM is the tool
        for those.  Returns a Detrended with eigen [nseg, ncomp], offdiag [nseg] and nwhole [nseg] beside basis, coef and
        data (all None after the undo or with outputs=False)."""
        (nexp, nseg), npix = self.mom_shape, self.npix
        run, flag, p0, p1, spec = self._inject(inject)
        pc = _abi.TrxPca(int(ncomp), int(nsweep), flag, 0, p0, p1)
        n = max(int(ncomp), 0) if outputs else 0
        basis, coef, data, eigen, offdiag = _zeros(n, (nseg, nexp, n), (n, npix), (nexp, npix), (nseg, n), nseg)
        nwhole = np.zeros(nseg, dtype=np.int64) if n else None
        nsing = C.c_int64(0)
        self._call("pca_observed", *run, C.byref(pc), _dp(basis), _dp(coef), _dp(data), _dp(eigen), _dp(offdiag),
                   nwhole.ctypes.data_as(_abi.c_int64_p) if n else None, C.byref(nsing), None)
        return Detrended(basis, coef, data, int(nsing.value), spec, eigen, offdiag, nwhole)

    def regress_observed(self, vectors, nfit: int = 0, niter: int = 10, inject=None, outputs: bool = True) -> "Detrended":
        """trx_regress_observed: detrend_observed with a weighted least-squares fit of GIVEN time vectors in SYSREM's place,
        on the device, always from the RAW data of set_observed -- every pixel column regressed on its segment's vectors
        under its own weights (xcor.regress_reference, bit for bit), then nfit SYSREM components of niter alternations on
        what is left (xcor.sysrem_reference of those residuals).  vectors: [nseg, nexp, nvec], or [nexp, nvec] for all
        segments (xcor.time_basis of the airmass, the basis of an earlier detrend_observed, ...); None or nvec = 0 is the
        undo.  inject, the outcome and outputs=False are detrend_observed's; any of the detrending calls undoes any other.
        The residuals become the observed data and the weighted filter of the merged basis the filter -- with nfit = 0 by
        the very factor the fit used.  Returns a Detrended with nsingular_fit beside basis [nseg, nexp, nvec + nfit], coef
        [nvec + nfit, npix], data, nsingular and spectrum."""
        (nexp, nseg), npix = self.mom_shape, self.npix
        vec = None
        if vectors is not None:
            vec = np.asarray(vectors, dtype=np.float64)
            if vec.ndim == 2:
                vec = np.broadcast_to(vec[None, :, :], (nseg,) + vec.shape)
            if vec.ndim != 3 or (vec.shape[2] and vec.shape[:2] != (nseg, nexp)):
                raise ValueError("Engine.regress_observed: vectors of shape [nseg][nexp][nvec] or [nexp][nvec]")
            vec = np.ascontiguousarray(vec)
        nvec = int(vec.shape[2]) if vec is not None else 0
        run, flag, p0, p1, spec = self._inject(inject)
        rg = _abi.TrxRegress(nvec, int(nfit), int(niter), flag, p0, p1, _dp(vec) if nvec else None)
        n = nvec + max(int(nfit), 0) if outputs and nvec else 0
        basis, coef, data = _zeros(n, (nseg, nexp, n), (n, npix), (nexp, npix))
        nfs, nsing = C.c_int64(0), C.c_int64(0)
        self._call("regress_observed", *run, C.byref(rg), _dp(basis), _dp(coef), _dp(data), C.byref(nfs), C.byref(nsing), None)
        return Detrended(basis, coef, data, int(nsing.value), spec, nsingular_fit=int(nfs.value))

    def weigh_observed(self, kind: int, clip: float = 0.0, min_live: int = 2, outputs: bool = True) -> "Weighed":
        """trx_weigh_observed: the column-scatter weights of the observed set, on the device, from the data installed (the
        residuals of detrend_observed, or the raw set) and ALWAYS from the weights as set_observed installed them
        (xcor.scatter_reference, bit for bit).  kind: _abi.SCATTER_VARIANCE (w' = 1 / var_p on the kept columns' live
        entries), SCATTER_MASK (w' = W on the kept columns) or SCATTER_NONE, the undo: set_observed's weights back in force.
        clip: 0 (none) or >= 1: a live column is kept if var_p <= clip^2 times its segment's median variance; min_live: the
        entries a live column needs.  The new weights become the observed set's, and an installed weighted filter is
        factorised again against them; run_filtered_moments, run_filtered_map and run_exposed_map then run under them.
        Returns a Weighed: variance [npix], median [nseg], weight [nexp, npix], nmasked, nsingular.  outputs=False leaves the
        three arrays on the device (None in the result)."""
        (nexp, nseg), npix = self.mom_shape, self.npix
        sc = _abi.TrxScatter(int(kind), int(min_live), float(clip))
        var, med, w = _zeros(bool(outputs) and int(kind) != _abi.SCATTER_NONE, npix, nseg, (nexp, npix))
        nm, nsing = C.c_int64(0), C.c_int64(0)
        self._call("weigh_observed", C.byref(sc), _dp(var), _dp(med), _dp(w), C.byref(nm), C.byref(nsing))
        return Weighed(var, med, w, int(nm.value), int(nsing.value))

    def highpass_observed(self, apply: bool = True, outputs: bool = True) -> "Highpassed":
        """trx_highpass_observed: the observed set's own data through the installed high-pass (set_highpass), on the device
        -- from the data as the last detrend_observed left them (its residuals, or the raw set), never from an earlier
        high-pass, and with live = (W > 0) of the weights as set_observed installed them (xcor.highpass_observed_reference,
        bit for bit).  The result becomes the observed data; weights, filter, high-pass, exposure table and gain stay.
        apply=False is the undo.  Every successful detrend_observed discards the high-pass: the order is detrend, high-pass,
        weigh, map.  Returns a Highpassed: data [nexp, npix] and ndead.  outputs=False leaves the data on the device."""
        data, = _zeros(bool(outputs) and bool(apply), (self.mom_shape[0], self.npix))
        nd = C.c_int64(0)
        self._call("highpass_observed", 1 if apply else 0, _dp(data), C.byref(nd))
        return Highpassed(data, int(nd.value))

    def set_normalise(self, nm):
        """trx_set_normalise: install the recipe of step 1b of the detrending calls (a transit_amd.xcor.Normalise; None:
        clear it) over the observed set in force: every (exposure, segment) row divided by its quantile, every column
        divided by or reduced by its mean in time, single entries clipped.  No device work, and nothing in force changes:
        detrend_observed, pca_observed and normalise_observed take the recipe from their next call on, between the
        injection and the fit.  set_observed and set_pixels drop it."""
        self._call("set_normalise", C.byref(nm.to_c()) if nm is not None else None)

    def normalise_observed(self, inject=None, outputs: bool = True) -> "Normalised":
        """trx_normalise_observed: "the detrend of zero components" -- the installed recipe (set_normalise) over the RAW data
        of set_observed, or over the injected data (inject as detrend_observed takes it), on the device
        (xcor.normalise_reference, bit for bit).  The result becomes the observed data, the filter slot is cleared and the
        weights of set_observed go back in force; detrend_observed(0) undoes it, and detrend_observed, pca_observed and this
        call undo one another.  The weights are NOT changed: rows with rowscale == 0, bad columns and columns of a low
        centre are for the driver to mask in set_observed.  Returns a Normalised: data [nexp, npix], rowscale [nexp, nseg],
        centre [npix], nclipped, nbad and spectrum.  outputs=False leaves the three arrays on the device."""
        (nexp, nseg), npix = self.mom_shape, self.npix
        run, flag, p0, p1, spec = self._inject(inject)
        data, scale, centre = _zeros(outputs, (nexp, npix), (nexp, nseg), npix)
        nc, nb = C.c_int64(0), C.c_int64(0)
        self._call("normalise_observed", *run, flag, p0, p1, _dp(data), _dp(scale), _dp(centre), C.byref(nc), C.byref(nb), None)
        return Normalised(data, scale, centre, int(nc.value), int(nb.value), spec)

    def gather(self, d_slice_ptr: int, d_all_ptr: int, count: int):
        """trx_gather: the one exchange of a sharded job -- every rank's `count` doubles (device
        memory) into d_all in rank order, ncclAllGather over the handle's communicator (a device
        copy without one)."""
        self._call("gather", C.c_void_p(d_slice_ptr), C.c_void_p(d_all_ptr), int(count))


def _rows(a):
    """one double pointer per row of a [K, ...] (None: no array; K = 0: one unused entry, ctypes has no empty array)"""
    return (_abi.c_double_p * max(len(a), 1))(*[_dp(row) for row in a]) if a is not None else None


def _per_atmosphere(who: str, what: str, x, k: int) -> np.ndarray:
    """x as [K][n] doubles, one row per atmosphere; what: "shifts of shape [K][nshift]", for the refusal"""
    a = np.ascontiguousarray(x, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] != k:
        raise ValueError("Batch.%s: %s, one row per atmosphere" % (who, what))
    return a


class Batch:
    """trx_batch: `ways` handles made from one description, each with a host thread of its own inside
    the library; run(atms, opts) deals the atmospheres to them (trx_run_batch) and returns their
    spectra -- each one what Engine.run gives for its atmosphere, bit for bit."""

    def __init__(self, static: _abi.TrxStatic, ways: int = 3):
        lib = hip_library()
        self._lib, self._b = lib, C.c_void_p()
        self.nwn = int(static.wn_hi - static.wn_lo)
        self.nbands, self.npix, self.mom_shape = 0, 0, (0, 0)       # of the sets installed: none yet
        rc = lib.trx_batch_create(C.byref(static), int(ways), C.byref(self._b))
        if rc != 0:
            raise EngineError(rc, "trx_batch_create", self._err())

    def _err(self) -> str:
        return (self._lib.trx_last_error(None) or b"").decode(errors="replace")

    def _set(self, name: str, *args):
        """the batch function `name` on the batch, a non-zero status raised with the batch's last error"""
        rc = getattr(self._lib, name)(self._b, *args)
        if rc != 0:
            raise EngineError(rc, name, self._err())

    def _call(self, name: str, atms, opts: _abi.TrxOpts, *args):
        """the batch function `name` over the atmospheres: args are what follows opts in its C signature"""
        k = len(atms)
        self._set(name, k, (_abi.TrxAtm * max(k, 1))(*atms), C.byref(opts), *args)

    def run(self, atms, opts: _abi.TrxOpts) -> np.ndarray:
        out = np.zeros((len(atms), self.nwn))
        self._call("trx_run_batch", atms, opts, _rows(out))
        return out

    def set_bands(self, bands):
        """trx_batch_set_bands: the same band set on every handle of the batch, or on none."""
        arr = _bands.to_c(bands)
        self._set("trx_batch_set_bands", len(bands), arr)
        self.nbands = len(bands)

    def run_bands(self, atms, opts: _abi.TrxOpts) -> np.ndarray:
        """trx_run_batch_bands: [K, nbands, 2], each atmosphere's sums what Engine.run_bands gives, bit for bit."""
        out = np.zeros((len(atms), self.nbands, 2))
        self._call("trx_run_batch_bands", atms, opts, _rows(out))
        return out

    def run_contrib(self, atms, opts: _abi.TrxOpts):
        """trx_run_batch_contrib: ([K, nbands, 2], [K, nbands, nlayer]), each atmosphere's pair what
        Engine.run_contrib gives, bit for bit (the atmospheres of one call share nlayer here)."""
        k = len(atms)
        nb = self.nbands
        nl = int(atms[0].nlayer) if k else 0
        if any(int(a.nlayer) != nl for a in atms):
            raise ValueError("Batch.run_contrib: atmospheres of different nlayer; call it once per nlayer")
        sums, contrib = np.zeros((k, nb, 2)), np.zeros((k, nb, nl))
        self._call("trx_run_batch_contrib", atms, opts, _rows(sums), _rows(contrib))
        return sums, contrib

    def set_pixels(self, pixels):
        """trx_batch_set_pixels: the same detector on every handle of the batch, or on none."""
        n = len(pixels) if pixels is not None else 0
        self._set("trx_batch_set_pixels", C.byref(_pixels.to_c(pixels)) if n else None)
        self.npix = n
        self.mom_shape = (0, 0)

    def run_pixels(self, atms, opts: _abi.TrxOpts, shifts) -> np.ndarray:
        """trx_run_batch_pixels: [K, nshift, npix, 2] for shifts of shape [K][nshift] (atmosphere j at its own shifts),
        each atmosphere's pairs what Engine.run_pixels gives, bit for bit."""
        sh = _per_atmosphere("run_pixels", "shifts of shape [K][nshift]", shifts, len(atms))
        out = np.zeros((len(atms), sh.shape[1], self.npix, 2))
        self._call("trx_run_batch_pixels", atms, opts, int(sh.shape[1]), _rows(sh), _rows(out))
        return out

    def set_observed(self, observed):
        """trx_batch_set_observed: the same observed set on every handle of the batch, or on none."""
        self._set("trx_batch_set_observed", C.byref(observed.to_c()) if observed is not None else None)
        self.mom_shape = (observed.nexp, observed.nseg) if observed is not None else (0, 0)

    def run_moments(self, atms, opts: _abi.TrxOpts, shifts) -> np.ndarray:
        """trx_run_batch_moments: [K, nexp, nseg, 7] for shifts of shape [K][nexp] (atmosphere j at its own shifts),
        each atmosphere's moments what Engine.run_moments gives, bit for bit."""
        sh = _per_atmosphere("run_moments", "shifts of shape [K][nexp]", shifts, len(atms))
        out = np.zeros((len(atms),) + self.mom_shape + (_abi.NMOMENT,))
        self._call("trx_run_batch_moments", atms, opts, int(sh.shape[1]), _rows(sh), _rows(out))
        return out

    def run_trail(self, atms, opts: _abi.TrxOpts, lags) -> np.ndarray:
        """trx_run_batch_trail: [K, nlag, nexp, nseg, 7] for lags of shape [K][nlag] (atmosphere j at its own lags), each
        atmosphere's trail what Engine.run_trail gives, bit for bit."""
        lg = _per_atmosphere("run_trail", "lags of shape [K][nlag]", lags, len(atms))
        out = np.zeros((len(atms), lg.shape[1]) + self.mom_shape + (_abi.NMOMENT,))
        self._call("trx_run_batch_trail", atms, opts, int(lg.shape[1]), _rows(lg), _rows(out))
        return out

    def run_velocity_map(self, atms, opts: _abi.TrxOpts, vm, per: bool = False):
        """trx_run_batch_velocity_map: the maps [K, nkp, nvsys] of one transit_amd.xcor.VelocityMap for all atmospheres
        -- with per=True, (maps, per [K, nlag, nexp]) --, each atmosphere's what Engine.run_velocity_map gives, bit for
        bit."""
        m = np.zeros((len(atms), vm.nkp, vm.nvsys))
        pr = np.zeros((len(atms), vm.nlag, self.mom_shape[0])) if per else None
        self._call("trx_run_batch_velocity_map", atms, opts, C.byref(vm.to_c()), _rows(m), _rows(pr))
        return (m, pr) if per else m

    def set_filter(self, filt):
        """trx_batch_set_filter: the same filter on every handle of the batch, or on none."""
        self._set("trx_batch_set_filter", C.byref(filt.to_c()) if filt is not None else None)

    def set_weighted_filter(self, wf):
        """trx_batch_set_weighted_filter: the same weighted filter on every handle of the batch, or on none."""
        self._set("trx_batch_set_weighted_filter", C.byref(wf.to_c()) if wf is not None else None)

    def set_highpass(self, hp):
        """trx_batch_set_highpass: the same high-pass on every handle of the batch, or on none."""
        self._set("trx_batch_set_highpass", C.byref(hp.to_c()) if hp is not None else None)

    def run_filtered_moments(self, atms, opts: _abi.TrxOpts, shifts) -> np.ndarray:
        """trx_run_batch_filtered_moments: [K, nexp, nseg, 7] for shifts of shape [K][nexp], each atmosphere's moments
        what Engine.run_filtered_moments gives, bit for bit."""
        sh = _per_atmosphere("run_filtered_moments", "shifts of shape [K][nexp]", shifts, len(atms))
        out = np.zeros((len(atms),) + self.mom_shape + (_abi.NMOMENT,))
        self._call("trx_run_batch_filtered_moments", atms, opts, int(sh.shape[1]), _rows(sh), _rows(out))
        return out

    def run_filtered_map(self, atms, opts: _abi.TrxOpts, vm) -> np.ndarray:
        """trx_run_batch_filtered_map: the maps [K, nkp, nvsys] of one transit_amd.xcor.VelocityMap for all atmospheres,
        each atmosphere's what Engine.run_filtered_map gives, bit for bit."""
        m = np.zeros((len(atms), vm.nkp, vm.nvsys))
        self._call("trx_run_batch_filtered_map", atms, opts, C.byref(vm.to_c()), _rows(m))
        return m

    def set_broadening(self, b):
        """trx_batch_set_broadening: one transit_amd.broaden.Rotation for every atmosphere of the following pixel,
        moment, filtered-moment and broadened runs, or a list with one per atmosphere (None or an empty list: clear);
        all entries are accepted, or none is kept."""
        bs = [] if b is None else list(b) if isinstance(b, (list, tuple)) else [b]
        arr = (_abi.TrxBroadening * max(len(bs), 1))(*[_broaden.to_c(x) for x in bs])
        self._set("trx_batch_set_broadening", len(bs), arr)

    def run_broadened(self, atms, opts: _abi.TrxOpts) -> np.ndarray:
        """trx_run_batch_broadened: [K, nwn], each atmosphere's broadened spectrum what Engine.run_broadened gives with
        that atmosphere's broadening, bit for bit."""
        out = np.zeros((len(atms), self.nwn))
        self._call("trx_run_batch_broadened", atms, opts, _rows(out))
        return out

    def set_exposures(self, ex):
        """trx_batch_set_exposures: one transit_amd.exposures.Exposures for every atmosphere of the following exposed,
        moment and filtered-moment runs, or a list with one per atmosphere (None or an empty list: clear); all entries
        are accepted, or none is kept.  The arrays are copied."""
        xs = [] if ex is None else list(ex) if isinstance(ex, (list, tuple)) else [ex]
        arr = (_abi.TrxExposures * max(len(xs), 1))(*[x.to_c() for x in xs])
        self._set("trx_batch_set_exposures", len(xs), arr)

    def run_exposed(self, atms, opts: _abi.TrxOpts, shifts) -> np.ndarray:
        """trx_run_batch_exposed: [K, nexp, npix, 2] for shifts of shape [K][nexp] (atmosphere j at its own shifts and
        with its own table), each atmosphere's pairs what Engine.run_exposed gives, bit for bit."""
        sh = _per_atmosphere("run_exposed", "shifts of shape [K][nexp]", shifts, len(atms))
        out = np.zeros((len(atms), sh.shape[1], self.npix, 2))
        self._call("trx_run_batch_exposed", atms, opts, int(sh.shape[1]), _rows(sh), _rows(out))
        return out

    def run_exposed_map(self, atms, opts: _abi.TrxOpts, vm) -> np.ndarray:
        """trx_run_batch_exposed_map: the maps [K, nkp, nvsys] of one transit_amd.xcor.VelocityMap for all atmospheres
        under the batch's exposure tables (one for all, or atmosphere j with its own), each atmosphere's what
        Engine.run_exposed_map gives, bit for bit."""
        m = np.zeros((len(atms), vm.nkp, vm.nvsys))
        self._call("trx_run_batch_exposed_map", atms, opts, C.byref(vm.to_c()), _rows(m))
        return m

    def close(self):
        if self._b:
            self._lib.trx_batch_destroy(self._b)
            self._b = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


LOG_FN = _abi.LOG_FN
_log_keep = None


def set_log(callback, max_level: int = 3):
    """Route the library's messages (trx_set_log) to callback(level, text); None = silent."""
    global _log_keep
    lib = hip_library()
    if callback is None:
        _log_keep = LOG_FN(0)
    else:
        _log_keep = LOG_FN(lambda lvl, msg, _u: callback(int(lvl), msg.decode(errors="replace")))
    lib.trx_set_log(_log_keep, None, int(max_level))


def device_count() -> int:
    return int(hip_library().trx_device_count())
