"""ctypes mirror of include/transit_hip.h (plain C structs, no torch types)."""
from __future__ import annotations

import ctypes as C

ABI_VERSION = 5

c_double_p = C.POINTER(C.c_double)
c_int16_p = C.POINTER(C.c_int16)
c_int32_p = C.POINTER(C.c_int32)
c_int64_p = C.POINTER(C.c_int64)
c_float_p = C.POINTER(C.c_float)
c_uint8_p = C.POINTER(C.c_uint8)

SOL_ECLIPSE, SOL_TRANSIT = 0, 1

STATUS = {
    0: "TRX_OK", -1: "TRX_E_ARG", -2: "TRX_E_NOMEM", -3: "TRX_E_HIP", -4: "TRX_E_NODEVICE",
    -5: "TRX_E_RANGE", -6: "TRX_E_UNSUPPORTED", -7: "TRX_E_ORDER", -8: "TRX_E_NOTREACHED",
}


class TrxCia(C.Structure):
    _fields_ = [("nspec", C.c_int32), ("mol", C.c_int32 * 2), ("nwave", C.c_int32),
                ("ntemp", C.c_int32), ("wn", c_double_p), ("temp", c_double_p), ("cs", c_double_p)]


class TrxOpacityGrid(C.Structure):
    _fields_ = [("nmol", C.c_int64), ("ntemp", C.c_int64), ("nlayer", C.c_int64), ("nwave", C.c_int64),
                ("mol_index", c_int32_p), ("temp", c_double_p), ("o", c_double_p)]


class TrxStatic(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("device", C.c_int32),
        ("wn_i", C.c_double), ("wn_d", C.c_double), ("nwn", C.c_int64), ("osamp", C.c_int32),
        ("nown", C.c_int64), ("wn_lo", C.c_int64), ("wn_hi", C.c_int64),
        ("ndop", C.c_int32), ("nlor", C.c_int32),
        ("dmin", C.c_float), ("dmax", C.c_float), ("lmin", C.c_float), ("lmax", C.c_float),
        ("timesalpha", C.c_float),
        ("nlines", C.c_int64), ("wl_um", c_double_p), ("isoid", c_int16_p), ("elow", c_double_p),
        ("gf", c_double_p),
        ("niso", C.c_int32), ("iso_mass", c_double_p), ("iso_ratio", c_double_p),
        ("iso_imol", c_int32_p),
        ("nmol", C.c_int32), ("mol_mass", c_double_p), ("mol_radius", c_double_p),
        ("mol_pol", c_double_p), ("mol_is_h2", c_int32_p),
        ("ncia", C.c_int32), ("cia", C.POINTER(TrxCia)),
        ("comm", C.c_void_p), ("nranks", C.c_int32), ("rank", C.c_int32),
        ("ogrid", C.POINTER(TrxOpacityGrid)),
    ]


class TrxAtm(C.Structure):
    _fields_ = [("nlayer", C.c_int32), ("rad_fct", C.c_double), ("radius", c_double_p),
                ("temp", c_double_p), ("press", c_double_p), ("density", c_double_p),
                ("abund", c_double_p), ("zpart", c_double_p)]


class TrxOpts(C.Structure):
    _fields_ = [
        ("solution", C.c_int32), ("toomuch", C.c_double), ("ethresh", C.c_double),
        ("wn_fct", C.c_double), ("nangles", C.c_int32), ("angles_deg", c_double_p),
        ("starrad_cm", C.c_double), ("transparent", C.c_int32), ("modlevel", C.c_int32),
        ("cloud_flag", C.c_int32), ("cloud_ext", C.c_double), ("cloud_top", C.c_double),
        ("cloud_bot", C.c_double), ("cloud_gamma", C.c_double), ("cloud_Q", C.c_double),
        ("cloud_r", C.c_double), ("cloud_sig", C.c_double), ("cloud_refwn", C.c_double),
        ("scat_flag", C.c_int32), ("scat_logext", C.c_double),
        ("layer_chunk", C.c_int32), ("eager", C.c_int32), ("profile", C.c_int32),
    ]


class TrxDebug(C.Structure):
    _fields_ = [("e", c_double_p), ("e_cs", c_double_p), ("tau", c_double_p), ("last", c_int64_p),
                ("intens", c_double_p), ("computed", c_uint8_p),
                ("er", c_double_p), ("e_scat", c_double_p), ("e_cloud", c_double_p)]


BAND_WEIGHTS, BAND_GAUSS = 0, 1


class TrxBand(C.Structure):
    _fields_ = [("kind", C.c_int32), ("pad", C.c_int32), ("first", C.c_int64), ("n", C.c_int64),
                ("weights", c_double_p), ("centre", C.c_double), ("fwhm", C.c_double), ("cut", C.c_double)]


class TrxPixels(C.Structure):
    _fields_ = [("npix", C.c_int64), ("centre", c_double_p), ("fwhm", c_double_p), ("cut", C.c_double)]


NMOMENT = 7


class TrxObserved(C.Structure):
    _fields_ = [("nexp", C.c_int32), ("nseg", C.c_int32), ("seg_first", c_int64_p), ("data", c_double_p),
                ("weight", c_double_p), ("gain", c_double_p)]


FILTER_MAX = 16


class TrxFilter(C.Structure):
    _fields_ = [("ncomp", C.c_int32), ("pad", C.c_int32), ("fwd", c_double_p), ("back", c_double_p)]


WFILTER_PIVOT = 2.0 ** -26      # TRX_WFILTER_PIVOT: a pivot at or below this share of its diagonal entry is singular


class TrxWfilter(C.Structure):
    _fields_ = [("ncomp", C.c_int32), ("pad", C.c_int32), ("basis", c_double_p)]


SYSREM_MAX_ITER = 64            # TRX_SYSREM_MAX_ITER: the most alternations per component of trx_detrend_observed


class TrxDetrend(C.Structure):
    _fields_ = [("ncomp", C.c_int32), ("niter", C.c_int32), ("inject", C.c_int32), ("pad", C.c_int32),
                ("p0", C.c_double), ("p1", C.c_double)]


PCA_MAX_SWEEP = 32              # TRX_PCA_MAX_SWEEP: the most Jacobi sweeps of trx_pca_observed
PCA_MAX_EXP = 128               # TRX_PCA_MAX_EXP: the most exposures of a set trx_pca_observed takes


class TrxPca(C.Structure):
    _fields_ = [("ncomp", C.c_int32), ("nsweep", C.c_int32), ("inject", C.c_int32), ("pad", C.c_int32),
                ("p0", C.c_double), ("p1", C.c_double)]


class TrxRegress(C.Structure):
    _fields_ = [("nvec", C.c_int32), ("nfit", C.c_int32), ("niter", C.c_int32), ("inject", C.c_int32),
                ("p0", C.c_double), ("p1", C.c_double), ("vectors", c_double_p)]


SCATTER_NONE, SCATTER_VARIANCE, SCATTER_MASK = 0, 1, 2      # TRX_SCATTER_*: the kinds of trx_weigh_observed


class TrxScatter(C.Structure):
    _fields_ = [("kind", C.c_int32), ("min_live", C.c_int32), ("clip", C.c_double)]


NORM_ROW_NONE, NORM_ROW_QUANTILE = 0, 1                     # TRX_NORM_ROW_*: the row kinds of trx_set_normalise
NORM_COL_NONE, NORM_COL_DIVIDE, NORM_COL_RATIO, NORM_COL_SUBTRACT = 0, 1, 2, 3      # TRX_NORM_COL_*: its column kinds


class TrxNormalise(C.Structure):
    _fields_ = [("row_kind", C.c_int32), ("col_kind", C.c_int32), ("quantile", C.c_double), ("clip", C.c_double)]


HIGHPASS_MAX_HALF = 1024


class TrxHighpass(C.Structure):
    _fields_ = [("half", C.c_int32), ("pad", C.c_int32), ("taps", c_double_p)]


STAT_CCF, STAT_LOGLIKE_BL19, STAT_CHI2 = 1, 2, 3


class TrxVmap(C.Structure):
    _fields_ = [("stat", C.c_int32), ("nlag", C.c_int32), ("p0", C.c_double), ("p1", C.c_double),
                ("lag", c_double_p), ("lag_kms", c_double_p), ("nkp", C.c_int32), ("nvsys", C.c_int32),
                ("kp", c_double_p), ("vsys", c_double_p), ("orbit", c_double_p), ("offset", c_double_p)]


BROADEN_NONE, BROADEN_ROTATION = 0, 1
BROADEN_MAX_HALF = 2048


class TrxBroadening(C.Structure):
    _fields_ = [("kind", C.c_int32), ("pad", C.c_int32), ("beta", C.c_double), ("limb", C.c_double)]


SMEAR_MAX = 0.01


class TrxExposures(C.Structure):
    _fields_ = [("nexp", C.c_int32), ("pad", C.c_int32), ("scale", c_double_p), ("smear", c_double_p)]


class TrxStats(C.Structure):
    _fields_ = [
        ("nlines_inrange", C.c_int64), ("ngroups", C.c_int64), ("nadd", C.c_int64),
        ("layers_swept", C.c_int64), ("neval", C.c_int64), ("nskip", C.c_int64),
        ("sum_bins", C.c_int64), ("table_floats", C.c_int64),
        ("ms_create_table", C.c_double), ("ms_run_total", C.c_double), ("ms_sweep", C.c_double),
        ("ms_k_sweep", C.c_double), ("ms_k_walk", C.c_double), ("ms_k_accum", C.c_double),
        ("sweep_launches", C.c_int64),
        ("ms_tau", C.c_double), ("ms_cia", C.c_double), ("ms_host_total", C.c_double),
        ("ms_spectrum", C.c_double), ("ncandidates", C.c_int64), ("walk_steps", C.c_int64), ("walk_records", C.c_int64), ("walk_record_lanes", C.c_int64),
        ("walk_layers", C.c_int64), ("sum_bins_walk", C.c_int64),
        ("walk_form_steps", C.c_int64 * 3), ("walk_form_layers", C.c_int64 * 3), ("walk_form_record_lanes", C.c_int64 * 3),
        ("walk_form_bins", C.c_int64 * 3), ("ms_k_walk_form", C.c_double * 3), ("ms_walk_span", C.c_double),
    ]

    def as_dict(self):
        return {name: (list(getattr(self, name)) if hasattr(getattr(self, name), "__len__") else getattr(self, name))
                for name, _ in self._fields_}


def bind_engine_api(lib, prefix: str = "trx_"):
    """Declare argtypes/restypes of the create/run/destroy family on *lib*.
    The same struct layouts serve any library exporting this ABI shape."""
    f = lambda n: getattr(lib, prefix + n)
    f("create").argtypes = [C.POINTER(TrxStatic), C.POINTER(C.c_void_p)]
    f("create").restype = C.c_int
    f("run").argtypes = [C.c_void_p, C.POINTER(TrxAtm), C.POINTER(TrxOpts), c_double_p,
                         C.POINTER(TrxDebug)]
    f("run").restype = C.c_int
    f("destroy").argtypes = [C.c_void_p]
    f("destroy").restype = None
    f("get_stats").argtypes = [C.c_void_p, C.POINTER(TrxStats)]
    f("get_stats").restype = C.c_int
    f("table_info").argtypes = [C.c_void_p, c_int64_p, c_int64_p, c_int64_p]
    f("table_info").restype = C.c_int
    f("table_copy").argtypes = [C.c_void_p, c_float_p]
    f("table_copy").restype = C.c_int
    f("width_grids").argtypes = [C.c_void_p, c_double_p, c_double_p]
    f("width_grids").restype = C.c_int
    f("sweep_permol").argtypes = [C.c_void_p, C.c_int32, c_double_p, c_double_p, c_double_p, C.c_double,
                                  C.c_int32, c_int32_p, c_double_p]
    f("sweep_permol").restype = C.c_int
    return lib


def bind_bands_api(lib):
    """argtypes/restypes of the band entry points (trx_set_bands, trx_run_bands and their batch forms)."""
    lib.trx_set_bands.argtypes = [C.c_void_p, C.c_int32, C.POINTER(TrxBand)]
    lib.trx_set_bands.restype = C.c_int
    lib.trx_run_bands.argtypes = [C.c_void_p, C.POINTER(TrxAtm), C.POINTER(TrxOpts), c_double_p, c_double_p,
                                  C.POINTER(TrxDebug)]
    lib.trx_run_bands.restype = C.c_int
    lib.trx_batch_set_bands.argtypes = [C.c_void_p, C.c_int32, C.POINTER(TrxBand)]
    lib.trx_batch_set_bands.restype = C.c_int
    lib.trx_run_batch_bands.argtypes = [C.c_void_p, C.c_int32, C.POINTER(TrxAtm), C.POINTER(TrxOpts),
                                        C.POINTER(c_double_p)]
    lib.trx_run_batch_bands.restype = C.c_int
    return lib


def bind_contrib_api(lib):
    """argtypes/restypes of the contribution-function entry points (trx_run_contrib, trx_run_batch_contrib)."""
    lib.trx_run_contrib.argtypes = [C.c_void_p, C.POINTER(TrxAtm), C.POINTER(TrxOpts), c_double_p, c_double_p,
                                    c_double_p, C.POINTER(TrxDebug)]
    lib.trx_run_contrib.restype = C.c_int
    lib.trx_run_batch_contrib.argtypes = [C.c_void_p, C.c_int32, C.POINTER(TrxAtm), C.POINTER(TrxOpts),
                                          C.POINTER(c_double_p), C.POINTER(c_double_p)]
    lib.trx_run_batch_contrib.restype = C.c_int
    return lib


def bind_pixels_api(lib):
    """argtypes/restypes of the detector-pixel entry points (trx_set_pixels, trx_run_pixels and their batch forms)."""
    lib.trx_set_pixels.argtypes = [C.c_void_p, C.POINTER(TrxPixels)]
    lib.trx_set_pixels.restype = C.c_int
    lib.trx_run_pixels.argtypes = [C.c_void_p, C.POINTER(TrxAtm), C.POINTER(TrxOpts), c_double_p, C.c_int32, c_double_p,
                                   c_double_p, C.POINTER(TrxDebug)]
    lib.trx_run_pixels.restype = C.c_int
    lib.trx_batch_set_pixels.argtypes = [C.c_void_p, C.POINTER(TrxPixels)]
    lib.trx_batch_set_pixels.restype = C.c_int
    lib.trx_run_batch_pixels.argtypes = [C.c_void_p, C.c_int32, C.POINTER(TrxAtm), C.POINTER(TrxOpts), C.c_int32,
                                         C.POINTER(c_double_p), C.POINTER(c_double_p)]
    lib.trx_run_batch_pixels.restype = C.c_int
    return lib


def bind_moments_api(lib):
    """argtypes/restypes of the moment entry points (trx_set_observed, trx_run_moments and their batch forms)."""
    lib.trx_set_observed.argtypes = [C.c_void_p, C.POINTER(TrxObserved)]
    lib.trx_set_observed.restype = C.c_int
    lib.trx_run_moments.argtypes = [C.c_void_p, C.POINTER(TrxAtm), C.POINTER(TrxOpts), c_double_p, C.c_int32, c_double_p,
                                    c_double_p, C.POINTER(TrxDebug)]
    lib.trx_run_moments.restype = C.c_int
    lib.trx_batch_set_observed.argtypes = [C.c_void_p, C.POINTER(TrxObserved)]
    lib.trx_batch_set_observed.restype = C.c_int
    lib.trx_run_batch_moments.argtypes = [C.c_void_p, C.c_int32, C.POINTER(TrxAtm), C.POINTER(TrxOpts), C.c_int32,
                                          C.POINTER(c_double_p), C.POINTER(c_double_p)]
    lib.trx_run_batch_moments.restype = C.c_int
    return lib


def bind_trail_api(lib):
    """argtypes/restypes of the trail entry points (trx_run_trail and its batch form)."""
    lib.trx_run_trail.argtypes = [C.c_void_p, C.POINTER(TrxAtm), C.POINTER(TrxOpts), c_double_p, C.c_int32, c_double_p,
                                  c_double_p, C.POINTER(TrxDebug)]
    lib.trx_run_trail.restype = C.c_int
    lib.trx_run_batch_trail.argtypes = [C.c_void_p, C.c_int32, C.POINTER(TrxAtm), C.POINTER(TrxOpts), C.c_int32,
                                        C.POINTER(c_double_p), C.POINTER(c_double_p)]
    lib.trx_run_batch_trail.restype = C.c_int
    return lib


def bind_vmap_api(lib):
    """argtypes/restypes of the detection-map entry points (trx_run_velocity_map and its batch form)."""
    lib.trx_run_velocity_map.argtypes = [C.c_void_p, C.POINTER(TrxAtm), C.POINTER(TrxOpts), c_double_p, C.POINTER(TrxVmap),
                                         c_double_p, c_double_p, C.POINTER(TrxDebug)]
    lib.trx_run_velocity_map.restype = C.c_int
    lib.trx_run_batch_velocity_map.argtypes = [C.c_void_p, C.c_int32, C.POINTER(TrxAtm), C.POINTER(TrxOpts), C.POINTER(TrxVmap),
                                               C.POINTER(c_double_p), C.POINTER(c_double_p)]
    lib.trx_run_batch_velocity_map.restype = C.c_int
    return lib


CELLMAP_CHUNK = 64      # kCellMapChunk (csrc/hip/trx_device.h): the most cells of a filtered map that go through the device at once


def bind_cellmap_api(lib):
    """argtypes/restypes of the filtered-map entry points (trx_run_filtered_map and its batch form)."""
    lib.trx_run_filtered_map.argtypes = [C.c_void_p, C.POINTER(TrxAtm), C.POINTER(TrxOpts), c_double_p, C.POINTER(TrxVmap),
                                         c_double_p, c_int32_p, C.POINTER(TrxDebug)]
    lib.trx_run_filtered_map.restype = C.c_int
    lib.trx_run_batch_filtered_map.argtypes = [C.c_void_p, C.c_int32, C.POINTER(TrxAtm), C.POINTER(TrxOpts), C.POINTER(TrxVmap),
                                               C.POINTER(c_double_p)]
    lib.trx_run_batch_filtered_map.restype = C.c_int
    return lib


EXPOSED_MAP_PAIR_BYTES = 1 << 33      # kExposedMapPairBytes (csrc/hip/trx_device.h): the most bytes of pixel pairs [R][npix][2] an exposed map makes


def bind_expmap_api(lib):
    """argtypes/restypes of the exposed-map entry points (trx_run_exposed_map and its batch form)."""
    lib.trx_run_exposed_map.argtypes = [C.c_void_p, C.POINTER(TrxAtm), C.POINTER(TrxOpts), c_double_p, C.POINTER(TrxVmap),
                                        c_double_p, c_int32_p, C.POINTER(C.c_int64), C.POINTER(TrxDebug)]
    lib.trx_run_exposed_map.restype = C.c_int
    lib.trx_run_batch_exposed_map.argtypes = [C.c_void_p, C.c_int32, C.POINTER(TrxAtm), C.POINTER(TrxOpts), C.POINTER(TrxVmap),
                                              C.POINTER(c_double_p)]
    lib.trx_run_batch_exposed_map.restype = C.c_int
    return lib


def bind_filter_api(lib):
    """argtypes/restypes of the filter entry points (trx_set_filter, trx_run_filtered_moments and their batch forms)."""
    lib.trx_set_filter.argtypes = [C.c_void_p, C.POINTER(TrxFilter)]
    lib.trx_set_filter.restype = C.c_int
    lib.trx_run_filtered_moments.argtypes = [C.c_void_p, C.POINTER(TrxAtm), C.POINTER(TrxOpts), c_double_p, C.c_int32,
                                             c_double_p, c_double_p, c_double_p, C.POINTER(TrxDebug)]
    lib.trx_run_filtered_moments.restype = C.c_int
    lib.trx_batch_set_filter.argtypes = [C.c_void_p, C.POINTER(TrxFilter)]
    lib.trx_batch_set_filter.restype = C.c_int
    lib.trx_set_weighted_filter.argtypes = [C.c_void_p, C.POINTER(TrxWfilter), C.POINTER(C.c_int64)]
    lib.trx_set_weighted_filter.restype = C.c_int
    lib.trx_batch_set_weighted_filter.argtypes = [C.c_void_p, C.POINTER(TrxWfilter)]
    lib.trx_batch_set_weighted_filter.restype = C.c_int
    lib.trx_run_batch_filtered_moments.argtypes = [C.c_void_p, C.c_int32, C.POINTER(TrxAtm), C.POINTER(TrxOpts), C.c_int32,
                                                   C.POINTER(c_double_p), C.POINTER(c_double_p)]
    lib.trx_run_batch_filtered_moments.restype = C.c_int
    return lib


def bind_highpass_api(lib):
    """argtypes/restypes of the high-pass entry points (trx_set_highpass, trx_run_highpassed, trx_batch_set_highpass)."""
    lib.trx_set_highpass.argtypes = [C.c_void_p, C.POINTER(TrxHighpass)]
    lib.trx_set_highpass.restype = C.c_int
    lib.trx_run_highpassed.argtypes = [C.c_void_p, C.POINTER(TrxAtm), C.POINTER(TrxOpts), c_double_p, C.c_int32,
                                       c_double_p, c_double_p, C.POINTER(TrxDebug)]
    lib.trx_run_highpassed.restype = C.c_int
    lib.trx_batch_set_highpass.argtypes = [C.c_void_p, C.POINTER(TrxHighpass)]
    lib.trx_batch_set_highpass.restype = C.c_int
    return lib


def bind_broaden_api(lib):
    """argtypes/restypes of the broadening entry points (trx_set_broadening, trx_run_broadened and their batch forms)."""
    lib.trx_set_broadening.argtypes = [C.c_void_p, C.POINTER(TrxBroadening)]
    lib.trx_set_broadening.restype = C.c_int
    lib.trx_run_broadened.argtypes = [C.c_void_p, C.POINTER(TrxAtm), C.POINTER(TrxOpts), c_double_p, c_double_p,
                                      C.POINTER(TrxDebug)]
    lib.trx_run_broadened.restype = C.c_int
    lib.trx_batch_set_broadening.argtypes = [C.c_void_p, C.c_int32, C.POINTER(TrxBroadening)]
    lib.trx_batch_set_broadening.restype = C.c_int
    lib.trx_run_batch_broadened.argtypes = [C.c_void_p, C.c_int32, C.POINTER(TrxAtm), C.POINTER(TrxOpts),
                                            C.POINTER(c_double_p)]
    lib.trx_run_batch_broadened.restype = C.c_int
    return lib


def bind_exposures_api(lib):
    """argtypes/restypes of the exposure-table entry points (trx_set_exposures, trx_run_exposed and their batch forms)."""
    lib.trx_set_exposures.argtypes = [C.c_void_p, C.POINTER(TrxExposures)]
    lib.trx_set_exposures.restype = C.c_int
    lib.trx_run_exposed.argtypes = [C.c_void_p, C.POINTER(TrxAtm), C.POINTER(TrxOpts), c_double_p, C.c_int32, c_double_p,
                                    c_double_p, C.POINTER(TrxDebug)]
    lib.trx_run_exposed.restype = C.c_int
    lib.trx_batch_set_exposures.argtypes = [C.c_void_p, C.c_int32, C.POINTER(TrxExposures)]
    lib.trx_batch_set_exposures.restype = C.c_int
    lib.trx_run_batch_exposed.argtypes = [C.c_void_p, C.c_int32, C.POINTER(TrxAtm), C.POINTER(TrxOpts), C.c_int32,
                                          C.POINTER(c_double_p), C.POINTER(c_double_p)]
    lib.trx_run_batch_exposed.restype = C.c_int
    return lib


def bind_sysrem_api(lib):
    """argtypes/restypes of the detrending entry point (trx_detrend_observed)."""
    lib.trx_detrend_observed.argtypes = [C.c_void_p, C.POINTER(TrxAtm), C.POINTER(TrxOpts), c_double_p, C.c_int32, c_double_p,
                                         C.POINTER(TrxDetrend), c_double_p, c_double_p, c_double_p, C.POINTER(C.c_int64),
                                         C.POINTER(TrxDebug)]
    lib.trx_detrend_observed.restype = C.c_int
    return lib


def bind_pca_api(lib):
    """argtypes/restypes of the principal-component entry point (trx_pca_observed)."""
    i64p = C.POINTER(C.c_int64)
    lib.trx_pca_observed.argtypes = [C.c_void_p, C.POINTER(TrxAtm), C.POINTER(TrxOpts), c_double_p, C.c_int32, c_double_p,
                                     C.POINTER(TrxPca), c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, i64p, i64p,
                                     C.POINTER(TrxDebug)]
    lib.trx_pca_observed.restype = C.c_int
    return lib


def bind_regress_api(lib):
    """argtypes/restypes of the regression entry point (trx_regress_observed)."""
    i64p = C.POINTER(C.c_int64)
    lib.trx_regress_observed.argtypes = [C.c_void_p, C.POINTER(TrxAtm), C.POINTER(TrxOpts), c_double_p, C.c_int32, c_double_p,
                                         C.POINTER(TrxRegress), c_double_p, c_double_p, c_double_p, i64p, i64p, C.POINTER(TrxDebug)]
    lib.trx_regress_observed.restype = C.c_int
    return lib


def bind_scatter_api(lib):
    """argtypes/restypes of the column-scatter entry point (trx_weigh_observed)."""
    lib.trx_weigh_observed.argtypes = [C.c_void_p, C.POINTER(TrxScatter), c_double_p, c_double_p, c_double_p,
                                       C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.trx_weigh_observed.restype = C.c_int
    return lib


def bind_hpdata_api(lib):
    """argtypes/restypes of the observed set's own high-pass (trx_highpass_observed)."""
    lib.trx_highpass_observed.argtypes = [C.c_void_p, C.c_int32, c_double_p, C.POINTER(C.c_int64)]
    lib.trx_highpass_observed.restype = C.c_int
    return lib


def bind_normalise_api(lib):
    """argtypes/restypes of the normalisation entry points (trx_set_normalise, trx_normalise_observed)."""
    i64p = C.POINTER(C.c_int64)
    lib.trx_set_normalise.argtypes = [C.c_void_p, C.POINTER(TrxNormalise)]
    lib.trx_set_normalise.restype = C.c_int
    lib.trx_normalise_observed.argtypes = [C.c_void_p, C.POINTER(TrxAtm), C.POINTER(TrxOpts), c_double_p, C.c_int32, c_double_p,
                                           C.c_int32, C.c_double, C.c_double, c_double_p, c_double_p, c_double_p, i64p, i64p,
                                           C.POINTER(TrxDebug)]
    lib.trx_normalise_observed.restype = C.c_int
    return lib
