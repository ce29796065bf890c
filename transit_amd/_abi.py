"""ctypes mirror of include/transit_hip.h (plain C structs, no torch types)."""
from __future__ import annotations

import ctypes as C
import os
import re

from .build import ROOT

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


CELLMAP_CHUNK = 64      # kCellMapChunk (csrc/hip/trx_device.h): the most cells of a filtered map that go through the device at once
EXPOSED_MAP_PAIR_BYTES = 1 << 33      # kExposedMapPairBytes (csrc/hip/trx_device.h): the most bytes of pixel pairs [R][npix][2] an exposed map makes


LOG_FN = C.CFUNCTYPE(None, C.c_int, C.c_char_p, C.c_void_p)     # trx_log_fn

HIP_HEADER = os.path.join(ROOT, "include", "transit_hip.h")
HOST_HEADER = os.path.join(ROOT, "include", "transit_host.h")

# a C type as a header writes it -> its ctypes: `const` and the parameter's name dropped, no blank at a star
CTYPES = {
    "void": None, "int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "long": C.c_long, "double": C.c_double,
    "int*": C.POINTER(C.c_int), "int32_t*": c_int32_p, "int64_t*": c_int64_p, "float*": c_float_p, "double*": c_double_p,
    "uint8_t*": c_uint8_p, "unsigned char*": c_uint8_p, "char*": C.c_char_p, "void*": C.c_void_p,
    "int32_t**": C.POINTER(c_int32_p), "double**": C.POINTER(c_double_p), "char**": C.POINTER(C.c_char_p),
    "void**": C.POINTER(C.c_void_p), "trx_log_fn": LOG_FN,
}

_prototypes = {}


def _ctype(decl: str, named: bool, opaque, where: str):
    """the ctypes of one declared type: CTYPES, a handle the header only names (`T *`: c_void_p, `T **`: a pointer to one)
    or `trx_<name> *`, a pointer to the structure Trx<Name> of this module"""
    t = re.sub(r"\bconst\b", " ", decl).strip()
    if named and re.search(r"[\s*]\w+$", t):
        t = re.sub(r"\w+$", "", t)
    t = re.sub(r"\s*\*\s*", "*", re.sub(r"\s+", " ", t)).strip()
    if t in CTYPES:
        return CTYPES[t]
    base, stars = t.rstrip("*"), len(t) - len(t.rstrip("*"))
    if base in opaque and stars in (1, 2):
        return C.c_void_p if stars == 1 else C.POINTER(C.c_void_p)
    struct = globals().get("".join(w.capitalize() for w in base.split("_")))      # trx_opacity_grid: TrxOpacityGrid
    if base.startswith("trx_") and stars == 1 and isinstance(struct, type) and issubclass(struct, C.Structure):
        return C.POINTER(struct)
    raise ValueError("%s: no ctypes for the C type '%s'" % (where, " ".join(decl.split())))


def parse(text: str, prefix: str):
    """{name: (restype, argtypes)} of every `<ret> <prefix>name(args);` of a header's text"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    opaque = set(re.findall(r"\btypedef\s+struct\s+(\w+)\s+\1\s*;", text))
    out = {}
    for ret, name, args in re.findall(r"^[ \t]*([\w \t*]+?)\s*\b(%s\w+)\s*\(([^()]*)\)\s*;" % re.escape(prefix), text, flags=re.M):
        pars = [] if args.strip() in ("", "void") else args.split(",")
        out[name] = (_ctype(ret, False, opaque, name + ", the return type"),
                     [_ctype(p, True, opaque, "%s, argument %d" % (name, i + 1)) for i, p in enumerate(pars)])
    return out


def prototypes(header_path: str, prefix: str):
    """parse() of a header file, read once per path and prefix"""
    key = (header_path, prefix)
    if key not in _prototypes:
        with open(header_path) as f:
            _prototypes[key] = parse(f.read(), prefix)
    return _prototypes[key]


def bind(lib, header_path: str, prefix: str, exported: str = ""):
    """Set argtypes and restype, as the header declares them, on every `<prefix>name` of it that *lib* exports (as
    `<exported>name`, where the library has the same family under a prefix of its own).  The header is the one place a
    signature is written: a type this module cannot turn into ctypes raises ValueError."""
    for name, (restype, argtypes) in prototypes(header_path, prefix).items():
        fn = getattr(lib, exported + name[len(prefix):] if exported else name, None)
        if fn is not None:
            fn.argtypes, fn.restype = argtypes, restype
    return lib


def bind_engine_api(lib, prefix: str = "trx_"):
    """transit_hip.h's signatures on a library of the same ABI shape that exports them as <prefix>name and has no header
    of its own (CEngine serves any such library)."""
    return bind(lib, HIP_HEADER, "trx_", prefix)
