"""High-passing the observed set itself without a device: xcor.highpass_observed_reference, the numpy mirror of
trx_highpass_observed, held bit for bit against the composition of the model's own xcor.highpass_reference over the pairs
(data, W > 0); the staging rule and the window walk of transit_amd/csrc/trx_highpass.h and the checks, extents, launch guard
and data levels of transit_amd/csrc/trx_hpdata.h through tests/hpdata_check.cpp, a stand-alone program over exact-size heap
arrays under -fsanitize=address,undefined that walks a whole set the way k_data_highpass does and holds every value against
the literal definition; the preconditions of the shared sets; and the ABI: the exported symbol and the kernel in the code
object."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from bits import same_bits
from host_check import build_check

import hpdata_cases as hc
import many_cases as mc
import scatter_cases as cs
import sysrem_cases as sc
from transit_amd import _abi, build, xcor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = [(nexp, weighted, stage, seg) for nexp in (7, 12) for weighted in (False, True) for stage in hc.STAGES for seg in hc.SEGS]


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return build_check("hpdata_check", tmp_path_factory.mktemp("hpdata_check"))


def test_staging_refusals_extents_guard_and_data_levels_under_sanitizers(check_exe):
    out = subprocess.run([check_exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert out.stderr == ""                              # (no sanitizer report)
    lines = out.stdout.splitlines()
    last = lines[-1].split()
    assert last[0] == "ok" and int(last[1]) >= 72, lines[-20:]
    assert not [line for line in lines if line.startswith("FAILED")]


def mirror_is_the_composition(d, w, seg, hp, what):
    """the mirror of one set under one table against the composition, bit for bit, and what follows from the definition;
    returns (the mirror's data, the live entries alone in their window)"""
    dead = np.zeros(d.shape, dtype=bool) if w is None else ~(w > 0)
    got, ndead = xcor.highpass_observed_reference(d, w, seg, hp)
    assert same_bits(got, hc.composition(d, w, seg, hp)), what
    assert ndead == np.count_nonzero(dead) and (ndead > 0) == (w is not None), what
    assert np.isfinite(got).all(), what
    # a dead entry is +0; a live entry alone in its window is r - (t0 r) / t0 -- +0 wherever that quotient is exact --; every
    # other live entry is not zero
    assert np.all(got[dead] == 0) and not np.signbit(got[dead]).any(), what
    lone = hc.alone(w, seg, hp, d.shape)
    assert not (lone & dead).any(), what
    assert same_bits(got[lone], d[lone] - (hp.taps[0] * d[lone]) / hp.taps[0]), what
    assert np.all(got[~dead & ~lone] != 0), what
    if hp.taps[0] == 1.0:
        assert np.array_equal(got == 0, dead | lone), what
    return got, lone


_LONG = {}


def long_data(weighted, stage):
    """(set, data the high-pass reads, weights or None) of many_cases.long_set: raw, or after xcor.sysrem_reference(.., 3, 2)"""
    ms = mc.long_set()[0]
    w = ms.weight if weighted else None
    if stage == "detrended" and weighted not in _LONG:
        _LONG[weighted] = xcor.sysrem_reference(ms.data, w, ms.seg_first, 3, 2)[2]
    return ms, (_LONG[weighted] if stage == "detrended" else ms.data), w


@pytest.mark.parametrize("stage", hc.STAGES)
@pytest.mark.parametrize("weighted", [False, True])
def test_the_mirror_is_the_composition_on_the_long_orders(weighted, stage):
    """segments of 1024, 1025 and 2049 pixels: two whole tiles of kHpTile; two and a tile of ONE pixel, whose window is all
    halo; four and a tile of one pixel"""
    ms, d, w = long_data(weighted, stage)
    for half in mc.LONG_HALVES:
        for name, hp in hc.tables(half).items():
            mirror_is_the_composition(d, w, ms.seg_first, hp, "long orders, %s, %s, half %d, %s" % ("edge weights" if weighted else "no weights", stage, half, name))


@pytest.mark.parametrize("nexp,weighted,stage,seg_name", SETS)
def test_the_mirror_is_the_composition_bit_for_bit(nexp, weighted, stage, seg_name):
    d, w = hc.the_data(nexp, weighted, stage, seg_name)
    seg = hc.SEGS[seg_name]
    dead = np.zeros(d.shape, dtype=bool) if w is None else ~(w > 0)
    one = slice(int(seg[0]), int(seg[1]))
    assert seg[1] - seg[0] == 1
    for half in hc.HALVES:
        for name, hp in hc.tables(half).items():
            what = "%d exposures, %s, %s, %s, half %d, %s" % (nexp, "edge weights" if weighted else "no weights", stage, seg_name, half, name)
            got, lone = mirror_is_the_composition(d, w, seg, hp, what)
            # The one-pixel segment's live entries are alone at every half.
            assert lone[:, one][~dead[:, one]].all(), what
            if hp.taps[0] == 1.0:
                if not weighted and half >= 1:
                    only = np.zeros(d.shape, dtype=bool)
                    only[:, one] = True
                    assert np.array_equal(got == 0, only), what      # (the zeros: exactly the one-pixel segment)


@pytest.mark.parametrize("nexp", [7, 12])
def test_twice_is_not_once_on_the_host(nexp):
    """why the device keeps the pre-high-pass data aside: the mirror applied to its own result differs nearly everywhere"""
    d, w = hc.the_data(nexp, True, "raw", "orders")
    hp = hc.tables(70)["gauss"]
    once = xcor.highpass_observed_reference(d, w, cs.SEG, hp)[0]
    twice = xcor.highpass_observed_reference(once, w, cs.SEG, hp)[0]
    differ = int(np.count_nonzero(once.view(np.int64) != twice.view(np.int64)))
    print("%d exposures: twice differs from once in %d of %d entries" % (nexp, differ, once.size))
    assert differ > 0.9 * np.count_nonzero(w > 0)


@pytest.mark.parametrize("nexp", [7, 12])
def test_the_preconditions_of_the_sets(nexp):
    d, w = hc.the_data(nexp, True, "raw", "orders")
    a, b = int(cs.SEG[sc.MASKED_SEG]), int(cs.SEG[sc.MASKED_SEG + 1])
    assert b - a == 65 and np.all(w[sc.MASKED_EXP, a:b] == 0)             # a row masked over a whole segment
    assert np.all(w[:, sc.MASKED_COL] == 0)                               # a column masked everywhere
    assert np.count_nonzero(w[:, a:b] > 0) > 0 and np.count_nonzero(w > 0) > 0.9 * w.size
    # the second segmentation: the same 800 pixels, one segment over two tiles of kHpTile with a ragged second one
    long = hc.SEGS["long"]
    assert list(np.diff(long)) == [1, 63, 0, 736] and long[-1] == cs.NPIX == 800
    assert long[3] + hc.TILE == hc.BORDER == 576 and 0 < long[4] - hc.BORDER < hc.TILE
    # a masked entry within NEAR pixels of the tile border on either side: a tile's halo crosses it at every half >= NEAR
    dead = np.argwhere(w <= 0)
    below = [int(q) for v, q in dead if hc.BORDER - hc.NEAR <= q < hc.BORDER and q != sc.MASKED_COL]
    above = [int(q) for v, q in dead if hc.BORDER <= q < hc.BORDER + hc.NEAR + 1 and q != sc.MASKED_COL]
    print("%d exposures: masked entries at pixels %s below and %s above the tile border %d" % (nexp, below, above, hc.BORDER))
    assert below and above and hc.NEAR in hc.HALVES
    # in the first segmentation the masked row's segment and the masked column lie in different segments
    assert not a <= sc.MASKED_COL < b


def walk_is_the_mirror(check_exe, tmp_path, d, w, seg, half, name):
    """the program's walk of one set under one table against the mirror, bit for bit"""
    nexp, npix, weighted = d.shape[0], d.shape[1], w is not None
    hp = hc.tables(half)[name]
    src, dst = tmp_path / ("in%d.bin" % half), tmp_path / ("out%d.bin" % half)
    with open(src, "wb") as f:
        f.write(np.array([nexp, npix, len(seg) - 1, half, int(weighted)], dtype=np.int64).tobytes())
        f.write(np.asarray(seg, dtype=np.int64).tobytes())
        f.write(hp.taps.tobytes())
        if weighted:
            f.write(np.ascontiguousarray(w).tobytes())
        f.write(np.ascontiguousarray(d).tobytes())
    out = subprocess.run([check_exe, "values", str(src), str(dst)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout[-2000:] + out.stderr[-4000:]
    assert "FAILED" not in out.stdout and " 0 differ from the literal definition" in out.stdout
    lines = {x[0]: x[1:] for x in (line.split() for line in out.stdout.splitlines())}
    want, ndead = xcor.highpass_observed_reference(d, w, seg, hp)
    got = np.fromfile(dst, dtype=np.float64).reshape(want.shape)
    assert same_bits(got, want), (half, name)
    assert int(lines["ndead"][0]) == ndead
    waves, full = int(lines["waves"][0]), int(lines["waves"][2])      # ("waves N full M")
    assert 0 <= full <= waves and (weighted or half == 0 or full < waves)      # (a window over a segment's edge is never full)
    if half == 0 and not weighted:
        assert full == waves


@pytest.mark.parametrize("nexp,weighted,stage,seg_name", SETS)
def test_the_programs_walk_is_the_mirror_bit_for_bit(check_exe, tmp_path, nexp, weighted, stage, seg_name):
    """every half; the three tables in turn, so that every table meets every half over the sets"""
    d, w = hc.the_data(nexp, weighted, stage, seg_name)
    seg = hc.SEGS[seg_name]
    turn = SETS.index((nexp, weighted, stage, seg_name))
    for i, half in enumerate(hc.HALVES):
        name = ("boxcar", "gauss", "random")[(turn + i) % 3]
        walk_is_the_mirror(check_exe, tmp_path, d, w, seg, half, name)


@pytest.mark.parametrize("stage", hc.STAGES)
@pytest.mark.parametrize("weighted", [False, True])
def test_the_programs_walk_on_the_long_orders(check_exe, tmp_path, weighted, stage):
    """k_data_highpass' own walk on the CPU over the long set: the tiles of one pixel of the 1025- and the 2049-pixel segment,
    and a half of 600 > kHpTile over three and five tiles"""
    ms, d, w = long_data(weighted, stage)
    for half in mc.LONG_HALVES:
        for name in hc.tables(half):
            walk_is_the_mirror(check_exe, tmp_path, d, w, ms.seg_first, half, name)


def test_the_mirror_refuses_what_it_does_not_define():
    hp = xcor.boxcar_highpass(3)
    with pytest.raises(ValueError):
        xcor.highpass_observed_reference(np.zeros(5), None, [0, 5], hp)
    with pytest.raises(ValueError):
        xcor.highpass_observed_reference(np.zeros((3, 5)), np.ones((3, 4)), [0, 5], hp)


def test_abi_symbol_and_kernel():
    txt = open(os.path.join(ROOT, "include", "transit_hip.h")).read()
    assert "int  trx_highpass_observed(trx_handle *h, int32_t apply" in txt and "#define TRX_ABI_VERSION 5" in txt
    path = build.lib_path("libtransit_hip.so")
    if not os.path.exists(path):
        build.build_hip()
    lib = ctypes.CDLL(path)
    assert hasattr(lib, "trx_highpass_observed")
    lib.trx_abi_version.restype = ctypes.c_int
    assert lib.trx_abi_version() == 5
    blob = open(path, "rb").read()
    assert b"k_data_highpass" in blob and b"k_pixel_highpass" in blob
    # refused without a handle, before anything is touched
    _abi.bind(lib, _abi.HIP_HEADER, "trx_")
    assert lib.trx_highpass_observed(None, 1, None, None) == -1
