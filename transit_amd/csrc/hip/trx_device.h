// trx_device.h -- plain structs shared by the host API (trx_api.hip) and the
// kernels (trx_kernels.hip.h).  Everything here is laid out for HBM:
//   * SoA, 8/4/2/1-byte columns, no row pointers;
//   * per-layer arrays are [layer][x] with x contiguous so that consecutive
//     lanes (lines, groups or wavenumbers) read consecutive addresses.
#pragma once
#include <stdint.h>

#include "../trx_numerics.h"

namespace trx {

constexpr int kMaxChunk   = 32;    // layers swept per top-down step (upper bound)
constexpr int kMaxIso     = 256;   // isotopes per run (per-isotope tables of a block live in LDS)
constexpr int kMaxAngles  = 16;
constexpr int kMaxDop     = 256;   // Doppler-width samples (ndop)
constexpr int kTileBins   = 4;     // coarse bins per wavefront tile in the accumulate kernel
constexpr int kTabPad     = 512;   // zero floats in front of and behind the Voigt tables (>= bins per wide tile, trx_rows.hip.h's too)

// One distinct Voigt profile of the table (opacity.c:258-270, getprofile).
struct ProfileJob {
  int64_t off;        // first float of the profile in the table
  int32_t nv;         // points (odd)
  int32_t regime;     // 0 quick (point samples), 1 fine (edge mean), 2 coarse (Simpson mean)
  int32_t m;          // sub-intervals per bin (regime 2)
  int32_t pad;
  double  half;       // dwn * (nv/2)
  double  sub;        // spacing of the evaluation points
  double  alphaL, alphaD;
  int64_t first_bin;  // prefix sum of nv over jobs (global bin index of bin 0)
};

// Static line-list description (layer independent), device pointers.
struct LinesDev {
  int64_t nlines;
  const double  *wavn;     // [nlines] 1/(wl*1e-4), cm-1
  const double  *elow;     // [nlines]
  const double  *gf;       // [nlines]
  const int16_t *iso;      // [nlines]
  const uint8_t *inrange;  // [nlines] extinction.c:410
  const int32_t *lgroup;   // [nlines] group index when the line anchors a co-added group, else -1
  int64_t ngroups;
  const int32_t *gfirst;   // [ngroups] first line of the co-added group (extinction.c:449-462)
  const int32_t *gcount;   // [ngroups] members
  const int32_t *giown;    // [ngroups] fine-grid index of the anchor (extinction.c:445-447)
  const int16_t *giso;     // [ngroups]
  const double  *gwavn;    // [ngroups] anchor wavenumber
  // isotope blocks: groups of isotope b are [gblock[b], gblock[b+1]) sorted by descending iown
  const int32_t *gblock;   // [niso+1]
  // cnt_ge[b*(nwn+1) + k] = number of groups of block b with iown/osamp >= k
  const int32_t *cnt_ge;
};

// Per-run, per-layer scalars prepared on the host in the reference's own
// arithmetic (extinction.c:364-395) -- [layer][iso] unless noted.
struct LayerDev {
  const double *negc_over_t;  // [layer]  -EXPCTE/T
  const double *strength_f;   // SIGCTE*isoratio/(m*Z)          (extinction.c:464)
  const double *density;      // density of the isotope's molecule (extinction.c:473)
  const double *alphad;       // Doppler width / wavenumber
  const double *alphal;       // Lorentz width
  const int32_t *idop0;       // nearest aDop index for alphad*wn[0] (extinction.c:393)
  const int32_t *ilor;        // nearest aLor index              (extinction.c:394)
  const int32_t *psmax;       // largest profile half-size the isotope can use in this layer
};

// What k_group_sweep needs to find, per isotope block, the lines whose profiles can reach the
// shard in some layer of the step (one contiguous run per block: the TLI is wavelength-sorted):
// every workgroup builds the table of those runs in LDS itself (up to kMaxIso blocks), from
// psmax of the step's layers and cnt_ge -- a shard of the grid (windowed) or the whole grid.
// (The runs as a kernel argument for lists of few isotopes were measured: no difference.)
struct SweepWindow {
  int windowed, osamp;
  long long lo, hi, nwn;            // shard [lo, hi) of nwn coarse bins
};

// ---- the Voigt table's copies: what their layouts (../trx_table.h) share with the kernels ----
constexpr int kWalkMaxFrame = 16;    // bins of the widest frame (k_line_walk<16>)

// (trx_rows.hip.h)
constexpr int kRowSpan = 256;                 // cells between the first and the last group of a run, at most
constexpr int kRowMaxT = 512;                 // bins of the larger tile
constexpr int kRowTail = kRowMaxT + kRowSpan + 8;   // zero floats the table carries behind its last profile

// The walk's rows (trx_walk.hip.h): every row is a whole number of 64-byte lines, its K entries
// behind `front` zeros and in front of at least as many -- the bins of a frame are consecutive
// entries of ONE row, inside ONE or two cache lines, and what a narrow profile does not reach is
// zero by position.  Profiles of up to 8 entries per row: 4 zeros, the entries, zeros to 16 floats
// (a frame of 8 bins = one aligned 64-byte line); up to 16 entries: 8 zeros, the entries, zeros to
// 32 floats; wider ones (no frame reads them) the same with whole lines.
TRX_HD void walk_row_layout(int K, int &front, int &stride)
{
  if (K <= 8) { front = 4; stride = 16; }
  else if (K <= 16) { front = 8; stride = 32; }
  else { front = 8; stride = (K + 16 + 15) & ~15; }
}

// ---- how far a line range of the walk can reach (k_line_walk; checked on the host by tests/reach_check.cpp) ----
// A group whose anchor sits at fine-grid phase imod of its cell (0 <= imod < osamp) touches a bin only when a
// lane's profile half-size ps has imod <= ps (the cell's own bin) or osamp - imod <= ps (the bin above).  The
// step's bound psm_s (LayerDev::psmax, wave maximum) is the widest profile of the isotope's WHOLE wavenumber
// range; a range of 32-512 groups takes far narrower ones where widths are Doppler-dominated (width ~ wavenumber).
//
// Can a lane take the sticky profile somewhere in the range?  Only on an anchor below its wcut.  Anchors lie no
// lower than half a fine-grid step below their grid point (iown is the NEAREST point, trx_groups.h) and the
// range's lowest anchor is in cell1: the grid point one fine step below that cell's lower edge is below every
// anchor of the range.  (wn_i + k*odwn as group_lines forms it; a contraction to one rounding moves it by an
// ulp, against half a step of margin.)
TRX_HD bool walk_may_stick(double wn_i, double odwn, int osamp, int cell1, double wcut)
{
  return wn_i + ((double)cell1 * (double)osamp - 1.0) * odwn < wcut;
}

// One lane's bound: ps_first is the half-size at the Doppler index of the range's FIRST anchor -- wavenumbers
// descend along a range, the index only falls, and on a table with TablePlan::psize_mono no profile is wider
// than the one an index above it: every "own" profile of the range is at most ps_first.  The sticky profile
// (possibly the block's widest: deep, Lorentz-dominated layers) counts only where the lane can take it.
TRX_HD int walk_lane_reach(int ps_first, int ps_sticky, bool may_stick)
{
  const int st = may_stick ? ps_sticky : 0;
  return ps_first > st ? ps_first : st;
}

// The range's bound from the wave maximum of its valid lanes' bounds (idle lanes enter as 0): never above the
// step's, and the step's alone where the table is not monotone or the switch (TRX_RANGE_REACH=0) says so.
TRX_HD int walk_range_reach(int psm_s, int lanes_max, bool use_range)
{
  return use_range && lanes_max < psm_s ? lanes_max : psm_s;
}

// A group at phase imod is out of reach of every bin under bound `reach`: strictly inside the zone
// (reach, osamp - reach).  (reach >= osamp / 2: the zone is empty.)
TRX_HD bool walk_group_out_of_reach(int imod, int osamp, int reach)
{
  return imod > reach && imod < osamp - reach;
}

// The same test as the walk makes it per group: the slots of a frame of NB bins (slot k = bin cell - Rc + k,
// Rc = NB/2 - 1, at fine distance |(k - Rc)*osamp - imod|) within `reach` = psq*osamp + psr of the anchor.
// 0 exactly when walk_group_out_of_reach.
TRX_HD unsigned walk_cand_slots(int NB, int imod, int osamp, int reach, int psq, int psr)
{
  if (NB == 2) return (imod <= reach ? 1u : 0u) | (osamp - imod <= reach ? 2u : 0u);
  const int Rc = NB / 2 - 1;
  const int klo = Rc - psq + (imod > psr ? 1 : 0), khi = Rc + psq + (imod + psr >= osamp ? 1 : 0);
  return ((2u << khi) - 1u) & ~((1u << klo) - 1u);   // (0 <= klo, khi < NB by the choice of NB; klo = khi + 1: none)
}

// RangeInfo::pad: the smallest and the largest phase of a range's anchors, 16 bits each -- for ranges whose
// anchors share ONE cell, on grids with osamp < 65536.  Any other range gets kRangeNoExit: smallest phase 0,
// which is inside no zone (reach >= 0), so such a range is always walked.
constexpr int32_t kRangeNoExit = 0;
TRX_HD int32_t walk_range_phases(bool one_cell, int osamp, int imod_min, int imod_max)
{
  if (!one_cell || osamp >= 65536) return kRangeNoExit;
  return (int32_t)((uint32_t)imod_min | ((uint32_t)imod_max << 16));
}

// Every group of the range is out of reach (walk_group_out_of_reach for its extreme phases, hence for all):
// the range adds nothing to any bin and its records are zeros.
TRX_HD bool walk_range_out_of_reach(int32_t phases, int osamp, int reach)
{
  const int lo = (int)((uint32_t)phases & 0xffffu), hi = (int)((uint32_t)phases >> 16);
  return walk_group_out_of_reach(lo, osamp, reach) && walk_group_out_of_reach(hi, osamp, reach);
}

// The walk's copy of the Voigt table ("tabW", built by trx_create): per profile `osamp` rows, row
// `ph` holding the entries q = osamp*kk + ph, kk = 0..K-1, between zeros (walk_row_layout:
// rows are whole 64-byte lines).  The bins of a frame sit a whole cell apart: they are
// CONSECUTIVE entries of one row, one or two wide loads per lane instead of a load per bin, inside
// one cache line for frames of up to 8 bins, and where a profile does not reach the entries are
// zero by position (kTabPad zeros around the whole).
struct alignas(16) WalkProfile {
  uint32_t centre4;                  // byte offset of (row 0, kk = ps / osamp)
  int32_t rowb;                      // bytes per row (walk_row_layout)
  int32_t psr;                       // ps % osamp
  int32_t ps;                        // half-width in table samples
};

// ---- the run products: what their host layouts (../trx_products.h) share with the kernels ----
// (trx_bands.hip.h)
constexpr int kBandLaneBins = 16;                     // bins per lane of a piece
constexpr int kBandPiece = 64 * kBandLaneBins;        // bins per piece

// one band as a shard sees it (trx_set_bands builds it on the host)
struct BandDev {
  int32_t kind, pad;        // TRX_BAND_WEIGHTS / TRX_BAND_GAUSS
  int64_t s;                // first in-shard bin, local to the shard
  int64_t woff;             // WEIGHTS: index of that bin's weight in BandArgs::w
  int64_t piece0, npieces;  // its pieces: piece0 .. piece0 + npieces - 1 (none: no bin in the shard)
  double centre, sigma;     // GAUSS: cm-1
};
struct BandPiece {
  int64_t start;            // local bin of the piece's first bin
  int32_t band, len;        // 1 <= len <= kBandPiece
};

// (trx_contrib.hip.h)
constexpr int kContribWaves = 4;                                  // waves per block: one bin per lane
constexpr int kContribSplit = kBandPiece / (64 * kContribWaves);  // sub-pieces (blocks) per piece

// (trx_pixels.hip.h)
constexpr int kPixBlock = 256;                        // lanes (pairs) per block: whole waves

// (trx_filter.hip.h)
struct FilterTile { int64_t first; int32_t seg, count; };      // pixels [first, first + count) of segment seg, 1 <= count <= 64

// (trx_highpass.hip.h)
constexpr int kHpBlock = 256;                         // lanes per block: whole waves
constexpr int kHpOuts = 2;                            // outputs a lane keeps in registers: pixels lane, lane + kHpBlock of the tile
constexpr int kHpTile = kHpBlock * kHpOuts;           // pixels per tile
// pixels [first, first + count) of the segment [seg_first, seg_last), 1 <= count <= kHpTile
struct HpTile { int64_t first, seg_first, seg_last; int32_t count, pad; };

// (trx_cellmap.hip.h) a filtered map goes through its cells in chunks: at most kCellMapChunk cells, and fewer where the
// chunk's filtered values [chunk][nexp][npix] would be above kCellMapValBytes -- never fewer than one
constexpr int kCellMapChunk = 64;
constexpr uint64_t kCellMapValBytes = (uint64_t)1 << 30;
constexpr int kCellTrackBlock = 256;                  // lanes ((cell, exposure) pairs) per block of k_cell_tracks

// (trx_expmap.hip.h) an exposed map's pixel rows are (lag, exposure) pairs: their pairs [R][npix][2] may take
// kExposedMapPairBytes at the most -- a design limit, not a measurement: with a high-pass a second buffer of that size
// stands beside the first, and the two stay under 16 GiB of the card's memory
constexpr uint64_t kExposedMapPairBytes = (uint64_t)1 << 33;
constexpr int kCellSpanWaves = 4;                     // exposures (waves) per block of k_cell_spans

}  // namespace trx
