// mifc_vortdiv_plan.h -- which kernel form a wind-family launch takes (relvort, divergence, the fused pair, absvort, the
// Jacobian, the fused pair with the wind speed), in which shape and on which grid: a pure host function of the request
// and the MIFC_* snapshot.  Plain C++, no HIP header: tests/test_vortdiv_plan_cpu.py compiles it with the host compiler.
// launch_vortdiv_rows (mifc_vortdiv.hip) asks plan_wind() and then only fills the kernel arguments and dispatches.
#ifndef MIFC_VORTDIV_PLAN_H
#define MIFC_VORTDIV_PLAN_H

#include <cstdlib>
#include <cstring>

#include "mifc_env.h"
#include "mifc_stencil_limits.h"

namespace mifc {

enum class WindOp { Relvort, Divergence, Vortdiv, Absvort, Jacobian };

// what the choice depends on, and nothing else
struct WindRequest
{
  WindOp op;
  int nx, ny_global, j0, ny_local, nlev;
  int row_begin, row_end; // a caller-chosen range of owned rows (row_end <= row_begin: all)
  bool rv, dv, ff, fc;    // outputs asked for (vorticity or the Jacobian, divergence, wind speed); a Coriolis field was passed
  bool ragged;            // some row does not start at a 16-byte boundary (width, bases or level strides)
  bool every_level_all_defined;
  bool undef_is_nan;
  bool has_partials; // a buffer for per-workgroup counts and the counters they are added to
  long partials_cap; // its entries
};

// Rows: waves walk bands of rows, WPB levels side by side.  Oneshot: a wave per 4 rows x 256 columns, no loop.
// OneshotTiles: the same with the rows of a tile shared through LDS.  LevelWalk: tiles that stay put and walk the levels,
// every wave loads and stores.  Split: the same tiles with loader waves and compute waves.
enum class WindForm { None, Rows, Oneshot, OneshotTiles, LevelWalk, Split };

// The shape of each form.  Defaults here; MIFC_VORTDIV_TUNE overrides them (wind_shape() below).
struct WindShape
{
  WindForm form = WindForm::Rows; // the form asked for (K); plan_wind() may decline it or run another
  // row-walking kernel.  XCD is read by every form, NT by the one-shot form, NTI by the level-walking one.
  int R = 8;      // rows per band
  int V = 2;      // float4 per lane and row (1, 2 or 3): a wave covers 256 * V columns
  int D = 1;      // rows kept in flight beyond the 3-row window (0 or 1)
  int NT = 1;     // nontemporal stores
  int WPB = 8;    // waves per workgroup (1, 2, 4 or 8): that many levels side by side
  int ORDER = 1;  // block order, see decode_block()
  int XCD = 1;    // XCD-aware blockIdx remap
  int ZZ = 1;     // odd bands walk upwards (halo rows meet in L2)
  int NTI = 0;    // nontemporal loads for the rows that no other band (level-walking: no other wave) reads
  int LDSX = 0;   // extra KiB of LDS requested per workgroup: limits the workgroups resident on a CU (occupancy experiments)
  struct
  {
    int tile_rows = 8; // 8 (10-wave workgroups) or 14 (16 waves; the fused pair only)
  } tiles;
  struct
  {
    int waves = 16;     // per workgroup: 8, 12 or 16
    int halo_waves = 1; // two of them only fetch the halo rows: the tile is waves - 2 rows high
    int prefetch = 2;   // levels in flight ahead of the one computed: 1 or 2
  } levelwalk;
  struct
  {
    int tile_rows = 10; // compute waves: 6, 8, 10, 12 or 14
    int loaders = 0;    // loader waves: 2 or 4; 0: 4 for 10-row tiles, 2 otherwise
    int prefetch = 2;   // levels the loaders run ahead: 1, 2 or 3
  } split;
  int lgroup = 0; // one-shot forms: level-minor unit order in groups of this many levels (0: address order);
                  // level-walking forms: levels per workgroup (0: all)
  // measurement build only (libmifc_measure.so): knobs that make the kernel compute something else
  int XH = 0, XS = 0, XL = 0, STA = 0; // no halo rows | (practically) no stores | no field loads | buffer stores with this cache policy
  int PADROWS = 0;                     // the last PADROWS rows of every level are padding (changes the level stride)
};

struct WindPlan : WindShape // form: the one that runs; the shape fields of that form are what the dispatch instantiates
{
  const char* note = ""; // what mifc_last_stencil_form() reports
  // RowsParams, see mifc_vortdiv.hip
  int nyg = 0, ny_local = 0;
  int lo = 0, hi = 0;
  long idx_lo = 0, idx_hi = 0;
  int nbands = 0, nwc = 0;
  int uL = 0, uB = 0, uW = 0, n_logical = 0, per_xcd = 0;
  // the launch
  int grid = 0, block = 0;
  long lds = 0;                    // dynamic LDS bytes
  bool counts_by_partials = false; // the workgroups leave their counts in the partials buffer; launch_count_partials_levels follows
};

inline int tune_value(const char* s, const char* key, int dflt)
{
  // finds "KEY=" at the start of the string or after a comma
  const size_t n = std::strlen(key);
  for (const char* p = s; p && *p;) {
    if (std::strncmp(p, key, n) == 0 && p[n] == '=')
      return std::atoi(p + n + 1);
    p = std::strchr(p, ',');
    if (p)
      ++p;
  }
  return dflt;
}

// MIFC_VORTDIV_TUNE="K=3,RB=12,D=0,LG=6" (the sweep tools and the tests) onto the named fields.  The string's keys are
// the row-walking kernel's; for the other forms some of them stand for something else:
//
//   key   K=0 rows          K=1 one-shot   K=2 tiles      K=3 level-walking        K=4 split roles
//   R     rows per band     -              -              -                        -
//   V     float4 per lane   -              -              -                        -
//   D     rows in flight    -              -              prefetch: 0 -> 1, 1 -> 2  prefetch: 0 -> 1, 1 -> 2
//   NT    nt stores         nt stores      -              -                        -
//   WPB   waves per wg      -              -              -                        loader waves (2 or 4)
//   ZZ    zigzag bands      -              -              halo waves               -
//   RB    -                 -              tile rows      waves per workgroup      tile rows
//   LG    -                 level group    level group    levels per workgroup     levels per workgroup
//   ORDER block order       -              -              -                        -
//   LDSX  extra LDS KiB     -              -              -                        -
//   NTI   nt loads          -              -              nt loads (halo waves)    -
//   XCD   every form: the XCD-aware block remap
//
// Values that are not instantiated fall back to the defaults noted at each line.  A forced form stays forced: plan_wind()
// declines what it cannot run in it instead of choosing another (one exception, see there).
inline WindShape wind_shape(const Env& env, int nx, int nlev)
{
  WindShape t; // R = 6 / WPB = 4 run within 1 % of this but fetch more (halo rows, map factors): HBM traffic 1.13-1.14x vs 1.08x of the minimum
  int RB = 8;
  if (env.has_vortdiv_tune) {
    const char* s = env.vortdiv_tune;
    const int K = tune_value(s, "K", 0);
    t.form = K == 1 ? WindForm::Oneshot : K == 2 ? WindForm::OneshotTiles : K == 3 ? WindForm::LevelWalk : K == 4 ? WindForm::Split : WindForm::Rows;
    t.R = tune_value(s, "R", t.R);
    t.D = tune_value(s, "D", t.D);
    t.NT = tune_value(s, "NT", t.NT);
    t.V = tune_value(s, "V", t.V);
    t.ORDER = tune_value(s, "ORDER", t.ORDER);
    t.XCD = tune_value(s, "XCD", t.XCD);
    t.WPB = tune_value(s, "WPB", t.WPB);
    t.ZZ = tune_value(s, "ZZ", t.ZZ);
    t.NTI = tune_value(s, "NTI", t.NTI);
    t.LDSX = tune_value(s, "LDSX", t.LDSX);
    t.lgroup = tune_value(s, "LG", t.lgroup);
    RB = tune_value(s, "RB", RB);
#ifdef MIFC_MEASUREMENT_BUILD
    t.XH = tune_value(s, "XH", 0);
    t.XS = tune_value(s, "XS", 0);
    t.PADROWS = tune_value(s, "PADROWS", 0);
    t.XL = tune_value(s, "XL", 0);
    t.STA = tune_value(s, "STA", 0);
#endif
  }
  if (t.WPB != 1 && t.WPB != 2 && t.WPB != 4 && t.WPB != 8)
    t.WPB = 4; // the kernel is compiled for workgroups of up to 8 waves
  if (t.V != 1 && t.V != 2 && t.V != 3)
    t.V = 2;
  if (nx <= 256)
    t.V = 1; // a second 256-column segment would be empty
  if (t.R < 1)
    t.R = 1;
  const int rmax = 32 / t.V; // map-factor tile in LDS: up to 3*V KiB per row (absvort), 96 KiB at most
  if (t.R > rmax)
    t.R = rmax;
  if (t.D < 0)
    t.D = 0;
  if (t.D > 1)
    t.D = 1; // deeper rings (2, 3) were measured -- same time, profiles/r01/experiments/sweep_d.txt -- and are not instantiated
  while (t.WPB > 1 && t.WPB / 2 >= nlev)
    t.WPB /= 2; // fewer levels than waves: do not launch waves that only stage map factors
  if (t.lgroup < 0)
    t.lgroup = 0;
  // the same keys read for the other forms (after the clamps above, which is why D never asks for a prefetch of 3)
  t.tiles.tile_rows = RB == 14 ? 14 : 8;
  t.levelwalk.waves = (RB == 16 || RB == 12 || RB == 8) ? RB : 16;
  t.levelwalk.halo_waves = t.ZZ != 0;
  t.levelwalk.prefetch = t.D >= 1 ? 2 : 1;
  t.split.tile_rows = (RB == 6 || RB == 8 || RB == 12 || RB == 14) ? RB : 10;
  t.split.loaders = (t.WPB == 2 || t.WPB == 4) ? t.WPB : 0;
  t.split.prefetch = t.D >= 2 ? 3 : (t.D == 1 ? 2 : 1);
  return t;
}

namespace plan_detail {

inline const char* form_name(WindForm f, bool ragged, bool ff)
{
  return f == WindForm::Oneshot ? "wind_oneshot" : f == WindForm::OneshotTiles ? "wind_oneshot_tiles" : f == WindForm::LevelWalk ? "wind_levelwalk"
         : f == WindForm::Split ? (ragged ? "wind_split_ragged" : ff ? "wind_split_ff" : "wind_split") : "wind_rows";
}

// The launch as `chunks` x tiles of tile_rows x tile_cols cells, one workgroup each, spread over the 8 XCDs.
// false: more units than the kernels' 32-bit decode takes.
inline bool set_units(WindPlan& p, int nx, int chunks, int tile_rows, int tile_cols)
{
  p.uB = (p.hi - p.lo + tile_rows - 1) / tile_rows;
  p.uW = (nx + tile_cols - 1) / tile_cols;
  const long units = (long)chunks * p.uB * p.uW;
  if (units > kUnitIndexLimit)
    return false;
  p.n_logical = (int)units;
  p.per_xcd = (p.n_logical + 7) / 8;
  p.grid = p.per_xcd * 8;
  return true;
}

} // namespace plan_detail

// The whole decision.  WindForm::None: not a launch of these kernels (the caller falls back to the flat kernels).
inline WindPlan plan_wind(const WindRequest& rq, const Env& env)
{
  using namespace plan_detail;
  const WindPlan none = [] { WindPlan p; p.form = WindForm::None; return p; }();
  const int nx = rq.nx, nlev = rq.nlev;
  const bool absv = rq.op == WindOp::Absvort, jac = rq.op == WindOp::Jacobian, fused = rq.rv && rq.dv;
  const bool forced = env.has_vortdiv_tune;
  if ((absv && !rq.fc) || (!rq.rv && !rq.dv) || nx < 8 || rq.ny_global < 3 || env.force_cell_kernel)
    return none;
  // the level-walking forms' tests are ONE compare per value ("ordered and != undef"), which is is_def() only for an
  // undef that is not NaN: a NaN undef takes the kernels with the generic two-compare test
  const bool nan_undef_tested = !rq.every_level_all_defined && rq.undef_is_nan;
  const bool deep = env.split_roles && env.levelwalk && !forced; // the default split-role form is available
  // Rows off 16-byte boundaries: only the split-role kernel has a form for them, i.e. deep batches of the wind operators
  // (nx % 256 == 1: the column whose value fillEdges copies into column nx-1 belongs to another workgroup)
  if (rq.ragged && (nx % 256 == 1 || !deep || !env.ragged_split || rq.ff))
    return none;
  // the wind speed as a third output exists in the split-role form only (whole fields, fused pair)
  if (rq.ff && !(fused && rq.op == WindOp::Vortdiv && rq.j0 == 0 && rq.ny_local == rq.ny_global && rq.row_end <= rq.row_begin && !nan_undef_tested && deep &&
                 nlev >= kLevelWalkMinLevels))
    return none;

  WindPlan p;
  static_cast<WindShape&>(p) = wind_shape(env, nx, nlev);
  const long rows = rq.ny_local, waves_per_band = (long)nlev * ((nx + 256 * p.V - 1) / (256 * p.V));
  if (!forced) {
    // A small launch (the reference's single-field call: one level) is latency-bound: shorter
    // bands put more waves on the chip, and their halo re-reads stay in L2.
    // One 1440x720 level: 8-row bands 270 waves, 2-row bands 1077; 8 levels (a chunk of the host pipeline) keep 8.
    // (MIFC_LEVELWALK_MIN_UNITS, the tests' switch, sends launches of any size to the level-walking forms)
    const bool small = env.levelwalk_min_units <= 0 && waves_per_band * ((rows + p.R - 1) / p.R) < kSmallLaunchWaves;
    if (small || nlev <= 2) {
      // ... and the wind operators have forms without any row loop.  Small launches: one 1440x720 level takes
      // 6.7 us (7.5 us with tests and counts) instead of 7.3 (10.8) with 2-row bands, 12.9 (21.6) with 8-row
      // bands.  One or two levels of any size: the row-walking workgroup would be one or two waves holding a
      // 32-KiB map-factor tile (5 waves per CU); a 4000x4000 level straight from HBM runs at 48 % of peak
      // that way, 66 % one-shot, 69 % as one-shot tiles with the row reuse in LDS
      // (profiles/r01/other_configs.jsonl, cold numbers).
      p.form = (small || jac) ? WindForm::Oneshot : WindForm::OneshotTiles;
    } else if (((!jac && !absv) || (env.split_roles && !nan_undef_tested)) && nlev >= kLevelWalkMinLevels && env.levelwalk) {
      // Deep batches: tiles that stay put and walk the levels (map factors once per chunk of levels, a narrow
      // window of each array open at any time).  12-wave workgroups, 10 computed rows + 2 halo waves, chunks of
      // about 6 levels (8 in shallower batches), balanced; 3-6 % faster than the row-walking kernel on every device tried
      // (profiles/r02/experiments/sweep_k3_*.txt).
      const long tiles = ((rows + 9) / 10) * ((nx + 255) / 256);
      const int target = nlev >= 48 ? 6 : 8; // levels per chunk; the chunks are then balanced
      const int nchunks = (nlev + target - 1) / target;
      if (tiles * nchunks >= (env.levelwalk_min_units > 0 ? env.levelwalk_min_units : kLevelWalkMinUnits)) {
        p.form = WindForm::LevelWalk;
        p.levelwalk.waves = 12;
        p.levelwalk.halo_waves = 1;
        p.levelwalk.prefetch = 1;
        p.lgroup = (nlev + nchunks - 1) / nchunks;
        // The same tiles with split roles -- 2 loader waves bring 14 rows of u and v straight into LDS two levels
        // ahead, 12 compute waves only read LDS and store (vortdiv_split_kernel).  The fused pair: 1-5 % faster than the
        // form above on every box, placement and shape tried, 4 % on the tested variant, up to 18 % on shallow batches
        // (profiles/r02/experiments/sweep_k4_*.txt, ab_split_roles.txt).  Absvort too (+2 % on the row-walking
        // kernel it ran before, which has no level-walking form of the first kind); relvort / divergence ALONE measure
        // the same in both forms (12 B per cell: +-1 %, the sign depends on the box -- profiles/r03/split_role_ops.txt) and
        // keep the first, MIFC_VORTDIV_TUNE="K=4,..." selects the split-role one.
        // (single outputs on big tested levels too: that kernel leaves its counts in the partials buffer, the first form adds them one by one)
        const bool big_tested = rq.has_partials && !rq.every_level_all_defined && tiles >= kPartialCountUnitsPerLevel;
        if (env.split_roles && !nan_undef_tested && (fused || absv || jac || rq.ragged || big_tested)) {
          p.form = WindForm::Split;
          p.split.tile_rows = 12;
          p.split.loaders = 2;
          p.split.prefetch = 2;
        }
      }
    }
    while (p.R > 2 && waves_per_band * ((rows + p.R - 1) / p.R) < kSmallLaunchWaves)
      p.R /= 2;
  }

  p.nyg = rq.ny_global - p.PADROWS;
  p.ny_local = rq.ny_local - p.PADROWS;
  p.lo = (rq.j0 >= 1) ? 0 : (1 - rq.j0);
  const int last = p.nyg - 1 - rq.j0; // local index of the global last row
  p.hi = (p.ny_local < last) ? p.ny_local : last;
  if (rq.row_end > rq.row_begin) { // a caller-chosen range of owned rows (halo overlap)
    p.lo = p.lo > rq.row_begin ? p.lo : rq.row_begin;
    p.hi = p.hi < rq.row_end ? p.hi : rq.row_end;
  }
  if (p.hi <= p.lo)
    return none; // slab without a single computed row (can only be a 1-row edge slab)
  // A row slab carries one halo row before owned row 0 and one after the last owned row; a whole field has neither.
  const bool has_north_halo = rq.j0 > 0;
  const bool has_south_halo = rq.j0 + p.ny_local < p.nyg;
  p.idx_lo = has_north_halo ? -(long)nx : 0;
  p.idx_hi = (long)nx * (p.ny_local + (has_south_halo ? 1 : 0)) - 1;
  // the row-walking geometry: units are (group of WPB levels, band of R rows, 256 * V columns).  Every form's launch has to fit it
  p.uL = (nlev + p.WPB - 1) / p.WPB;
  if (!set_units(p, nx, p.uL, p.R, 256 * p.V))
    return none;
  p.nbands = p.uB;
  p.nwc = p.uW;

  // only the split-role kernel has the third output / takes rows at any alignment
  if ((rq.ff || rq.ragged) && p.form != WindForm::Split)
    return none;
  p.note = form_name(p.form, rq.ragged, rq.ff);
  // big tested levels: counts by plain stores + one small launch (StencilParams::partials).  The one-shot tiles index
  // partials[unit of the launch], which is level-major only in address order
  auto counts_by_partials = [&](bool level_walking) {
    const long per_level = (long)p.uB * p.uW;
    return rq.has_partials && !rq.every_level_all_defined && !rq.ff && (level_walking || p.lgroup == 0) && per_level >= kPartialCountUnitsPerLevel &&
           per_level * nlev <= rq.partials_cap;
  };
  // the level-walking forms: levels per workgroup, 32-bit offsets inside a level
  auto level_chunks = [&] {
    p.lgroup = (p.lgroup > 0 && p.lgroup < nlev) ? p.lgroup : nlev;
    return (nlev + p.lgroup - 1) / p.lgroup;
  };
  const bool level_fits = (long)nx * (p.ny_local + 2) < 0x7fffffffL;

  if (p.form == WindForm::Split && nan_undef_tested) {
    // Only a forced tuning gets here, and it is the one case where another form runs than the one asked for: the first
    // level-walking form, one level ahead.  Absvort has no such form.
    if (absv)
      return none;
    p.form = WindForm::LevelWalk;
    p.levelwalk.prefetch = 1;
  }
  if (p.form == WindForm::Split && jac && forced)
    return none; // the Jacobian has the default shape only
  // forms an operator does not have: absvort and the Jacobian walk levels in the split-role form only, and the Jacobian has no tiles
  if ((p.form == WindForm::LevelWalk && (absv || jac)) || (p.form == WindForm::OneshotTiles && jac))
    p.form = WindForm::Rows; // (forced tunings only; reported under the name of the form asked for)

  switch (p.form) {
  case WindForm::Oneshot: // units are (level, block of 4 rows, 256-column segment)
    if (!set_units(p, nx, nlev, 4, 256))
      return none;
    if (absv || jac)
      p.NT = 1;
    p.block = 256;
    break;
  case WindForm::OneshotTiles: // units are (level, block of tile_rows rows, 256-column segment)
    if (!fused || absv)
      p.tiles.tile_rows = 8;
    if (!set_units(p, nx, nlev, p.tiles.tile_rows, 256))
      return none;
    p.block = 64 * (p.tiles.tile_rows + 2);
    p.counts_by_partials = counts_by_partials(false);
    break;
  case WindForm::LevelWalk: // units are (level chunk, row block, 256-column segment)
    if (!fused) {         // one output: the default shape only
      p.levelwalk.waves = 12;
      p.levelwalk.halo_waves = 1;
      p.levelwalk.prefetch = 1;
    }
    if (!set_units(p, nx, level_chunks(), p.levelwalk.waves - (p.levelwalk.halo_waves ? 2 : 0), 256) || !level_fits)
      return none;
    p.block = 64 * p.levelwalk.waves;
    break;
  case WindForm::Split: { // the same units; loader waves / compute waves
    auto& s = p.split;
    const bool single = !fused || absv;
    if (single || rq.ragged || rq.ff || jac) { // the default shape only (one output: and its one-level-ahead sibling)
      s.tile_rows = 12;
      s.loaders = 2;
      s.prefetch = (single && !rq.ragged && !jac && s.prefetch == 1) ? 1 : 2;
    } else { // the shapes that are instantiated: 6, 8 and 14 rows with 2 loaders, 10 and 12 rows with 2 or 4; three levels ahead not everywhere
      if (s.tile_rows == 10)
        s.loaders = s.loaders == 2 ? 2 : 4;
      else
        s.loaders = (s.tile_rows == 12 && s.loaders == 4) ? 4 : 2;
      const bool pf3 = s.tile_rows == 6 || s.tile_rows == 8 || (s.tile_rows == 12 && s.loaders == 2) || (s.tile_rows == 10 && s.loaders == 4);
      if (s.prefetch == 3 && !pf3)
        s.prefetch = 2;
    }
    const int nchunks = level_chunks();
    if (!set_units(p, nx, nchunks, s.tile_rows, 256) || !level_fits)
      return none;
    p.block = 64 * (s.tile_rows + s.loaders);
    p.counts_by_partials = counts_by_partials(true);
    break;
  }
  default: // Rows: the geometry is set.  What is instantiated: plain stores and single outputs at the default depth only;
           // the Jacobian with nontemporal stores, 1 or 2 float4 per lane, and without the LDSX experiment
    if (jac) {
      // (the bands were laid out for the V asked for: a forced V=3 leaves the third 256 columns of each to no wave)
      p.V = p.V == 3 ? 2 : p.V;
      p.NT = 1;
      p.LDSX = 0;
    }
    if (!p.NT || !fused || jac)
      p.D = 1;
    p.block = 64 * p.WPB;
    p.lds = (long)p.R * 1024 * p.V * (absv ? 3 : 2) + (long)p.LDSX * 1024;
    break;
  }
  return p;
}

} // namespace mifc

#endif // MIFC_VORTDIV_PLAN_H
