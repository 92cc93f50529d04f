// C entry around plan_wind() (mi-fieldcalc_amd/csrc/mifc_vortdiv_plan.h) for tests/test_vortdiv_plan_cpu.py: host compiler only.
#include <cstdio>
#include <cstring>

#include "mifc_vortdiv_plan.h"

extern "C" {

// rq: op (0 relvort, 1 divergence, 2 vortdiv, 3 absvort, 4 jacobian), nx, ny_global, j0, ny_local, nlev, row_begin, row_end, rv, dv, ff, fc,
//     ragged, every_level_all_defined, undef_is_nan
// sw: MIFC_VORTDIV_SPLIT, MIFC_VORTDIV_LEVELWALK, MIFC_RAGGED_SPLIT, MIFC_LEVELWALK_MIN_UNITS, MIFC_FORCE_CELL_KERNEL
// out: form, grid, block, lds, R, V, D, NT, WPB, tiles.tile_rows, levelwalk.waves, .halo_waves, .prefetch, split.tile_rows, .loaders, .prefetch,
//      lgroup, uB, uW, n_logical, counts_by_partials
void mifc_test_plan_wind(const int* rq, const char* tune, const int* sw, long partials_cap, long* out, char* note, int note_len)
{
  mifc::WindRequest r{};
  r.op = (mifc::WindOp)rq[0];
  r.nx = rq[1];
  r.ny_global = rq[2];
  r.j0 = rq[3];
  r.ny_local = rq[4];
  r.nlev = rq[5];
  r.row_begin = rq[6];
  r.row_end = rq[7];
  r.rv = rq[8];
  r.dv = rq[9];
  r.ff = rq[10];
  r.fc = rq[11];
  r.ragged = rq[12];
  r.every_level_all_defined = rq[13];
  r.undef_is_nan = rq[14];
  r.has_partials = partials_cap > 0;
  r.partials_cap = partials_cap;
  mifc::Env e;
  e.split_roles = sw[0];
  e.levelwalk = sw[1];
  e.ragged_split = sw[2];
  e.levelwalk_min_units = sw[3];
  e.force_cell_kernel = sw[4];
  e.has_vortdiv_tune = tune && *tune;
  if (e.has_vortdiv_tune)
    std::snprintf(e.vortdiv_tune, sizeof e.vortdiv_tune, "%s", tune);
  const mifc::WindPlan p = mifc::plan_wind(r, e);
  const long v[] = {(long)p.form, p.grid, p.block, p.lds, p.R, p.V, p.D, p.NT, p.WPB, p.tiles.tile_rows, p.levelwalk.waves, p.levelwalk.halo_waves,
                    p.levelwalk.prefetch, p.split.tile_rows, p.split.loaders, p.split.prefetch, p.lgroup, p.uB, p.uW, p.n_logical, p.counts_by_partials};
  std::memcpy(out, v, sizeof v);
  std::snprintf(note, (size_t)note_len, "%s", p.note);
}
}
