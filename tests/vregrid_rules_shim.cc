// C entries around mifc_vregrid_rules.h (mi-fieldcalc_amd/csrc) for tests/test_vregrid_cpu.py: host compiler only, built
// with -ffp-contract=off.  A whole call goes through tests/host/vregrid_rules_driver.h.
#include "host/vregrid_rules_driver.h"

extern "C" {

void mifc_test_vregrid_run(int kind, int nx, int ny, int nlev, int nf, int nt, const float* fields, const int* fdefined_in, const float* coord,
                           int fdef_ps, const int* fdef_coord, const float* alevel, const float* blevel, const float* tcoord, const int* fdef_tcoord,
                           int method, int from, int outside, float undef, float* out, int* flags)
{
  const vregrid_test::Call c = {kind, nx, ny, nlev, nf, nt, fields, fdefined_in, coord, fdef_ps, fdef_coord, alevel, blevel, tcoord, fdef_tcoord,
                                method, from, outside, undef};
  vregrid_test::run(c, out, flags);
}

// one column of nlev usable-or-NaN coordinates: out = kmin, kmax as the walk in the given direction leaves them
void mifc_test_vregrid_extremes(const float* col, int nlev, int descending, int* out)
{
  mifc::VregridExtremes e;
  mifc::vregrid_extremes_start(e);
  for (int s = 0; s < nlev; ++s) {
    const int k = descending ? nlev - 1 - s : s;
    mifc::vregrid_extremes_level(e, col[k], k, descending != 0);
  }
  out[0] = e.kmin;
  out[1] = e.kmax;
}

int mifc_test_vregrid_brackets(float c_a, float c_b, float ct)
{
  return mifc::vregrid_brackets(c_a, c_b, ct) ? 1 : 0;
}

} // extern "C"
