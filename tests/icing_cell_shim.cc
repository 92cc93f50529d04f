// The host build of the per-cell vessel-icing models (mi-fieldcalc_amd/csrc/mifc_icing_cell.h, the text the GPU kernels
// compile) over a whole field, with the reference's field loop and flag.  Compiled at test time with g++
// (-ffp-contract=off, glibc libm); tests/test_vessel_icing_cpu.py compares it with the compiled reference bit for bit.
// The trip-count histograms feed tools/bench_vessel_icing.py.
#include "mifc_icing_cell.h"

#include <vector>

namespace {
struct HistTrips
{
  long long* disp_h;  // [10002]: trips of the shallow-water fixed point
  long long* level_h; // [1002]: trips of the per-level freezing-fraction loop (MINCOG: the bisection's)
  void count_disp(int j) const
  {
    if (disp_h)
      disp_h[j < 10001 ? j : 10001] += 1;
  }
  void count_level(int j) const
  {
    if (level_h)
      level_h[j < 1001 ? j : 1001] += 1;
  }
  void disp(int j) const { count_disp(j); }
  void level(int j) const { count_level(j); }
};
} // namespace

extern "C" {

// 1 computed, 0 the reference's false, -1 the level count overflows an int
int iccell_run(int model, int nx, int ny, const float* const* in, float vs, float alpha, float zmin, float zmax, int alt, float* icing, int* fdefined,
               float undef, long long* disp_hist, long long* level_hist)
{
  mifc_icing::IcingConsts C;
  const int rc = mifc_icing::icing_consts(model, vs, alpha, zmin, zmax, alt, &C);
  if (rc != 1)
    return rc;
  std::vector<double> E((size_t)C.number);
  for (int k = 0; k < C.number; ++k)
    E[(size_t)k] = mifc_icing::icing_level_factor(zmin, k);
  HistTrips tr = {disp_hist, level_hist};
  const bool all = *fdefined == 0;
  const long n = (long)nx * ny;
  long bad = 0;
  for (long i = 0; i < n; ++i) {
    const float sal = in[0][i], wave = in[1][i], xw = in[2][i], yw = in[3][i], at = in[4][i], rh = in[5][i], sst = in[6][i], p = in[7][i],
                Pw = in[8][i], aice = in[9][i], depth = in[10][i];
    if (mifc_icing::icing_defined(model, all, sal, wave, xw, yw, at, rh, sst, p, aice, depth, undef)) {
      icing[i] = model == mifc_icing::MODSTALL ? mifc_icing::modstall_cell(sal, wave, xw, yw, at, rh, sst, p, Pw, depth, C, E, tr)
                                               : mifc_icing::mincog_cell(sal, wave, xw, yw, at, rh, sst, p, Pw, depth, C, E, tr);
    } else {
      icing[i] = undef;
      bad += 1;
    }
  }
  *fdefined = bad == 0 ? 0 : (bad == n ? 1 : 2);
  return 1;
}

// mismatches of sinhf_fdlibm against glibc's sinhf over the floats lo_bits, lo_bits + stride, ... < hi_bits, both signs
long long iccell_sinhf_mismatches(unsigned lo_bits, unsigned hi_bits, unsigned stride)
{
  long long d = 0;
  for (unsigned u = lo_bits; u < hi_bits; u += stride)
    for (int s = 0; s < 2; ++s) {
      const float x = mifc_icing::bits_fl(u | (s ? 0x80000000u : 0u));
      if (mifc_icing::fl_bits(mifc_icing::sinhf_fdlibm(x)) != mifc_icing::fl_bits(std::sinh(x)))
        d += 1;
    }
  return d;
}

int iccell_bisect_iterations()
{
  mifc_icing::IcingConsts C = mifc_icing::IcingConsts();
  mifc_icing::icing_consts(mifc_icing::MINCOG, 0, 0, 0, 0, 1, &C);
  return C.bisect_iter;
}

} // extern "C"
