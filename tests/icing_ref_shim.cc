// Flat C wrappers around the reference's iterative vessel-icing models, for tests/test_vessel_icing_cpu.py,
// tests/test_gpu_vessel_icing.py and tools/bench_vessel_icing.py.  Compiled at test time into a temporary directory
// and linked against oracle/_ref/libmifc_ref.so, which exports miutil::fieldcalc::vesselIcingModStall /
// vesselIcingMincog (tests/golden/reference_symbols.txt).  The prototypes come from the project's source-compatible
// header; the tests load the result with RTLD_LOCAL | RTLD_DEEPBIND, so these calls bind to the reference library's
// definitions and never to libmi-fieldcalc.so's.
#include <mi_fieldcalc/FieldCalculations.h>

extern "C" {

int icref_modstall(int nx, int ny, const float* const* in, float vs, float alpha, float zmin, float zmax, float* icing, int* fdefined, float undef)
{
  miutil::ValuesDefined f = static_cast<miutil::ValuesDefined>(*fdefined);
  const bool ok = miutil::fieldcalc::vesselIcingModStall(nx, ny, in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], in[8], in[9], in[10], vs,
                                                         alpha, zmin, zmax, icing, f, undef);
  *fdefined = static_cast<int>(f);
  return ok ? 1 : 0;
}

int icref_mincog(int nx, int ny, const float* const* in, float vs, float alpha, float zmin, float zmax, int alt, float* icing, int* fdefined,
                 float undef)
{
  miutil::ValuesDefined f = static_cast<miutil::ValuesDefined>(*fdefined);
  const bool ok = miutil::fieldcalc::vesselIcingMincog(nx, ny, in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], in[8], in[9], in[10], vs,
                                                       alpha, zmin, zmax, alt, icing, f, undef);
  *fdefined = static_cast<int>(f);
  return ok ? 1 : 0;
}

} // extern "C"
