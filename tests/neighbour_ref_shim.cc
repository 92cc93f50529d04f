// Flat C wrappers around the reference's neighbourhood functions, for tests/test_neighbour_cpu.py and
// tests/test_gpu_neighbour.py.  Compiled at test time into a temporary directory and linked against
// oracle/_ref/libmifc_ref.so, which exports miutil::fieldcalc::neighbourProbFunctions / neighbourFunctions
// (tests/golden/reference_symbols.txt).  The prototypes come from the project's source-compatible header;
// the tests load the result with RTLD_LOCAL | RTLD_DEEPBIND, so these calls bind to the reference library's
// definitions and never to libmi-fieldcalc.so's.
#include <mi_fieldcalc/FieldCalculations.h>

#include <vector>

namespace {
typedef bool (*NeighbourFn)(int, int, const float*, const std::vector<float>&, int, float*, miutil::ValuesDefined&, float);

int call(NeighbourFn fn, int nx, int ny, const float* field, const float* constants, int nconstants, int compute, float* fres, int* fdefined,
         float undef)
{
  const std::vector<float> c(constants, constants + nconstants);
  miutil::ValuesDefined f = static_cast<miutil::ValuesDefined>(*fdefined);
  const bool ok = fn(nx, ny, field, c, compute, fres, f, undef);
  *fdefined = static_cast<int>(f);
  return ok ? 1 : 0;
}
} // namespace

extern "C" {

int nbref_neighbourProbFunctions(int nx, int ny, const float* field, const float* constants, int nconstants, int compute, float* fres,
                                 int* fdefined, float undef)
{
  return call(miutil::fieldcalc::neighbourProbFunctions, nx, ny, field, constants, nconstants, compute, fres, fdefined, undef);
}

int nbref_neighbourFunctions(int nx, int ny, const float* field, const float* constants, int nconstants, int compute, float* fres, int* fdefined,
                             float undef)
{
  return call(miutil::fieldcalc::neighbourFunctions, nx, ny, field, constants, nconstants, compute, fres, fdefined, undef);
}

} // extern "C"
