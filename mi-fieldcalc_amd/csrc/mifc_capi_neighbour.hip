// mifc_capi_neighbour.hip -- C ABI of the neighbourhood statistics
// (FieldCalculations.cc:2862-3061): the reference's argument handling, the
// refusals where the reference is undefined ("Neighbourhood
// statistics"), then the kernels of mifc_neighbour.hip.
#include "mifc_ctx.h"

#include <string>

using namespace mifc_host;

namespace {

// the reference converts its float constants with `int x = constants[k]`: defined only for values that truncate into int
bool const_to_int(mifc_ctx* c, const char* fn, const float* constants, int k, int* out)
{
  const float v = constants[k];
  if (!(v >= -2147483648.0f && v < 2147483648.0f)) {
    c->err = std::string(fn) + ": constant " + std::to_string(k) + " is NaN or outside the int range (the reference's conversion is undefined)";
    return false;
  }
  *out = (int)v;
  return true;
}

// What one call computes.  kind: 0 nothing to write (success), 1 threshold 0/1 (range 0), 2 box count, 3 window walk
struct NbPlan
{
  int kind;
  bool flag_unchanged;
  bool keeps_cells; // neighbourFunctions leaves interior cells that no block covers as they were
  mifc::NeighbourParams P;
};

// 1: plan made.  0: refused -- the reference's `false` (c->err empty) or a deviation (c->err says which).
int nb_plan(mifc_ctx* c, int which, int compute, int nx, int ny, const float* field, const float* fres, const float* constants, int nconstants,
            const char* fn, NbPlan* p)
{
  p->kind = 0;
  p->flag_unchanged = false;
  p->keeps_cells = false;
  mifc::NeighbourParams& P = p->P;
  P = mifc::NeighbourParams();
  if (nx < 1 || ny < 1 || (long)nx * (long)ny > 0x7fffffffL || !field || !fres || (nconstants > 0 && !constants))
    return 0;
  P.nx = nx;
  P.ny = ny;
  P.compute = compute;
  P.in = field;
  P.out = const_cast<float*>(fres);
  int limit = 0, range = 3, step = 3;
  if (which == MIFC_NEIGHBOUR_PROB) {
    if (nconstants < 2) // :2871
      return 0;
    if (!const_to_int(c, fn, constants, 0, &limit) || !const_to_int(c, fn, constants, 1, &range))
      return 0;
    if (range < 0 || range > nx || range > ny) {
      c->err = std::string(fn) + ": range < 0 or larger than nx / ny (the reference reads and writes outside the field)";
      return 0;
    }
    P.range = range;
    P.limit = (float)limit;
    if (range == 0) { // :2880-2893: the 0/1 field (compute 5 / 6) or nothing, the flag as it was
      p->kind = (compute == 5 || compute == 6) ? 1 : 0;
      p->flag_unchanged = true;
      return 1;
    }
    if (compute != 5 && compute != 6) {
      c->err = std::string(fn) + ": compute must be 5 or 6 when range > 0 (the reference box-averages the uninitialised output)";
      return 0;
    }
    P.nf = (float)((2 * range + 1) * (2 * range + 1)); // :2917
    p->kind = 2;
    return 1;
  }
  // neighbourFunctions :2967-2986
  if (nconstants < 1 || (nconstants < 2 && compute > 3))
    return 0;
  if (compute < 4) {
    if (!const_to_int(c, fn, constants, 0, &range) || (nconstants == 2 && !const_to_int(c, fn, constants, 1, &step)))
      return 0;
  } else {
    if (!const_to_int(c, fn, constants, 0, &limit) || !const_to_int(c, fn, constants, 1, &range) ||
        (nconstants == 3 && !const_to_int(c, fn, constants, 2, &step)))
      return 0;
  }
  if (range > nx || range > ny || range < 1 || step < 1)
    return 0;
  if (step / 2 > range) {
    c->err = std::string(fn) + ": step / 2 > range (the reference's blocks overlap, wrap across rows and can leave the field)";
    return 0;
  }
  const float ngridp = (float)((2 * range + 1) * (2 * range + 1)); // :3008
  if (compute == 4) {
    const float q = ngridp * (float)limit / 100.0f; // :3010, in the reference's float operations
    if (!(q > -1.0f && q < ngridp)) {
      c->err = std::string(fn) + ": the percentile index is outside the window (the reference reads outside its value list)";
      return 0;
    }
    P.ii = (int)q;
  }
  if (field == fres) {
    c->err = std::string(fn) + ": field == fres (the reference's result then depends on its own loop order)";
    return 0;
  }
  P.range = range;
  P.step = step;
  P.limit = (float)limit;
  P.nf = ngridp;
  // compute 5 / 6 at every cell is the box count (same count, same division, same border)
  p->kind = ((compute == 5 || compute == 6) && step == 1) ? 2 : 3;
  p->keeps_cells = step > 1;
  return 1;
}

int nb_run(mifc_ctx* c, NbPlan& p, int nlev, const float* field, float* fres, int* fdefined, int nflags, float undef, int memkind)
{
  mifc::NeighbourParams& P = p.P;
  const size_t n = (size_t)P.nx * (size_t)P.ny * (size_t)nlev;
  if (p.kind != 0) {
    Staging st(c, memkind);
    P.nlev = nlev;
    P.level_stride = (long)P.nx * (long)P.ny;
    P.undef = undef;
    P.in = st.in(field, n);
    // host fields: cells that no block covers must come back as the caller had them
    P.out = st.out(fres, n, p.keeps_cells);
    if (!st.ok())
      return 0;
    if (p.kind == 2) {
      P.bits = static_cast<u64*>(st.scratch((size_t)nlev * P.ny * mifc::neighbour_words(P.nx) * sizeof(u64)));
      if (!st.ok())
        return 0;
      MIFC_LAUNCH(c, mifc::launch_neighbour_box(P, c->stream));
    } else if (p.kind == 1) {
      MIFC_LAUNCH(c, mifc::launch_neighbour_threshold(P, c->stream));
    } else {
      MIFC_LAUNCH(c, mifc::launch_neighbour_functions(P, c->stream));
    }
    if (!st.finish())
      return 0;
  }
  if (!p.flag_unchanged)
    for (int l = 0; l < nflags; ++l)
      fdefined[l] = MIFC_SOME_DEFINED; // :2928, :2988
  return 1;
}

} // namespace

extern "C" {

int mifc_neighbourProbFunctions(mifc_ctx* c, int nx, int ny, const float* field, const float* constants, int nconstants, int compute, float* fres,
                                int* fdefined, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  if (!fdefined || *fdefined != MIFC_ALL_DEFINED) // :2868
    return 0;
  NbPlan p;
  if (!nb_plan(c, MIFC_NEIGHBOUR_PROB, compute, nx, ny, field, fres, constants, nconstants, "neighbourProbFunctions", &p))
    return 0;
  return nb_run(c, p, 1, field, fres, fdefined, 1, undef, memkind);
}

int mifc_neighbourFunctions(mifc_ctx* c, int nx, int ny, const float* field, const float* constants, int nconstants, int compute, float* fres,
                            int* fdefined, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  if (!fdefined || *fdefined != MIFC_ALL_DEFINED) // :2965
    return 0;
  NbPlan p;
  if (!nb_plan(c, MIFC_NEIGHBOUR_FUNCTIONS, compute, nx, ny, field, fres, constants, nconstants, "neighbourFunctions", &p))
    return 0;
  return nb_run(c, p, 1, field, fres, fdefined, 1, undef, memkind);
}

int mifc_neighbour_levels(mifc_ctx* c, int which, int compute, int nx, int ny, int nlev, const float* field, const float* constants, int nconstants,
                          float* fres, int* fdefined, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  if (which != MIFC_NEIGHBOUR_PROB && which != MIFC_NEIGHBOUR_FUNCTIONS) {
    c->err = "mifc_neighbour_levels: which must be MIFC_NEIGHBOUR_PROB or MIFC_NEIGHBOUR_FUNCTIONS";
    return 0;
  }
  if (nlev < 1 || !fdefined)
    return 0;
  for (int l = 0; l < nlev; ++l)
    if (fdefined[l] != MIFC_ALL_DEFINED)
      return 0;
  const long cells = (long)nx * (long)ny;
  if (cells > 0 && (long)nlev > 0x7fffffffL / cells) {
    c->err = "mifc_neighbour_levels: the batch holds more than 2^31 - 1 cells";
    return 0;
  }
  NbPlan p;
  const char* fn = which == MIFC_NEIGHBOUR_PROB ? "neighbourProbFunctions" : "neighbourFunctions";
  if (!nb_plan(c, which, compute, nx, ny, field, fres, constants, nconstants, fn, &p))
    return 0;
  return nb_run(c, p, nlev, field, fres, fdefined, nlev, undef, memkind);
}

} // extern "C"
