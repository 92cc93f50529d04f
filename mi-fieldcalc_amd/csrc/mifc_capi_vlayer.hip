// mifc_capi_vlayer.hip -- C ABI of mifc_vlayer_hlevels / mifc_vlayer_fields (include/mifc.h; EXTENSION, no reference
// function) on the level-batch driver (mifc_levelbatch.h): its own refusals, the product slots, two or four fields per
// launch of the kernel of mifc_vlayer.hip (vlayer_pass_fields).
#include "mifc_levelbatch.h"

using namespace mifc_host;

namespace {

struct Call
{
  LevelBatchCall b;
  float lo, hi;
  const float *lo_field, *hi_field;
  const int* products;
  int nproducts;
  float* const* fres;
  int* fdefined_out;
};

int run(mifc_ctx* c, const Call& call)
{
  CTX_OR_FAIL(c);
  const LevelBatchCall& a = call.b;
  const int nf = a.nfields, np = call.nproducts, nlev = a.nlev;
  if (!check_counts(c, a, mifc::VLAYER_MAX_FIELDS))
    return 0;
  if (np < 1 || np > mifc::VLAYER_PRODUCTS)
    return refuse(c, a, "nproducts " + std::to_string(np) + " outside 1.." + std::to_string(mifc::VLAYER_PRODUCTS));
  if (!check_grid(c, a))
    return 0;
  if (!a.fields || !call.fres || !call.fdefined_out || !call.products || !a.coord || (a.hybrid() && (!a.alevel || !a.blevel)))
    return refuse(c, a, a.hybrid() ? "a null pointer (fields, ps, alevel, blevel, products, fres or fdefined_out)"
                                   : "a null pointer (fields, coord, products, fres or fdefined_out)");
  if (!check_field_pointers(c, a, call.fres))
    return 0;
  int slot[mifc::VLAYER_PRODUCTS], group = 0;
  std::fill(slot, slot + mifc::VLAYER_PRODUCTS, -1);
  for (int p = 0; p < np; ++p) {
    const int code = call.products[p];
    if (code < MIFC_VLAYER_INTEGRAL || code > MIFC_VLAYER_COORD_OF_MIN)
      return refuse(c, a, "products[" + std::to_string(p) + "] = " + std::to_string(code) + " is no MIFC_VLAYER_* product");
    if (slot[code - 1] >= 0)
      return refuse(c, a, "product " + std::to_string(code) + " asked for twice");
    slot[code - 1] = p;
    group |= code <= MIFC_VLAYER_MEAN ? mifc::VLAYER_SUMS : mifc::VLAYER_EXTREMES;
  }
  // a scalar bound in use: against the other scalar, or at least a number (the per-cell test of rule 2 does the rest)
  if (!call.lo_field && !call.hi_field && !(call.lo < call.hi))
    return refuse(c, a, "the layer is empty: not lo < hi");
  if ((!call.lo_field && call.lo != call.lo) || (!call.hi_field && call.hi != call.hi))
    return refuse(c, a, "a NaN bound");
  if (!check_levels(c, a))
    return 0;
  const size_t cells = a.cells(), plane = cells * sizeof(float);
  if (!check_overlaps(c, a, {{call.fres, nf, plane * (size_t)np, "fres"}}, {{call.lo_field, plane, "lo_field"}, {call.hi_field, plane, "hi_field"}}))
    return 0;
  if (cells == 0) {
    std::fill_n(call.fdefined_out, nf * np, MIFC_ALL_DEFINED); // checkDefined(0, 0)
    return 1;
  }

  LevelTable tab;
  Staging st(c, a.memkind); // blocks only: a host batch is staged band by band
  if (!tab.build(c, a, (size_t)nf) || !tab.upload(c, st))
    return 0;
  BandPlan plan;
  PlaneGroup *in[mifc::VLAYER_MAX_FIELDS], *out[mifc::VLAYER_MAX_FIELDS];
  for (int f = 0; f < nf; ++f)
    in[f] = plan.in(a.fields[f], (size_t)nlev);
  PlaneGroup *coord = plan.in(a.coord, a.coord_planes()), *lo = plan.in(call.lo_field, 1), *hi = plan.in(call.hi_field, 1);
  for (int f = 0; f < nf; ++f)
    out[f] = plan.out(call.fres[f], (size_t)np);
  if (!plan.place(c, st, a, (size_t)(mifc::env().vlayer_chunk_mib > 0 ? mifc::env().vlayer_chunk_mib : 256) << 20))
    return 0;

  mifc::VlayerParams P;
  fill_params(P, a, tab, plan, coord);
  P.hybrid = a.hybrid() ? 1 : 0;
  P.group = group;
  P.lo = call.lo;
  P.hi = call.hi;
  std::copy(slot, slot + mifc::VLAYER_PRODUCTS, P.slot);
  P.lo_field = lo->dev;
  P.hi_field = hi->dev;

  // the launches of one problem of rows.n() columns: vlayer_pass_fields(group) fields each
  auto launch_passes = [&](const BandRows& rows) -> int {
    P.n = rows.n();
    const int pass = mifc::vlayer_pass_fields(group);
    for (int f0 = 0; f0 < nf; f0 += pass) {
      P.f0 = f0;
      P.nfields = std::min(pass, nf - f0);
      for (int f = 0; f < P.nfields; ++f) {
        P.fields[f] = in[f0 + f]->dev;
        P.out[f] = out[f0 + f]->dev;
      }
      MIFC_LAUNCH(c, mifc::launch_vlayer(P, c->stream));
    }
    return 1;
  };
  if (!plan.run(c, a, launch_passes) || !tab.read_counts(c) || !st.finish()) // finish(): the one synchronisation of the call
    return 0;
  for (int f = 0; f < nf; ++f)
    for (int p = 0; p < np; ++p)
      call.fdefined_out[f * np + p] = tab.classify((size_t)f, cells);
  return 1;
}

} // namespace

extern "C" {

int mifc_vlayer_hlevels(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields, const float* ps,
                        int fdef_ps, const float* alevel, const float* blevel, float lo, float hi, const float* lo_field, const float* hi_field,
                        const int* products, int nproducts, float* const* fres, int* fdefined_out, float undef, int memkind)
{
  const Call a = {{"mifc_vlayer_hlevels", COORD_HYBRID, nx, ny, nlev, fields, fdefined_in, nfields, ps, fdef_ps, nullptr, alevel, blevel, undef, memkind},
                  lo, hi, lo_field, hi_field, products, nproducts, fres, fdefined_out};
  return run(c, a);
}

int mifc_vlayer_fields(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields, const float* coord,
                       const int* fdef_coord, float lo, float hi, const float* lo_field, const float* hi_field, const int* products,
                       int nproducts, float* const* fres, int* fdefined_out, float undef, int memkind)
{
  const Call a = {{"mifc_vlayer_fields", COORD_FIELD, nx, ny, nlev, fields, fdefined_in, nfields, coord, MIFC_SOME_DEFINED, fdef_coord, nullptr,
                   nullptr, undef, memkind},
                  lo, hi, lo_field, hi_field, products, nproducts, fres, fdefined_out};
  return run(c, a);
}

} // extern "C"
