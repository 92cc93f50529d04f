// mifc_capi_vderiv.hip -- C ABI of mifc_vderiv_hlevels / mifc_vderiv_fields / mifc_vderiv_levels (include/mifc.h;
// EXTENSION, no reference function) on the level-batch driver (mifc_levelbatch.h): its own refusals, for the `levels`
// form the weights in the tail of the device table (vderiv_level_weights), two or four fields per launch of the kernel
// of mifc_vderiv.hip (vderiv_pass_fields).
#include "mifc_levelbatch.h"

using namespace mifc_host;

static_assert(COORD_HYBRID == mifc::VDERIV_HYBRID && COORD_FIELD == mifc::VDERIV_FIELD && COORD_LEVELS == mifc::VDERIV_LEVELS, "VderivParams::kind");

namespace {

struct Call
{
  LevelBatchCall b;
  int method;
  float* const* fres;
  int* fdefined_out;
  float* const* fmag;
  int* fdefined_mag;
};

int run(mifc_ctx* c, const Call& call)
{
  CTX_OR_FAIL(c);
  const LevelBatchCall& a = call.b;
  const bool by_level = a.kind == COORD_LEVELS;
  if (!check_counts(c, a, mifc::VDERIV_MAX_FIELDS) || !check_grid(c, a))
    return 0;
  if (call.method != MIFC_VDERIV_CENTRED && call.method != MIFC_VDERIV_WEIGHTED)
    return refuse(c, a, "unknown method " + std::to_string(call.method));
  if (!a.fields || !a.coord || (a.hybrid() && (!a.alevel || !a.blevel)))
    return refuse(c, a, a.hybrid() ? "a null pointer (fields, ps, alevel or blevel)" : (by_level ? "a null pointer (fields or levels)" : "a null pointer (fields or coord)"));
  if (!call.fres && !call.fmag)
    return refuse(c, a, "fres and fmag are both null: nothing to write");
  if (call.fmag && (a.nfields & 1) != 0)
    return refuse(c, a, "fmag with an odd nfields: a magnitude takes the fields 2j and 2j + 1");
  if (call.fmag && !call.fdefined_mag)
    return refuse(c, a, "fmag without fdefined_mag");
  if (call.fres && !call.fdefined_out)
    return refuse(c, a, "fres without fdefined_out");
  const int nf = a.nfields, nm = call.fmag ? nf / 2 : 0, nlev = a.nlev;
  if (!check_field_pointers(c, a, call.fres))
    return 0;
  for (int j = 0; j < nm; ++j)
    if (!call.fmag[j])
      return refuse(c, a, "a null pointer (fmag[" + std::to_string(j) + "])");
  if (by_level)
    for (int k = 0; k < nlev; ++k)
      if (a.coord[k] != a.coord[k])
        return refuse(c, a, "levels[" + std::to_string(k) + "] is NaN");
  if (!check_levels(c, a))
    return 0;
  const size_t cells = a.cells(), batch = cells * (size_t)nlev * sizeof(float);
  const size_t n_out = call.fres ? (size_t)nf * (size_t)nlev : 0, n_mag = (size_t)nm * (size_t)nlev; // counters: one per output level
  if (!check_overlaps(c, a, {{call.fres, call.fres ? nf : 0, batch, "fres"}, {call.fmag, nm, batch, "fmag"}}))
    return 0;
  if (cells == 0) {
    std::fill_n(call.fdefined_out, n_out, MIFC_ALL_DEFINED); // checkDefined(0, 0)
    std::fill_n(call.fdefined_mag, n_mag, MIFC_ALL_DEFINED);
    return 1;
  }

  LevelTable tab; // the counters of the derivatives, then those of the magnitudes; `levels`: four weights per level in the tail
  if (!tab.build(c, a, (size_t)(nf + nm) * (size_t)nlev, by_level ? 4 * (size_t)nlev * sizeof(double) : 0))
    return 0;
  if (by_level)
    vderiv_level_weights(tab, a, call.method);
  Staging st(c, a.memkind); // blocks only: a host batch is staged band by band
  if (!tab.upload(c, st))
    return 0;
  BandPlan plan;
  PlaneGroup *in[mifc::VDERIV_MAX_FIELDS], *out[mifc::VDERIV_MAX_FIELDS], *mag[mifc::VDERIV_MAX_FIELDS / 2];
  for (int f = 0; f < nf; ++f)
    in[f] = plan.in(a.fields[f], (size_t)nlev);
  PlaneGroup* coord = plan.in(a.coord, a.coord_planes()); // (`levels`: no planes, null)
  for (int f = 0; f < nf; ++f)
    out[f] = plan.out(call.fres ? call.fres[f] : nullptr, (size_t)nlev);
  for (int j = 0; j < nm; ++j)
    mag[j] = plan.out(call.fmag[j], (size_t)nlev);
  if (!plan.place(c, st, a, (size_t)(mifc::env().vderiv_chunk_mib > 0 ? mifc::env().vderiv_chunk_mib : 256) << 20))
    return 0;

  mifc::VderivParams P;
  fill_params(P, a, tab, plan, coord);
  P.kind = a.kind;
  P.what = (call.fres ? mifc::VDERIV_DERIV : 0) | (call.fmag ? mifc::VDERIV_MAG : 0);
  P.method = call.method;
  P.n_undefined_mag = P.n_undefined + (size_t)nf * (size_t)nlev;
  P.lev_w = static_cast<const double*>(tab.dev_tail());

  // the launches of one problem of rows.n() columns: four fields each, two where both the derivatives and the magnitudes are
  // written (an even number: a vector stays in one launch)
  auto launch_passes = [&](const BandRows& rows) -> int {
    P.n = rows.n();
    const int pass = mifc::vderiv_pass_fields(P.what);
    for (int f0 = 0; f0 < nf; f0 += pass) {
      P.f0 = f0;
      P.nfields = std::min(pass, nf - f0);
      for (int f = 0; f < P.nfields; ++f) {
        P.fields[f] = in[f0 + f]->dev;
        P.out[f] = out[f0 + f]->dev;
      }
      for (int j = 0; j < P.nfields / 2; ++j)
        P.mag[j] = nm ? mag[f0 / 2 + j]->dev : nullptr;
      MIFC_LAUNCH(c, mifc::launch_vderiv(P, c->stream));
    }
    return 1;
  };
  if (!plan.run(c, a, launch_passes) || !tab.read_counts(c) || !st.finish()) // finish(): the one synchronisation of the call
    return 0;
  for (size_t j = 0; j < n_out; ++j)
    call.fdefined_out[j] = tab.classify(j, cells);
  for (size_t j = 0; j < n_mag; ++j)
    call.fdefined_mag[j] = tab.classify((size_t)nf * (size_t)nlev + j, cells);
  return 1;
}

} // namespace

extern "C" {

int mifc_vderiv_hlevels(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields, const float* ps,
                        int fdef_ps, const float* alevel, const float* blevel, int method, float* const* fres, int* fdefined_out,
                        float* const* fmag, int* fdefined_mag, float undef, int memkind)
{
  const Call a = {{"mifc_vderiv_hlevels", COORD_HYBRID, nx, ny, nlev, fields, fdefined_in, nfields, ps, fdef_ps, nullptr, alevel, blevel, undef, memkind},
                  method, fres, fdefined_out, fmag, fdefined_mag};
  return run(c, a);
}

int mifc_vderiv_fields(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields, const float* coord,
                       const int* fdef_coord, int method, float* const* fres, int* fdefined_out, float* const* fmag, int* fdefined_mag,
                       float undef, int memkind)
{
  const Call a = {{"mifc_vderiv_fields", COORD_FIELD, nx, ny, nlev, fields, fdefined_in, nfields, coord, MIFC_SOME_DEFINED, fdef_coord, nullptr,
                   nullptr, undef, memkind},
                  method, fres, fdefined_out, fmag, fdefined_mag};
  return run(c, a);
}

int mifc_vderiv_levels(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields, const float* levels,
                       int method, float* const* fres, int* fdefined_out, float* const* fmag, int* fdefined_mag, float undef, int memkind)
{
  const Call a = {{"mifc_vderiv_levels", COORD_LEVELS, nx, ny, nlev, fields, fdefined_in, nfields, levels, MIFC_SOME_DEFINED, nullptr, nullptr,
                   nullptr, undef, memkind},
                  method, fres, fdefined_out, fmag, fdefined_mag};
  return run(c, a);
}

} // extern "C"
