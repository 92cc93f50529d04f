// mifc_capi_vinterp.hip -- C ABI of mifc_vinterp_hlevels / mifc_vinterp_fields (include/mifc.h; EXTENSION, no reference
// function) on the level-batch driver (mifc_levelbatch.h): its own refusals, the targets of a pass, up to 32 targets per
// launch of the kernel of mifc_vinterp.hip.
#include "mifc_levelbatch.h"

#include <cmath>
#include <cstring>

using namespace mifc_host;

namespace {

struct Call
{
  LevelBatchCall b;
  const float* targets;
  int ntargets, method;
  float* const* fres;
  int* fdefined_out;
};

int run(mifc_ctx* c, const Call& call)
{
  CTX_OR_FAIL(c);
  const LevelBatchCall& a = call.b;
  const int nf = a.nfields, nt = call.ntargets, nlev = a.nlev, method = call.method;
  if (!check_counts(c, a, mifc::VINTERP_MAX_FIELDS))
    return 0;
  if (nt < 1 || nt > mifc::VINTERP_MAX_TARGETS)
    return refuse(c, a, "ntargets " + std::to_string(nt) + " outside 1.." + std::to_string(mifc::VINTERP_MAX_TARGETS));
  if (!check_grid(c, a))
    return 0;
  if (method != MIFC_VINTERP_LINEAR && method != MIFC_VINTERP_LOG)
    return refuse(c, a, "unknown method " + std::to_string(method) + " (MIFC_VINTERP_LINEAR or MIFC_VINTERP_LOG)");
  if (!a.fields || !call.fres || !call.fdefined_out || !call.targets || !a.coord || (a.hybrid() && (!a.alevel || !a.blevel)))
    return refuse(c, a, a.hybrid() ? "a null pointer (fields, ps, alevel, blevel, targets, fres or fdefined_out)"
                                   : "a null pointer (fields, coord, targets, fres or fdefined_out)");
  if (!check_field_pointers(c, a, call.fres))
    return 0;
  for (int t = 0; t < nt; ++t) {
    if (call.targets[t] != call.targets[t])
      return refuse(c, a, "targets[" + std::to_string(t) + "] is NaN");
    if (method == MIFC_VINTERP_LOG && !(call.targets[t] > 0.f))
      return refuse(c, a, "MIFC_VINTERP_LOG with targets[" + std::to_string(t) + "] <= 0");
  }
  if (!check_levels(c, a))
    return 0;
  const size_t cells = a.cells(), n_counts = (size_t)nf * (size_t)nt;
  if (!check_overlaps(c, a, {{call.fres, nf, cells * (size_t)nt * sizeof(float), "fres"}}))
    return 0;
  if (cells == 0) {
    std::fill_n(call.fdefined_out, n_counts, MIFC_ALL_DEFINED); // checkDefined(0, 0)
    return 1;
  }

  LevelTable tab;
  Staging st(c, a.memkind); // blocks only: a host batch is staged band by band
  if (!tab.build(c, a, n_counts) || !tab.upload(c, st))
    return 0;
  BandPlan plan;
  PlaneGroup *in[mifc::VINTERP_MAX_FIELDS], *out[mifc::VINTERP_MAX_FIELDS];
  for (int f = 0; f < nf; ++f)
    in[f] = plan.in(a.fields[f], (size_t)nlev);
  PlaneGroup* coord = plan.in(a.coord, a.coord_planes());
  for (int f = 0; f < nf; ++f)
    out[f] = plan.out(call.fres[f], (size_t)nt);
  if (!plan.place(c, st, a, (size_t)(mifc::env().vinterp_chunk_mib > 0 ? mifc::env().vinterp_chunk_mib : 256) << 20))
    return 0;

  mifc::VinterpParams P;
  fill_params(P, a, tab, plan, coord);
  P.hybrid = a.hybrid() ? 1 : 0;
  P.method = method;
  P.nfields = nf;
  P.nt_call = nt;
  for (int f = 0; f < nf; ++f) {
    P.fields[f] = in[f]->dev;
    P.out[f] = out[f]->dev;
  }

  // the launches of one problem of rows.n() columns: 32 targets each
  auto launch_passes = [&](const BandRows& rows) -> int {
    P.n = rows.n();
    for (int t0 = 0; t0 < nt; t0 += mifc::VINTERP_PASS) {
      P.t0 = t0;
      P.nt = std::min(mifc::VINTERP_PASS, nt - t0);
      for (int t = 0; t < mifc::VINTERP_PASS; ++t) {
        const float ct = t < P.nt ? call.targets[t0 + t] : 1.f, ckey = ct + 0.f; // the key of -0 is that of +0 (the same target)
        int bits;
        std::memcpy(&bits, &ckey, sizeof bits);
        P.target[t] = ct;
        P.target_key[t] = mifc::vinterp_key(bits);
        P.target_log[t] = (method == MIFC_VINTERP_LOG && t < P.nt) ? std::log((double)ct) : 0.0;
      }
      MIFC_LAUNCH(c, mifc::launch_vinterp(P, c->stream));
    }
    return 1;
  };
  if (!plan.run(c, a, launch_passes) || !tab.read_counts(c) || !st.finish()) // finish(): the one synchronisation of the call
    return 0;
  for (size_t j = 0; j < n_counts; ++j)
    call.fdefined_out[j] = tab.classify(j, cells);
  return 1;
}

} // namespace

extern "C" {

int mifc_vinterp_hlevels(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields, const float* ps,
                         int fdef_ps, const float* alevel, const float* blevel, const float* targets, int ntargets, int method,
                         float* const* fres, int* fdefined_out, float undef, int memkind)
{
  const Call a = {{"mifc_vinterp_hlevels", COORD_HYBRID, nx, ny, nlev, fields, fdefined_in, nfields, ps, fdef_ps, nullptr, alevel, blevel, undef, memkind},
                  targets, ntargets, method, fres, fdefined_out};
  return run(c, a);
}

int mifc_vinterp_fields(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields, const float* coord,
                        const int* fdef_coord, const float* targets, int ntargets, int method, float* const* fres, int* fdefined_out,
                        float undef, int memkind)
{
  const Call a = {{"mifc_vinterp_fields", COORD_FIELD, nx, ny, nlev, fields, fdefined_in, nfields, coord, MIFC_SOME_DEFINED, fdef_coord, nullptr,
                   nullptr, undef, memkind},
                  targets, ntargets, method, fres, fdefined_out};
  return run(c, a);
}

} // extern "C"
