// mifc_capi_vregrid.hip -- C ABI of mifc_vregrid_hlevels / mifc_vregrid_fields / mifc_vregrid_levels (include/mifc.h;
// EXTENSION, no reference function) on the level-batch driver (mifc_levelbatch.h): its own refusals, the target planes as
// one more input group of the band, the form of the kernel of mifc_vregrid.hip (cells per lane, `tb` target planes per
// launch).  The `levels` form goes to the kernel as a hybrid coordinate whose alevel is `levels`, whose blevel is zero and
// whose ps is not read.
#include "mifc_levelbatch.h"

#include <cstdio>

using namespace mifc_host;

namespace {

struct Call
{
  LevelBatchCall b;
  const float* tcoord;
  const int* fdef_tcoord;
  int ntargets, method, from, outside;
  float* const* fres;
  int* fdefined_out;
};

// mifc_last_vregrid_form: the shape of the calling thread's last call that launched
struct VregridForm
{
  int v = 0, tb = 0, passes = 0, last = 0, clamp = 0, kind = 0, log = 0, launches = 0;
};
thread_local VregridForm t_form;
thread_local char t_form_text[128];

// the target planes of a pass: what the lane's slots in LDS and the bits of its found-mask allow, and of that (one cell
// per lane) the 24 that leave the LDS room for as many workgroups as the registers do
int pass_targets(int v)
{
  const int most = std::min(mifc::VREGRID_MAX_TB, mifc::VREGRID_MAX_LDS / (256 * v * (int)sizeof(float)));
  const int asked = mifc::env().vregrid_tb;
  return asked > 0 ? std::min(asked, most) : std::min(most, mifc::VREGRID_TB);
}

int run(mifc_ctx* c, const Call& call)
{
  CTX_OR_FAIL(c);
  const LevelBatchCall& a = call.b;
  const bool by_level = a.kind == COORD_LEVELS;
  const int nf = a.nfields, nt = call.ntargets, nlev = a.nlev;
  if (!check_counts(c, a, mifc::VREGRID_MAX_FIELDS))
    return 0;
  if (nt < 1 || nt > mifc::VREGRID_MAX_TARGETS)
    return refuse(c, a, "ntargets " + std::to_string(nt) + " outside 1.." + std::to_string(mifc::VREGRID_MAX_TARGETS));
  if (!check_grid(c, a))
    return 0;
  if (call.method != MIFC_VINTERP_LINEAR && call.method != MIFC_VINTERP_LOG)
    return refuse(c, a, "unknown method " + std::to_string(call.method) + " (MIFC_VINTERP_LINEAR or MIFC_VINTERP_LOG)");
  if (call.from != MIFC_VREGRID_FROM_FIRST && call.from != MIFC_VREGRID_FROM_LAST)
    return refuse(c, a, "unknown from " + std::to_string(call.from) + " (MIFC_VREGRID_FROM_FIRST or MIFC_VREGRID_FROM_LAST)");
  if (call.outside != MIFC_VREGRID_OUTSIDE_UNDEF && call.outside != MIFC_VREGRID_OUTSIDE_CLAMP)
    return refuse(c, a, "unknown outside " + std::to_string(call.outside) + " (MIFC_VREGRID_OUTSIDE_UNDEF or MIFC_VREGRID_OUTSIDE_CLAMP)");
  if (!a.fields || !call.fres || !call.fdefined_out || !call.tcoord || !a.coord || (a.hybrid() && (!a.alevel || !a.blevel)))
    return refuse(c, a, a.hybrid() ? "a null pointer (fields, ps, alevel, blevel, tcoord, fres or fdefined_out)"
                                   : (by_level ? "a null pointer (fields, levels, tcoord, fres or fdefined_out)"
                                               : "a null pointer (fields, coord, tcoord, fres or fdefined_out)"));
  if (!check_field_pointers(c, a, call.fres))
    return 0;
  if (by_level)
    for (int k = 0; k < nlev; ++k)
      if (a.coord[k] != a.coord[k])
        return refuse(c, a, "levels[" + std::to_string(k) + "] is NaN");
  if (!check_levels(c, a))
    return 0;
  const size_t cells = a.cells(), n_counts = (size_t)nf * (size_t)nt, tbytes = cells * (size_t)nt * sizeof(float);
  if (!check_overlaps(c, a, {{call.fres, nf, tbytes, "fres"}}, {{call.tcoord, tbytes, "tcoord"}}))
    return 0;
  if (cells == 0) {
    std::fill_n(call.fdefined_out, n_counts, MIFC_ALL_DEFINED); // checkDefined(0, 0)
    return 1;
  }

  // the table of the per-level scalars; `levels`: a hybrid table of (levels[k], 0)
  LevelTable tab;
  Staging st(c, a.memkind); // blocks only: a host batch is staged band by band
  LevelBatchCall as_table = a;
  std::vector<float> zeros;
  if (by_level) {
    try { // nothing may be thrown across the C ABI
      zeros.assign((size_t)nlev, 0.f);
    } catch (...) {
      c->err = "out of host memory";
      return 0;
    }
    as_table.kind = COORD_HYBRID;
    as_table.alevel = a.coord;
    as_table.blevel = zeros.data();
  }
  if (!tab.build(c, as_table, n_counts) || !tab.upload(c, st))
    return 0;
  BandPlan plan;
  PlaneGroup *in[mifc::VREGRID_MAX_FIELDS], *out[mifc::VREGRID_MAX_FIELDS];
  for (int f = 0; f < nf; ++f)
    in[f] = plan.in(a.fields[f], (size_t)nlev);
  PlaneGroup* coord = plan.in(a.coord, a.coord_planes()); // (`levels`: no planes, null)
  PlaneGroup* tcoord = plan.in(call.tcoord, (size_t)nt);
  for (int f = 0; f < nf; ++f)
    out[f] = plan.out(call.fres[f], (size_t)nt);
  if (!plan.place(c, st, a, (size_t)(mifc::env().vregrid_chunk_mib > 0 ? mifc::env().vregrid_chunk_mib : 256) << 20))
    return 0;

  mifc::VregridParams P;
  fill_params(P, a, tab, plan, coord);
  P.hybrid = a.kind == COORD_FIELD ? 0 : 1;
  P.no_ps = by_level ? 1 : 0;
  P.method = call.method;
  P.from = call.from;
  P.outside = call.outside;
  P.nfields = nf;
  P.nt_call = nt;
  P.tcoord = tcoord->dev;
  // The form (measured): one cell per lane.  Four cells per lane on the 16-byte grid -- more registers,
  // fewer waves, fewer targets per pass -- was slower in every case measured and runs where MIFC_VREGRID_V=4 asks for it.
  if (P.vec4 && mifc::env().vregrid_v != 4)
    P.vec4 = 0;
  P.tb = pass_targets(P.vec4 ? 4 : 1);
  for (int f = 0; f < nf; ++f) {
    P.fields[f] = in[f]->dev;
    P.out[f] = out[f]->dev;
  }

  // the launches of one problem of rows.n() columns: tb target planes each
  int launches = 0;
  auto launch_passes = [&](const BandRows& rows) -> int {
    P.n = rows.n();
    for (int t0 = 0; t0 < nt; t0 += P.tb) {
      P.t0 = t0;
      P.nt = std::min(P.tb, nt - t0);
      P.tc_all = 0;
      for (int t = 0; t < P.nt; ++t)
        if (call.fdef_tcoord && call.fdef_tcoord[t0 + t] == MIFC_ALL_DEFINED)
          P.tc_all |= 1u << t;
      MIFC_LAUNCH(c, mifc::launch_vregrid(P, c->stream));
      launches += 1;
    }
    return 1;
  };
  if (!plan.run(c, a, launch_passes) || !tab.read_counts(c) || !st.finish()) // finish(): the one synchronisation of the call
    return 0;
  for (size_t j = 0; j < n_counts; ++j)
    call.fdefined_out[j] = tab.classify(j, cells);
  t_form = {P.vec4 ? 4 : 1, P.tb, (nt + P.tb - 1) / P.tb, call.from == MIFC_VREGRID_FROM_LAST ? 1 : 0, call.outside == MIFC_VREGRID_OUTSIDE_CLAMP ? 1 : 0,
            a.kind, call.method == MIFC_VINTERP_LOG ? 1 : 0, launches};
  return 1;
}

} // namespace

extern "C" {

int mifc_vregrid_hlevels(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields, const float* ps,
                         int fdef_ps, const float* alevel, const float* blevel, const float* tcoord, const int* fdef_tcoord, int ntargets, int method,
                         int from, int outside, float* const* fres, int* fdefined_out, float undef, int memkind)
{
  const Call a = {{"mifc_vregrid_hlevels", COORD_HYBRID, nx, ny, nlev, fields, fdefined_in, nfields, ps, fdef_ps, nullptr, alevel, blevel, undef, memkind},
                  tcoord, fdef_tcoord, ntargets, method, from, outside, fres, fdefined_out};
  return run(c, a);
}

int mifc_vregrid_fields(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields, const float* coord,
                        const int* fdef_coord, const float* tcoord, const int* fdef_tcoord, int ntargets, int method, int from, int outside,
                        float* const* fres, int* fdefined_out, float undef, int memkind)
{
  const Call a = {{"mifc_vregrid_fields", COORD_FIELD, nx, ny, nlev, fields, fdefined_in, nfields, coord, MIFC_SOME_DEFINED, fdef_coord, nullptr,
                   nullptr, undef, memkind},
                  tcoord, fdef_tcoord, ntargets, method, from, outside, fres, fdefined_out};
  return run(c, a);
}

int mifc_vregrid_levels(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields, const float* levels,
                        const float* tcoord, const int* fdef_tcoord, int ntargets, int method, int from, int outside, float* const* fres,
                        int* fdefined_out, float undef, int memkind)
{
  const Call a = {{"mifc_vregrid_levels", COORD_LEVELS, nx, ny, nlev, fields, fdefined_in, nfields, levels, MIFC_SOME_DEFINED, nullptr, nullptr,
                   nullptr, undef, memkind},
                  tcoord, fdef_tcoord, ntargets, method, from, outside, fres, fdefined_out};
  return run(c, a);
}

const char* mifc_last_vregrid_form(void)
{
  const VregridForm& f = t_form;
  if (f.launches == 0)
    return "";
  std::snprintf(t_form_text, sizeof t_form_text, "v=%d tb=%d passes=%d from=%s outside=%s coord=%s method=%s launches=%d", f.v, f.tb, f.passes,
                f.last ? "last" : "first", f.clamp ? "clamp" : "undef", f.kind == COORD_HYBRID ? "hybrid" : (f.kind == COORD_FIELD ? "field" : "levels"),
                f.log ? "log" : "linear", f.launches);
  return t_form_text;
}

} // extern "C"
