// mifc_capi_vcumul.hip -- C ABI of mifc_vcumul_hlevels / mifc_vcumul_fields / mifc_vcumul_levels (include/mifc.h;
// EXTENSION, no reference function) on the level-batch driver (mifc_levelbatch.h): its own refusals, for the `levels`
// form g(levels[k]) (computed here once per level, in the tail of the device table), the start and the base planes as
// one-plane groups of the band, four fields per launch of the kernel of mifc_vcumul.hip.
#include "mifc_levelbatch.h"

#include <cmath>
#include <cstdio>

using namespace mifc_host;

static_assert(COORD_HYBRID == mifc::VDERIV_HYBRID && COORD_FIELD == mifc::VDERIV_FIELD && COORD_LEVELS == mifc::VDERIV_LEVELS, "VcumulParams::kind");

namespace {

struct Call
{
  LevelBatchCall b;
  int method, from;
  const float* start;
  int fdef_start;
  const float* const* base;
  const int* fdef_base;
  const double* scale;
  float* const* fres;
  int* fdefined_out;
};

// mifc_last_vcumul_form: the shape of the calling thread's last launch and the launches of its call
struct VcumulForm
{
  int v = 0, fields = 0, log = 0, last = 0, launches = 0;
};
thread_local VcumulForm t_form;
thread_local char t_form_text[96];

const char* const BASE_NAMES[mifc::VCUMUL_MAX_FIELDS] = {"base[0]", "base[1]", "base[2]", "base[3]", "base[4]", "base[5]", "base[6]", "base[7]"};

int run(mifc_ctx* c, const Call& call)
{
  CTX_OR_FAIL(c);
  const LevelBatchCall& a = call.b;
  const bool by_level = a.kind == COORD_LEVELS, by_log = call.method == MIFC_VCUMUL_LOG;
  if (!check_counts(c, a, mifc::VCUMUL_MAX_FIELDS) || !check_grid(c, a))
    return 0;
  if (call.method != MIFC_VCUMUL_LINEAR && call.method != MIFC_VCUMUL_LOG)
    return refuse(c, a, "unknown method " + std::to_string(call.method));
  if (call.from != MIFC_VCUMUL_FROM_FIRST && call.from != MIFC_VCUMUL_FROM_LAST)
    return refuse(c, a, "unknown from " + std::to_string(call.from));
  if (!a.fields || !a.coord || (a.hybrid() && (!a.alevel || !a.blevel)))
    return refuse(c, a, a.hybrid() ? "a null pointer (fields, ps, alevel or blevel)" : (by_level ? "a null pointer (fields or levels)" : "a null pointer (fields or coord)"));
  if (!call.fres || !call.fdefined_out)
    return refuse(c, a, "a null pointer (fres or fdefined_out)");
  const int nf = a.nfields, nlev = a.nlev;
  if (!check_field_pointers(c, a, call.fres))
    return 0;
  if (call.scale)
    for (int f = 0; f < nf; ++f)
      if (call.scale[f] != call.scale[f])
        return refuse(c, a, "scale[" + std::to_string(f) + "] is NaN");
  if (by_level)
    for (int k = 0; k < nlev; ++k) {
      if (a.coord[k] != a.coord[k])
        return refuse(c, a, "levels[" + std::to_string(k) + "] is NaN");
      if (by_log && !(a.coord[k] > 0.f))
        return refuse(c, a, "levels[" + std::to_string(k) + "] <= 0 with MIFC_VCUMUL_LOG");
    }
  if (!check_levels(c, a))
    return 0;
  const size_t cells = a.cells(), plane = cells * sizeof(float), batch = plane * (size_t)nlev;
  const size_t n_out = (size_t)nf * (size_t)nlev; // counters: one per output level
  const float* base[mifc::VCUMUL_MAX_FIELDS];
  for (int f = 0; f < mifc::VCUMUL_MAX_FIELDS; ++f)
    base[f] = call.base && f < nf ? call.base[f] : nullptr;
  if (!check_overlaps(c, a, {{call.fres, nf, batch, "fres"}},
                      {{call.start, plane, "start"},
                       {base[0], plane, BASE_NAMES[0]},
                       {base[1], plane, BASE_NAMES[1]},
                       {base[2], plane, BASE_NAMES[2]},
                       {base[3], plane, BASE_NAMES[3]},
                       {base[4], plane, BASE_NAMES[4]},
                       {base[5], plane, BASE_NAMES[5]},
                       {base[6], plane, BASE_NAMES[6]},
                       {base[7], plane, BASE_NAMES[7]}}))
    return 0;
  if (cells == 0) {
    std::fill_n(call.fdefined_out, n_out, MIFC_ALL_DEFINED); // checkDefined(0, 0)
    return 1;
  }

  LevelTable tab; // `levels`: g(levels[k]) per level in the tail
  if (!tab.build(c, a, n_out, by_level ? (size_t)nlev * sizeof(double) : 0))
    return 0;
  if (by_level) {
    double* g = static_cast<double*>(tab.tail());
    for (int k = 0; k < nlev; ++k)
      g[k] = by_log ? std::log((double)a.coord[k]) : (double)a.coord[k]; // rule 1
  }
  Staging st(c, a.memkind); // blocks only: a host batch is staged band by band
  if (!tab.upload(c, st))
    return 0;
  BandPlan plan;
  PlaneGroup *in[mifc::VCUMUL_MAX_FIELDS], *out[mifc::VCUMUL_MAX_FIELDS], *bases[mifc::VCUMUL_MAX_FIELDS];
  for (int f = 0; f < nf; ++f)
    in[f] = plan.in(a.fields[f], (size_t)nlev);
  PlaneGroup* coord = plan.in(a.coord, a.coord_planes()); // (`levels`: no planes, null)
  PlaneGroup* start = plan.in(call.start, 1);
  for (int f = 0; f < nf; ++f)
    bases[f] = plan.in(base[f], 1);
  for (int f = 0; f < nf; ++f)
    out[f] = plan.out(call.fres[f], (size_t)nlev);
  if (!plan.place(c, st, a, (size_t)(mifc::env().vcumul_chunk_mib > 0 ? mifc::env().vcumul_chunk_mib : 256) << 20))
    return 0;

  mifc::VcumulParams P;
  fill_params(P, a, tab, plan, coord);
  P.kind = a.kind;
  P.method = call.method;
  P.from = call.from;
  P.start = start->dev;
  P.start_all = call.fdef_start == MIFC_ALL_DEFINED ? 1 : 0;
  P.lev_g = static_cast<const double*>(tab.dev_tail());

  // the launches of one problem of rows.n() columns: four fields each
  int launches = 0;
  auto launch_passes = [&](const BandRows& rows) -> int {
    P.n = rows.n();
    for (int f0 = 0; f0 < nf; f0 += mifc::VCUMUL_PASS) {
      P.f0 = f0;
      P.nfields = std::min(mifc::VCUMUL_PASS, nf - f0);
      P.base_all = 0;
      for (int f = 0; f < P.nfields; ++f) {
        P.fields[f] = in[f0 + f]->dev;
        P.out[f] = out[f0 + f]->dev;
        P.base[f] = bases[f0 + f]->dev;
        P.scale[f] = call.scale ? call.scale[f0 + f] : 1.0;
        if (call.fdef_base && call.fdef_base[f0 + f] == MIFC_ALL_DEFINED)
          P.base_all |= 1 << f;
      }
      MIFC_LAUNCH(c, mifc::launch_vcumul(P, c->stream));
      launches += 1;
    }
    return 1;
  };
  if (!plan.run(c, a, launch_passes) || !tab.read_counts(c) || !st.finish()) // finish(): the one synchronisation of the call
    return 0;
  for (size_t j = 0; j < n_out; ++j)
    call.fdefined_out[j] = tab.classify(j, cells);
  t_form = {plan.vec4 ? 4 : 1, std::min(mifc::VCUMUL_PASS, nf), by_log ? 1 : 0, call.from == MIFC_VCUMUL_FROM_LAST ? 1 : 0, launches};
  return 1;
}

Call make(const LevelBatchCall& b, int method, int from, const float* start, int fdef_start, const float* const* base, const int* fdef_base,
          const double* scale, float* const* fres, int* fdefined_out)
{
  return {b, method, from, start, fdef_start, base, fdef_base, scale, fres, fdefined_out};
}

} // namespace

extern "C" {

int mifc_vcumul_hlevels(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields, const float* ps,
                        int fdef_ps, const float* alevel, const float* blevel, int method, int from, const float* start, int fdef_start,
                        const float* const* base, const int* fdef_base, const double* scale, float* const* fres, int* fdefined_out, float undef,
                        int memkind)
{
  return run(c, make({"mifc_vcumul_hlevels", COORD_HYBRID, nx, ny, nlev, fields, fdefined_in, nfields, ps, fdef_ps, nullptr, alevel, blevel, undef, memkind},
                     method, from, start, fdef_start, base, fdef_base, scale, fres, fdefined_out));
}

int mifc_vcumul_fields(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields, const float* coord,
                       const int* fdef_coord, int method, int from, const float* start, int fdef_start, const float* const* base,
                       const int* fdef_base, const double* scale, float* const* fres, int* fdefined_out, float undef, int memkind)
{
  return run(c, make({"mifc_vcumul_fields", COORD_FIELD, nx, ny, nlev, fields, fdefined_in, nfields, coord, MIFC_SOME_DEFINED, fdef_coord, nullptr,
                      nullptr, undef, memkind},
                     method, from, start, fdef_start, base, fdef_base, scale, fres, fdefined_out));
}

int mifc_vcumul_levels(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields, const float* levels,
                       int method, int from, const float* start, int fdef_start, const float* const* base, const int* fdef_base,
                       const double* scale, float* const* fres, int* fdefined_out, float undef, int memkind)
{
  return run(c, make({"mifc_vcumul_levels", COORD_LEVELS, nx, ny, nlev, fields, fdefined_in, nfields, levels, MIFC_SOME_DEFINED, nullptr, nullptr,
                      nullptr, undef, memkind},
                     method, from, start, fdef_start, base, fdef_base, scale, fres, fdefined_out));
}

const char* mifc_last_vcumul_form(void)
{
  const VcumulForm& f = t_form;
  if (f.launches == 0)
    return "";
  std::snprintf(t_form_text, sizeof t_form_text, "v=%d fields=%d method=%s from=%s launches=%d", f.v, f.fields, f.log ? "log" : "linear",
                f.last ? "last" : "first", f.launches);
  return t_form_text;
}

} // extern "C"
