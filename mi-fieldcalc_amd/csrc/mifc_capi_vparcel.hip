// mifc_capi_vparcel.hip -- C ABI of mifc_vparcel_hlevels / mifc_vparcel_fields / mifc_vparcel_levels (include/mifc.h;
// EXTENSION, no reference function) on the level-batch driver (mifc_levelbatch.h): its own refusals, for the `levels`
// form the pressure and pi_from_p of every level (computed here once per level with the host's powf, like the reference,
// in the tail of the device table), the source planes and the output planes as one-plane groups of the band, one launch
// of the kernel of mifc_vparcel.hip per band.
#include "mifc_levelbatch.h"

#include <cmath>
#include <cstdio>

using namespace mifc_host;

static_assert(COORD_HYBRID == mifc::VDERIV_HYBRID && COORD_FIELD == mifc::VDERIV_FIELD && COORD_LEVELS == mifc::VDERIV_LEVELS, "VparcelParams::kind");

namespace {

struct Call
{
  LevelBatchCall b;
  int from, src_level;
  const float* t_src;
  int fdef_tsrc;
  const float* q_src;
  int fdef_qsrc;
  const float* p_src;
  int fdef_psrc;
  float* planes[mifc::VPARCEL_PLANES]; // cape, cin, plcl, plfc, pel
  float* tparcel;
  int* fdefined_out;
};

// mifc_last_vparcel_form: the shape of the calling thread's last launch and the launches of its call
struct VparcelForm
{
  int v = 0, kind = 0, last = 0, src = 0, outputs = 0, launches = 0;
};
thread_local VparcelForm t_form;
thread_local char t_form_text[112];

const char* const PLANE_NAMES[mifc::VPARCEL_PLANES] = {"cape", "cin", "plcl", "plfc", "pel"};
const char* const KIND_NAMES[3] = {"hlevels", "fields", "levels"};

inline float pi_from_p(float p) // FieldCalculations.cc:308-316, host powf like the reference
{
  return K_CP * powf(p * K_P0INV, K_KAPPA);
}

int run(mifc_ctx* c, const float* t, const Call& call)
{
  CTX_OR_FAIL(c);
  const float* fields[1] = {t};
  LevelBatchCall a = call.b;
  a.fields = fields;
  a.nfields = 1;
  const bool by_level = a.kind == COORD_LEVELS;
  if (!check_counts(c, a, 1) || !check_grid(c, a))
    return 0;
  if (call.from != MIFC_VPARCEL_FROM_FIRST && call.from != MIFC_VPARCEL_FROM_LAST)
    return refuse(c, a, "unknown from " + std::to_string(call.from));
  const int nlev = a.nlev;
  if (call.src_level < -1 || call.src_level >= nlev)
    return refuse(c, a, "src_level " + std::to_string(call.src_level) + " outside -1.." + std::to_string(nlev - 1));
  if (!t || !a.coord || (a.hybrid() && (!a.alevel || !a.blevel)))
    return refuse(c, a, a.hybrid() ? "a null pointer (t, ps, alevel or blevel)" : (by_level ? "a null pointer (t or levels)" : "a null pointer (t or p)"));
  if (!call.q_src || (call.src_level < 0 && (!call.t_src || !call.p_src)))
    return refuse(c, a, call.src_level < 0 ? "a null pointer (t_src, q_src or p_src with src_level -1)" : "a null pointer (q_src)");
  bool any_out = call.tparcel != nullptr;
  for (int o = 0; o < mifc::VPARCEL_PLANES; ++o)
    any_out = any_out || call.planes[o] != nullptr;
  if (!any_out)
    return refuse(c, a, "no output (cape, cin, plcl, plfc, pel and tparcel are all null)");
  if (!call.fdefined_out)
    return refuse(c, a, "a null pointer (fdefined_out)");
  if (by_level)
    for (int k = 0; k < nlev; ++k) {
      if (a.coord[k] != a.coord[k])
        return refuse(c, a, "levels[" + std::to_string(k) + "] is NaN");
      if (!(a.coord[k] > 0.f))
        return refuse(c, a, "levels[" + std::to_string(k) + "] <= 0");
    }
  if (!check_levels(c, a))
    return 0;
  const size_t cells = a.cells(), plane = cells * sizeof(float), batch = plane * (size_t)nlev;
  const size_t n_out = (size_t)mifc::VPARCEL_PLANES + (size_t)nlev; // counters: the planes, then tparcel level by level
  // the source planes that the call reads (with a source level t_src and p_src are not looked at)
  const float* t_src = call.src_level < 0 ? call.t_src : nullptr;
  const float* p_src = call.src_level < 0 ? call.p_src : nullptr;
  {
    float* const tp[1] = {call.tparcel};
    auto one = [&](int o) { return Outputs{&call.planes[o], call.planes[o] ? 1 : 0, plane, PLANE_NAMES[o]}; };
    if (!check_overlaps(c, a, {one(0), one(1), one(2), one(3), one(4), {tp, call.tparcel ? 1 : 0, batch, "tparcel"}},
                        {{t_src, plane, "t_src"}, {call.q_src, plane, "q_src"}, {p_src, plane, "p_src"}}))
      return 0;
  }
  auto flag_of = [&](int counter) { return call.fdefined_out + counter; };
  if (cells == 0) {
    for (int o = 0; o < mifc::VPARCEL_PLANES; ++o)
      if (call.planes[o])
        *flag_of(o) = MIFC_ALL_DEFINED; // checkDefined(0, 0)
    if (call.tparcel)
      std::fill_n(flag_of(mifc::VPARCEL_PLANES), nlev, MIFC_ALL_DEFINED);
    return 1;
  }

  LevelTable tab; // `levels`: p and pi per level in the tail
  if (!tab.build(c, a, n_out, by_level ? (size_t)nlev * 2 * sizeof(float) : 0))
    return 0;
  if (by_level) {
    float* lp = static_cast<float*>(tab.tail());
    for (int k = 0; k < nlev; ++k) {
      lp[k] = a.coord[k];
      lp[nlev + k] = pi_from_p(a.coord[k]);
    }
  }
  Staging st(c, a.memkind); // blocks only: a host batch is staged band by band
  if (!tab.upload(c, st))
    return 0;
  BandPlan plan;
  PlaneGroup* in_t = plan.in(t, (size_t)nlev);
  PlaneGroup* coord = plan.in(a.coord, a.coord_planes()); // (`levels`: no planes, null)
  PlaneGroup* in_ts = plan.in(t_src, 1);
  PlaneGroup* in_qs = plan.in(call.q_src, 1);
  PlaneGroup* in_ps = plan.in(p_src, 1);
  PlaneGroup* out[mifc::VPARCEL_PLANES];
  for (int o = 0; o < mifc::VPARCEL_PLANES; ++o)
    out[o] = plan.out(call.planes[o], 1);
  PlaneGroup* out_tp = plan.out(call.tparcel, (size_t)nlev);
  if (!plan.place(c, st, a, (size_t)(mifc::env().vparcel_chunk_mib > 0 ? mifc::env().vparcel_chunk_mib : 256) << 20))
    return 0;

  mifc::VparcelParams P;
  fill_params(P, a, tab, plan, coord);
  P.kind = a.kind;
  P.from = call.from;
  P.src_level = call.src_level;
  P.t = in_t->dev;
  P.t_src = in_ts->dev;
  P.q_src = in_qs->dev;
  P.p_src = in_ps->dev;
  P.tsrc_all = call.fdef_tsrc == MIFC_ALL_DEFINED ? 1 : 0;
  P.qsrc_all = call.fdef_qsrc == MIFC_ALL_DEFINED ? 1 : 0;
  P.psrc_all = call.fdef_psrc == MIFC_ALL_DEFINED ? 1 : 0;
  int outputs = 0;
  for (int o = 0; o < mifc::VPARCEL_PLANES; ++o) {
    P.planes[o] = out[o]->dev;
    outputs += call.planes[o] ? 1 : 0;
  }
  P.tparcel = out_tp->dev;
  outputs += call.tparcel ? 1 : 0;
  P.lev_p = static_cast<const float*>(tab.dev_tail());

  int launches = 0;
  auto launch = [&](const BandRows& rows) -> int {
    P.n = rows.n();
    MIFC_LAUNCH(c, mifc::launch_vparcel(P, c->stream));
    launches += 1;
    return 1;
  };
  if (!plan.run(c, a, launch) || !tab.read_counts(c) || !st.finish()) // finish(): the one synchronisation of the call
    return 0;
  for (int o = 0; o < mifc::VPARCEL_PLANES; ++o)
    if (call.planes[o])
      *flag_of(o) = tab.classify((size_t)o, cells);
  if (call.tparcel)
    for (int k = 0; k < nlev; ++k)
      *flag_of(mifc::VPARCEL_PLANES + k) = tab.classify((size_t)(mifc::VPARCEL_PLANES + k), cells);
  t_form = {plan.vec4 ? 4 : 1, a.kind, call.from == MIFC_VPARCEL_FROM_LAST ? 1 : 0, call.src_level, outputs, launches};
  return 1;
}

Call make(const LevelBatchCall& b, int from, int src_level, const float* t_src, int fdef_tsrc, const float* q_src, int fdef_qsrc, const float* p_src,
          int fdef_psrc, float* cape, float* cin, float* plcl, float* plfc, float* pel, float* tparcel, int* fdefined_out)
{
  return {b, from, src_level, t_src, fdef_tsrc, q_src, fdef_qsrc, p_src, fdef_psrc, {cape, cin, plcl, plfc, pel}, tparcel, fdefined_out};
}

} // namespace

extern "C" {

int mifc_vparcel_hlevels(mifc_ctx* c, int nx, int ny, int nlev, const float* t, const int* fdefined_in, const float* ps, int fdef_ps,
                         const float* alevel, const float* blevel, int from, int src_level, const float* t_src, int fdef_tsrc, const float* q_src,
                         int fdef_qsrc, const float* p_src, int fdef_psrc, float* cape, float* cin, float* plcl, float* plfc, float* pel,
                         float* tparcel, int* fdefined_out, float undef, int memkind)
{
  return run(c, t,
             make({"mifc_vparcel_hlevels", COORD_HYBRID, nx, ny, nlev, nullptr, fdefined_in, 1, ps, fdef_ps, nullptr, alevel, blevel, undef, memkind}, from,
                  src_level, t_src, fdef_tsrc, q_src, fdef_qsrc, p_src, fdef_psrc, cape, cin, plcl, plfc, pel, tparcel, fdefined_out));
}

int mifc_vparcel_fields(mifc_ctx* c, int nx, int ny, int nlev, const float* t, const int* fdefined_in, const float* p, const int* fdef_coord, int from,
                        int src_level, const float* t_src, int fdef_tsrc, const float* q_src, int fdef_qsrc, const float* p_src, int fdef_psrc,
                        float* cape, float* cin, float* plcl, float* plfc, float* pel, float* tparcel, int* fdefined_out, float undef, int memkind)
{
  return run(c, t,
             make({"mifc_vparcel_fields", COORD_FIELD, nx, ny, nlev, nullptr, fdefined_in, 1, p, MIFC_SOME_DEFINED, fdef_coord, nullptr, nullptr, undef,
                   memkind},
                  from, src_level, t_src, fdef_tsrc, q_src, fdef_qsrc, p_src, fdef_psrc, cape, cin, plcl, plfc, pel, tparcel, fdefined_out));
}

int mifc_vparcel_levels(mifc_ctx* c, int nx, int ny, int nlev, const float* t, const int* fdefined_in, const float* levels, int from, int src_level,
                        const float* t_src, int fdef_tsrc, const float* q_src, int fdef_qsrc, const float* p_src, int fdef_psrc, float* cape,
                        float* cin, float* plcl, float* plfc, float* pel, float* tparcel, int* fdefined_out, float undef, int memkind)
{
  return run(c, t,
             make({"mifc_vparcel_levels", COORD_LEVELS, nx, ny, nlev, nullptr, fdefined_in, 1, levels, MIFC_SOME_DEFINED, nullptr, nullptr, nullptr, undef,
                   memkind},
                  from, src_level, t_src, fdef_tsrc, q_src, fdef_qsrc, p_src, fdef_psrc, cape, cin, plcl, plfc, pel, tparcel, fdefined_out));
}

const char* mifc_last_vparcel_form(void)
{
  const VparcelForm& f = t_form;
  if (f.launches == 0)
    return "";
  std::snprintf(t_form_text, sizeof t_form_text, "v=%d form=%s from=%s src=%d outputs=%d launches=%d", f.v, KIND_NAMES[f.kind], f.last ? "last" : "first",
                f.src, f.outputs, f.launches);
  return t_form_text;
}

} // extern "C"
