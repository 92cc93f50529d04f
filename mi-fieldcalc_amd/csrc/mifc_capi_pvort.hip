// mifc_capi_pvort.hip -- C ABI of mifc_pvort_hlevels / mifc_pvort_fields / mifc_pvort_levels (include/mifc.h;
// EXTENSION, no reference function) on the level-batch driver (mifc_levelbatch.h): the head of the call with the three
// fields u, v, th, its refusals, the level table with one counter per level and, for the `levels` form, the weights of
// mifc_vderiv_levels in its tail (vderiv_level_weights).  Device memory is used in place.  Host memory is staged band by
// band, but a band of rows is no complete problem here: the BandPlan is placed with a halo of one row, so a band carries
// the neighbour rows its rows need (rows 0 and ny - 1 those of rows 1 and ny - 2) and only the rows it owns are
// downloaded.  Every cell is computed by the same arithmetic whichever band it falls into, so the result does not depend
// on the bands.
#include "mifc_levelbatch.h"

#include <cstdio>

using namespace mifc_host;

static_assert(COORD_HYBRID == mifc::VDERIV_HYBRID && COORD_FIELD == mifc::VDERIV_FIELD && COORD_LEVELS == mifc::VDERIV_LEVELS, "PvortParams::kind");

namespace {

struct Call
{
  LevelBatchCall b;
  const float *xmapr, *ymapr, *fcoriolis;
  int method;
  double scale;
  float* fpv;
  int* fdefined_out;
};

// mifc_last_pvort_form: the shape of the calling thread's last call that launched
struct PvortForm
{
  int v = 0, kind = 0, weighted = 0, launches = 0, bands = 0;
};
thread_local PvortForm t_form;
thread_local char t_form_text[112];

int clamp_row(int y, int ny)
{
  return std::min(std::max(y, 1), ny - 2);
}

int run(mifc_ctx* c, const Call& call, const float* u, const float* v, const float* th)
{
  CTX_OR_FAIL(c);
  const float* const fields[3] = {u, v, th};
  LevelBatchCall a = call.b;
  a.fields = fields;
  a.nfields = 3;
  const bool by_level = a.kind == COORD_LEVELS;
  if (!check_counts(c, a, 3) || !check_grid(c, a))
    return 0;
  const int nx = a.nx, ny = a.ny, nlev = a.nlev;
  if (a.cells() != 0 && (nx < 3 || ny < 3))
    return refuse(c, a, "nx < 3 or ny < 3: a centred difference needs both neighbours");
  if (call.method != MIFC_VDERIV_CENTRED && call.method != MIFC_VDERIV_WEIGHTED)
    return refuse(c, a, "unknown method " + std::to_string(call.method));
  if (call.scale != call.scale)
    return refuse(c, a, "scale is NaN");
  if (!u || !v || !th || !a.coord || (a.hybrid() && (!a.alevel || !a.blevel)))
    return refuse(c, a, a.hybrid() ? "a null pointer (u, v, th, ps, alevel or blevel)" : (by_level ? "a null pointer (u, v, th or levels)" : "a null pointer (u, v, th or p)"));
  if (!call.xmapr || !call.ymapr)
    return refuse(c, a, "a null pointer (xmapr or ymapr)");
  if (!call.fpv || !call.fdefined_out)
    return refuse(c, a, "a null pointer (fpv or fdefined_out)");
  if (by_level)
    for (int k = 0; k < nlev; ++k)
      if (a.coord[k] != a.coord[k])
        return refuse(c, a, "levels[" + std::to_string(k) + "] is NaN");
  if (!check_levels(c, a))
    return 0;
  const size_t cells = a.cells(), plane = cells * sizeof(float), batch = plane * (size_t)nlev;
  float* const outs[1] = {call.fpv};
  if (!check_overlaps(c, a, {{outs, 1, batch, "fpv"}}, {{call.xmapr, plane, "xmapr"}, {call.ymapr, plane, "ymapr"}, {call.fcoriolis, plane, "fcoriolis"}}))
    return 0;
  if (cells == 0) {
    std::fill_n(call.fdefined_out, (size_t)nlev, MIFC_ALL_DEFINED); // checkDefined(0, 0)
    return 1;
  }

  LevelTable tab; // one counter per level; `levels`: the four weights of mifc_vderiv_levels per level in the tail
  if (!tab.build(c, a, (size_t)nlev, by_level ? 4 * (size_t)nlev * sizeof(double) : 0))
    return 0;
  if (by_level)
    vderiv_level_weights(tab, a, call.method);
  Staging st(c, a.memkind); // blocks only: a host batch is staged band by band
  if (!tab.upload(c, st))
    return 0;

  // u, v, th | the coordinate | xmapr, ymapr, fcoriolis | fpv; a band of host memory carries one neighbour row on each side
  BandPlan plan;
  PlaneGroup* const gu = plan.in(u, (size_t)nlev);
  PlaneGroup* const gv = plan.in(v, (size_t)nlev);
  PlaneGroup* const gth = plan.in(th, (size_t)nlev);
  PlaneGroup* const coord = plan.in(a.coord, a.coord_planes()); // (`levels`: no planes, null)
  PlaneGroup* const gxm = plan.in(call.xmapr, 1);
  PlaneGroup* const gym = plan.in(call.ymapr, 1);
  PlaneGroup* const gf = plan.in(call.fcoriolis, 1);
  PlaneGroup* const gout = plan.out(call.fpv, (size_t)nlev);
  if (!plan.place(c, st, a, (size_t)(mifc::env().pvort_chunk_mib > 0 ? mifc::env().pvort_chunk_mib : 256) << 20, 1))
    return 0;

  mifc::PvortParams P;
  std::memset(&P, 0, sizeof P);
  P.kind = a.kind;
  P.method = call.method;
  P.nx = nx;
  P.ny = ny;
  P.nlev = nlev;
  P.ps_all = a.fdef_ps == MIFC_ALL_DEFINED ? 1 : 0;
  P.undef = a.undef;
  P.scale = call.scale;
  P.ab = tab.ab();
  P.lev_bits = tab.lev_bits();
  P.lev_w = static_cast<const double*>(tab.dev_tail());
  P.n_undefined = tab.n_undefined();
  P.u = gu->dev;
  P.v = gv->dev;
  P.th = gth->dev;
  P.coord = coord->dev;
  P.xmapr = gxm->dev;
  P.ymapr = gym->dev;
  P.fcoriolis = gf->dev;
  P.out = gout->dev;
  P.stride = plan.stride;
  P.vec4 = plan.vec4 && (nx & 3) == 0 ? 1 : 0; // (whole rows on the 16-byte grid, which the plan does not ask for)

  // one launch over the rows of a problem: the interior rows among its own, and the ring rows beside them
  int launches = 0;
  auto launch = [&](const BandRows& rows) -> int {
    P.own0 = rows.own0;
    P.own1 = rows.own1;
    P.c0 = clamp_row(rows.own0, ny);
    P.c1 = clamp_row(rows.own1 - 1, ny);
    P.g0 = rows.first;
    P.rows = rows.staged;
    MIFC_LAUNCH(c, mifc::launch_pvort(P, c->stream));
    launches += 1;
    return 1;
  };
  if (!plan.run(c, a, launch))
    return 0;
  if (!tab.read_counts(c) || !st.finish()) // finish(): the one synchronisation of the call
    return 0;
  const size_t interior = (size_t)(nx - 2) * (size_t)(ny - 2);
  for (int k = 0; k < nlev; ++k)
    call.fdefined_out[k] = tab.classify((size_t)k, interior);
  t_form = {P.vec4 ? 4 : 1, a.kind, call.method == MIFC_VDERIV_WEIGHTED ? 1 : 0, launches, launches}; // (a band is one launch)
  return 1;
}

} // namespace

extern "C" {

int mifc_pvort_hlevels(mifc_ctx* c, int nx, int ny, int nlev, const float* u, const float* v, const float* th, const int* fdefined_in, const float* ps,
                       int fdef_ps, const float* alevel, const float* blevel, const float* xmapr, const float* ymapr, const float* fcoriolis, int method,
                       double scale, float* fpv, int* fdefined_out, float undef, int memkind)
{
  const Call a = {{"mifc_pvort_hlevels", COORD_HYBRID, nx, ny, nlev, nullptr, fdefined_in, 3, ps, fdef_ps, nullptr, alevel, blevel, undef, memkind},
                  xmapr, ymapr, fcoriolis, method, scale, fpv, fdefined_out};
  return run(c, a, u, v, th);
}

int mifc_pvort_fields(mifc_ctx* c, int nx, int ny, int nlev, const float* u, const float* v, const float* th, const int* fdefined_in, const float* p,
                      const int* fdef_coord, const float* xmapr, const float* ymapr, const float* fcoriolis, int method, double scale, float* fpv,
                      int* fdefined_out, float undef, int memkind)
{
  const Call a = {{"mifc_pvort_fields", COORD_FIELD, nx, ny, nlev, nullptr, fdefined_in, 3, p, MIFC_SOME_DEFINED, fdef_coord, nullptr, nullptr, undef, memkind},
                  xmapr, ymapr, fcoriolis, method, scale, fpv, fdefined_out};
  return run(c, a, u, v, th);
}

int mifc_pvort_levels(mifc_ctx* c, int nx, int ny, int nlev, const float* u, const float* v, const float* th, const int* fdefined_in, const float* levels,
                      const float* xmapr, const float* ymapr, const float* fcoriolis, int method, double scale, float* fpv, int* fdefined_out, float undef,
                      int memkind)
{
  const Call a = {{"mifc_pvort_levels", COORD_LEVELS, nx, ny, nlev, nullptr, fdefined_in, 3, levels, MIFC_SOME_DEFINED, nullptr, nullptr, nullptr, undef, memkind},
                  xmapr, ymapr, fcoriolis, method, scale, fpv, fdefined_out};
  return run(c, a, u, v, th);
}

const char* mifc_last_pvort_form(void)
{
  const PvortForm& f = t_form;
  if (f.launches == 0)
    return "";
  static const char* const KINDS[3] = {"hybrid", "field", "levels"};
  const int v = f.v;
  std::snprintf(t_form_text, sizeof t_form_text, "v=%d kind=%s method=%s tile=%dx%d launches=%d bands=%d", v, KINDS[f.kind], f.weighted ? "weighted" : "centred",
                mifc::PVORT_LANES_X * v, mifc::PVORT_TILE_ROWS, f.launches, f.bands);
  return t_form_text;
}

} // extern "C"
