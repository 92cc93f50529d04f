// mifc_capi_pvort.hip -- C ABI of mifc_pvort_hlevels / mifc_pvort_fields / mifc_pvort_levels (include/mifc.h;
// EXTENSION, no reference function) on the level-batch driver (mifc_levelbatch.h): the head of the call with the three
// fields u, v, th, its refusals, the level table with one counter per level and, for the `levels` form, the weights of
// mifc_vderiv_levels in its tail.  Device memory is used in place.  Host memory is staged band by band, but a band of
// rows is no complete problem here: a band carries the neighbour rows its rows need (rows 0 and ny - 1 those of rows 1
// and ny - 2), only the rows it owns are downloaded.  That loop is this file's own (BandPlan knows no halo).  Every cell
// is computed by the same arithmetic whichever band it falls into, so the result does not depend on the bands.
#include "mifc_levelbatch.h"

#include <cstdint>
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
  if (by_level) {
    // rules 3 to 5 of mifc_vderiv_* for a coordinate that is the same in every cell of a level, as mifc_capi_vderiv.hip
    // has them: in double, every operation rounded on its own (this file is compiled without contraction like the kernels)
    double* w = static_cast<double*>(tab.tail());
    const float* lv = a.coord;
    for (int k = 0; k < nlev; ++k) {
      const bool lower = k > 0 && lv[k - 1] != lv[k], upper = k < nlev - 1 && lv[k + 1] != lv[k];
      const double d0 = (double)lv[k], dm = k > 0 ? (double)lv[k - 1] : 0.0, dp = k < nlev - 1 ? (double)lv[k + 1] : 0.0;
      const double h1 = d0 - dm, h2 = dp - d0;
      if (lower)
        w[4 * k] = 1.0 / h1;
      if (upper)
        w[4 * k + 1] = 1.0 / h2;
      bool fold = false;
      if (lower && upper) {
        if (call.method == MIFC_VDERIV_WEIGHTED) {
          const double s = h1 + h2;
          fold = s == 0.0;
          if (!fold) {
            const double p1 = h1 * s, p2 = h2 * s;
            w[4 * k + 2] = h2 / p1;
            w[4 * k + 3] = h1 / p2;
          }
        } else {
          const double dc = dp - dm;
          fold = dc == 0.0;
          if (!fold)
            w[4 * k + 2] = 1.0 / dc;
        }
      }
      tab.bits()[k] |= (lower ? 1u << mifc::VDERIV_LOWER_BIT : 0u) | (upper ? 1u << mifc::VDERIV_UPPER_BIT : 0u) |
                       (fold ? 1u << mifc::VDERIV_FOLD_BIT : 0u);
    }
  }
  Staging st(c, a.memkind); // blocks only: a host batch is staged band by band
  if (!tab.upload(c, st))
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

  int launches = 0, bands = 0;
  if (a.memkind != MIFC_MEM_HOST) {
    // the caller's planes: one launch over all rows
    uintptr_t all = reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(th) |
                    reinterpret_cast<uintptr_t>(call.xmapr) | reinterpret_cast<uintptr_t>(call.ymapr) | reinterpret_cast<uintptr_t>(call.fcoriolis) |
                    reinterpret_cast<uintptr_t>(call.fpv);
    if (!by_level)
      all |= reinterpret_cast<uintptr_t>(a.coord);
    P.u = u;
    P.v = v;
    P.th = th;
    P.coord = by_level ? nullptr : a.coord;
    P.xmapr = call.xmapr;
    P.ymapr = call.ymapr;
    P.fcoriolis = call.fcoriolis;
    P.out = call.fpv;
    P.stride = (long)cells;
    P.vec4 = ((nx & 3) == 0 && (all & 15) == 0) ? 1 : 0;
    P.g0 = 0;
    P.rows = ny;
    P.c0 = 1;
    P.c1 = ny - 2;
    P.own0 = 0;
    P.own1 = ny;
    MIFC_LAUNCH(c, mifc::launch_pvort(P, c->stream));
    launches = bands = 1;
  } else {
    // u, v, th | the coordinate | xmapr, ymapr, fcoriolis | fpv, one behind the other in one block; a band owns `own`
    // rows and is staged with the rows around them, `staged` at most
    const size_t coord_planes = a.coord_planes(), n_map = call.fcoriolis ? 3 : 2;
    const size_t planes = 4 * (size_t)nlev + coord_planes + n_map;
    const size_t budget = (size_t)(mifc::env().pvort_chunk_mib > 0 ? mifc::env().pvort_chunk_mib : 256) << 20;
    const size_t staged = std::min<size_t>((size_t)ny, std::max<size_t>(3, plan_band(budget, planes, (size_t)nx, (size_t)ny).rows));
    const size_t own = staged >= (size_t)ny ? (size_t)ny : staged - 2;
    const size_t S = align_up(staged * (size_t)nx, 64);
    float* d = static_cast<float*>(st.scratch(planes * S * sizeof(float)));
    if (!st.ok())
      return 0;
    struct Group
    {
      const float* host;
      float* dev;
      size_t planes;
    };
    Group in[7] = {{u, nullptr, (size_t)nlev}, {v, nullptr, (size_t)nlev}, {th, nullptr, (size_t)nlev}, {by_level ? nullptr : a.coord, nullptr, coord_planes},
                   {call.xmapr, nullptr, 1},   {call.ymapr, nullptr, 1},   {call.fcoriolis, nullptr, call.fcoriolis ? (size_t)1 : 0}};
    for (Group& g : in) {
      g.dev = g.planes ? d : nullptr;
      d += g.planes * S;
    }
    float* const dev_out = d;
    P.u = in[0].dev;
    P.v = in[1].dev;
    P.th = in[2].dev;
    P.coord = in[3].dev;
    P.xmapr = in[4].dev;
    P.ymapr = in[5].dev;
    P.fcoriolis = in[6].dev;
    P.out = dev_out;
    P.stride = (long)S;
    P.vec4 = (nx & 3) == 0 ? 1 : 0; // (the block and S are on the 16-byte grid)
    const size_t pitch = plane, dpitch = S * sizeof(float);
    for (size_t r0 = 0; r0 < (size_t)ny; r0 += own) {
      const int own0 = (int)r0, own1 = (int)std::min(r0 + own, (size_t)ny);
      P.own0 = own0;
      P.own1 = own1;
      P.c0 = clamp_row(own0, ny);
      P.c1 = clamp_row(own1 - 1, ny);
      P.g0 = P.c0 - 1;
      P.rows = P.c1 + 1 - P.g0 + 1;
      const size_t width = (size_t)P.rows * (size_t)nx * sizeof(float), off = (size_t)P.g0 * (size_t)nx;
      for (const Group& g : in)
        if (g.dev)
          MIFC_HIP(c, hipMemcpy2DAsync(g.dev, dpitch, g.host + off, pitch, width, g.planes, hipMemcpyHostToDevice, c->stream));
      MIFC_LAUNCH(c, mifc::launch_pvort(P, c->stream));
      const size_t mine = (size_t)own0 * (size_t)nx;
      MIFC_HIP(c, hipMemcpy2DAsync(call.fpv + mine, pitch, dev_out + (mine - off), dpitch, (size_t)(own1 - own0) * (size_t)nx * sizeof(float), (size_t)nlev,
                                   hipMemcpyDeviceToHost, c->stream));
      launches += 1;
      bands += 1;
    }
  }
  if (!tab.read_counts(c) || !st.finish()) // finish(): the one synchronisation of the call
    return 0;
  const size_t interior = (size_t)(nx - 2) * (size_t)(ny - 2);
  for (int k = 0; k < nlev; ++k)
    call.fdefined_out[k] = tab.classify((size_t)k, interior);
  t_form = {P.vec4 ? 4 : 1, a.kind, call.method == MIFC_VDERIV_WEIGHTED ? 1 : 0, launches, bands};
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
