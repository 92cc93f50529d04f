// mifc_capi_twostage.hip -- the host side of the two-stage operators (thermalFrontParameter, plevelqvector: mifc_fused2.hip,
// or pass by pass through run_stencil()) and of the second-order Shapiro filter (mifc_shapiro.hip): the single-field entries
// and their branches of mifc_stencil_levels_ex on ONE driver per operator pair.  A driver works on device pointers and on
// nlev >= 1 levels nx * ny floats apart; a single field is a batch of one.  Each driver decides its route once and notes it
// (mifc_last_stencil_form) as its last act:
//   two_stage_levels()   fused2 | fused2_redo | two_stage_passes
//   shapiro_levels()     shapiro_fused | shapiro_sweeps

#include <cmath>
#include <cstring>
#include <vector>

#include "mifc_stencil_host.h"

using namespace mifc_host;

namespace {

// grid.y of one launch.  The launchers of the two-stage kernel, of the stencil passes and of the filter's sweeps split a deeper
// batch themselves; the filter's one-launch form does not, so its driver runs in slices.
const int kMaxLaunchLevels = 65535;

int noted(const char* form, int rc)
{
  mifc::note_form(form);
  return rc;
}

// The levels of a batch in two groups, the ones whose input flag is ALL_DEFINED (no tests) first.  The kernels take a
// group's levels from a list on the device (c->d_levels) -- or, with a null list, in order: so a batch whose levels all
// fall into one group, a single field among them, sends none.  The object has to outlive the synchronisation behind the
// launches: the copy of the list may read its host side until then.
struct FlagGroups
{
  int n_all = 0;             // levels of the first group
  const int* list = nullptr; // c->d_levels, or null: one group, every level in order
  std::vector<int> order;    // host side of the list
};

int flag_groups(mifc_ctx* c, const int* fdefined, int nlev, FlagGroups* g)
{
  for (int l = 0; l < nlev; ++l)
    g->n_all += fdefined[l] == MIFC_ALL_DEFINED;
  if (g->n_all == 0 || g->n_all == nlev)
    return 1;
  if (!ensure_levels(c, (size_t)nlev))
    return 0;
  g->order.resize(nlev);
  int a = 0, t = g->n_all;
  for (int l = 0; l < nlev; ++l)
    g->order[fdefined[l] == MIFC_ALL_DEFINED ? a++ : t++] = l;
  MIFC_HIP(c, hipMemcpyAsync(c->d_levels, g->order.data(), sizeof(int) * (size_t)nlev, hipMemcpyHostToDevice, c->stream));
  g->list = c->d_levels;
  return 1;
}

// ---- thermalFrontParameter and plevelqvector ---------------------------------------------------------------------------

// One request of either operator on device pointers: the kernel's own description of the fields (F.a = tx | z; F.t,
// F.fcoriolis: Q-vector only; levels F.level_stride = nx * ny floats apart) plus the depth of the batch and, for the
// Q-vector, its two scalars as host tables with one entry per level.
struct TwoStage
{
  mifc::Fused2Params F;
  int nlev;
  const float *tscale, *cscale;
};

TwoStage two_stage(int op, int nx, int ny, int nlev, float undef)
{
  TwoStage q;
  std::memset(&q, 0, sizeof q);
  q.F.op = op;
  q.F.nx = nx;
  q.F.ny = ny;
  q.F.level_stride = (long)nx * ny;
  q.F.undef = undef;
  q.nlev = nlev;
  return q;
}

// plevelqvector's two scalars of a pressure level (:526-540, :564); false where the reference returns false
bool qvector_scales(float p, int compute, float* tscale, float* cscale)
{
  if (compute == 1 || compute == 3)
    *tscale = 1.0f;
  else if (compute == 2 || compute == 4)
    *tscale = K_CP * powf(p / 1000.0f, 287.f / K_CP) / K_CP; // :539, host powf like the reference
  else
    return false;
  *cscale = (float)((double)(-287.f) / ((double)p * 100.)); // :564
  return true;
}

// thermalFrontParameter pass by pass (:2266-2309), each pass ONE launch over the levels: |grad T| into a scratch batch, then
// the front parameter; the second pass takes every level's "all defined" from the flag the first returned for it (:2286).
int tfp_two_passes(mifc_ctx* c, const TwoStage& q, int* fdefined)
{
  const mifc::Fused2Params& F = q.F;
  Staging st(c, MIFC_MEM_DEVICE);
  float* d_absdelt = static_cast<float*>(st.scratch((size_t)F.level_stride * (size_t)q.nlev * sizeof(float)));
  if (!st.ok())
    return 0;
  const StencilCall pass1 = {mifc::ST_GRAD_ABS, F.nx, F.ny, q.nlev, F.a, nullptr, F.xmapr, F.ymapr, nullptr, d_absdelt, nullptr};
  if (!run_stencil(c, pass1, fdefined, F.undef, MIFC_MEM_DEVICE))
    return 0;
  const StencilCall pass2 = {mifc::ST_TFP, F.nx, F.ny, q.nlev, F.a, d_absdelt, F.xmapr, F.ymapr, nullptr, F.out, nullptr};
  return run_stencil(c, pass2, fdefined, F.undef, MIFC_MEM_DEVICE);
}

// The three passes of plevelqvector (:555-590), each ONE launch over the levels: geostrophic wind x and y into scratch
// batches, then the Q-vector component.  The flags thread through the passes like the reference's fDefined: the x pass
// leaves NONE_DEFINED (:664), so the y pass always tests; the last pass tests whatever it is handed.
int qvector_three_passes(mifc_ctx* c, const TwoStage& q, int* fdefined)
{
  const mifc::Fused2Params& F = q.F;
  const size_t nb = (size_t)F.level_stride * (size_t)q.nlev;
  Staging st(c, MIFC_MEM_DEVICE);
  float* d_ug = static_cast<float*>(st.scratch(nb * sizeof(float)));
  float* d_vg = static_cast<float*>(st.scratch(nb * sizeof(float)));
  if (!st.ok())
    return 0;
  const StencilCall pass1 = {mifc::ST_GWIND_X, F.nx, F.ny, q.nlev, F.a, nullptr, F.xmapr, F.ymapr, F.fcoriolis, d_ug, nullptr};
  if (!run_stencil(c, pass1, fdefined, F.undef, MIFC_MEM_DEVICE))
    return 0;
  const StencilCall pass2 = {mifc::ST_GWIND_Y, F.nx, F.ny, q.nlev, F.a, nullptr, F.xmapr, F.ymapr, F.fcoriolis, d_vg, nullptr};
  if (!run_stencil(c, pass2, fdefined, F.undef, MIFC_MEM_DEVICE))
    return 0;
  StencilCall pass3 = {F.op == mifc::F2_QVEC_X ? mifc::ST_QVEC_X : mifc::ST_QVEC_Y, F.nx, F.ny, q.nlev, d_ug, d_vg, F.xmapr, F.ymapr, nullptr, F.out, nullptr};
  pass3.f2 = F.t;
  pass3.scale = F.scale;
  pass3.scale2 = F.scale2;
  pass3.scale_lev = F.scale_lev;
  pass3.scale2_lev = F.scale2_lev;
  return run_stencil(c, pass3, fdefined, F.undef, MIFC_MEM_DEVICE);
}

// The driver.  One launch per flag group (of at most 65 535 levels each: launch_fused2 splits) with the intermediate fields
// in LDS where the kernel takes the grid (fused2_supported; MIFC_FUSED2=0: never -- A/B measurements, tests), else the
// passes over all levels at once.
int two_stage_levels(mifc_ctx* c, TwoStage q, int* fdefined)
{
  mifc::Fused2Params& F = q.F;
  const bool tfp = F.op == mifc::F2_TFP;
  const int nlev = q.nlev;
  if (!ensure_levels(c, (size_t)nlev))
    return 0;
  F.counts = c->d_counts; // three per level: 3 * nlev <= 5 * cap_lev after ensure_levels()
  // the Q-vector's scalars depend on the level's pressure: one level carries them in the parameters, a batch in tables on
  // the device, indexed by level whatever the order of the launches (every route synchronises before it returns, so the
  // host tables outlive the copies)
  if (!tfp) {
    F.scale = q.tscale[0];
    F.scale2 = q.cscale[0];
  }
  if (!tfp && nlev > 1) {
    MIFC_HIP(c, hipMemcpyAsync(c->d_ab, q.tscale, sizeof(float) * (size_t)nlev, hipMemcpyHostToDevice, c->stream));
    MIFC_HIP(c, hipMemcpyAsync(c->d_ab + c->cap_lev, q.cscale, sizeof(float) * (size_t)nlev, hipMemcpyHostToDevice, c->stream));
    F.scale_lev = c->d_ab;
    F.scale2_lev = c->d_ab + c->cap_lev;
  }
  if (!mifc::env().fused2 || !mifc::fused2_supported(F))
    return noted("two_stage_passes", tfp ? tfp_two_passes(c, q, fdefined) : qvector_three_passes(c, q, fdefined));

  FlagGroups g;
  if (!pinned_acquire(c) || !flag_groups(c, fdefined, nlev, &g)) // the counts come back through the pinned mirror
    return 0;
  MIFC_HIP(c, hipMemsetAsync(c->d_counts, 0, 3 * sizeof(u64) * (size_t)nlev, c->stream));
  for (int group = 0; group < 2; ++group) {
    const int first = group == 0 ? 0 : g.n_all, count = group == 0 ? g.n_all : nlev - g.n_all;
    if (count == 0)
      continue;
    F.check = group;
    F.n_launch_levels = count;
    F.levels = g.list ? g.list + first : nullptr;
    MIFC_LAUNCH(c, mifc::launch_fused2(F, c->stream));
  }
  MIFC_HIP(c, hipMemcpyAsync(pinned_counts(c), c->d_counts, 3 * sizeof(u64) * (size_t)nlev, hipMemcpyDeviceToHost, c->stream));
  MIFC_HIP(c, hipStreamSynchronize(c->stream));
  // thermalFrontParameter's second pass tests its inputs only if the first pass left something undefined (:2286).  The
  // kernel ran it tested; where the first pass turned out clean AND the test rejected a cell the untested loop would have
  // computed (a NaN gradient from defined inputs), the result differs: those levels go again, pass by pass, each with its
  // own flag.  (The passes reuse the mirror, so every level is classified before the first repair.)
  std::vector<int> redo;
  for (int l = 0; l < nlev; ++l) {
    const u64* k = pinned_counts(c) + 3 * (size_t)l;
    if (tfp && fdefined[l] != MIFC_ALL_DEFINED && k[0] == 0 && k[2] != 0)
      redo.push_back(l);
    else
      fdefined[l] = mifc_classify(k[1], (u64)F.level_stride - 2 * (u64)F.nx); // :2303, :590
  }
  for (int l : redo) {
    TwoStage one = q;
    one.nlev = 1;
    one.F.a += (size_t)l * (size_t)F.level_stride;
    one.F.out += (size_t)l * (size_t)F.level_stride;
    if (!tfp_two_passes(c, one, fdefined + l))
      return 0;
  }
  return noted(redo.empty() ? "fused2" : "fused2_redo", 1);
}

// ---- shapiro2_filter (FieldCalculations.cc:2076-2179) ------------------------------------------------------------------

// The driver: the four sweeps of every level in one launch per flag group (src -> dst, two different arrays) where the
// kernel takes the grid, else the masks and the sweeps as launches over the levels of each group, in place on the output
// like the reference (:2099-2104).  d_in == d_out is allowed (:2088): the one-launch route then goes through a scratch
// batch and is copied back, the sweeps run in place anyway.  Scratch comes from the caller's staging, whose finish() is the
// synchronisation, as does g.  The flags are read, not written.
int shapiro_levels(mifc_ctx* c, Staging& st, FlagGroups& g, int nx, int ny, int nlev, const float* d_in, float* d_out, const int* fdefined, float undef)
{
  const size_t n = (size_t)nx * ny, nb = n * (size_t)nlev;
  float* tmp = nullptr; // the one-launch route's destination of an in-place call, the sweeps' second field
  if (d_out == d_in && !(tmp = static_cast<float*>(st.scratch(nb * sizeof(float)))))
    return 0;
  float* dst = tmp ? tmp : d_out;
  // (no clause for the level stride: the tile form takes multiples of four columns only, so its levels stay 16-byte aligned;
  // the register form takes any alignment)
  const bool fused = mifc::env().shapiro_fused && mifc::shapiro2_fused_supported(nx, ny, d_in, dst); // MIFC_SHAPIRO_FUSED=0: the sweeps
  if (!fused && n > 0x7fffffffu) // the sweep kernels index a level with an int
    return 0;
  if (!flag_groups(c, fdefined, nlev, &g))
    return 0;
  const int n_tested = nlev - g.n_all;
  if (fused) {
    if (g.n_all > 0)
      MIFC_LAUNCH(c, mifc::launch_shapiro2_fused_levels(nx, ny, 1, undef, d_in, dst, g.n_all, (long)n, g.list, c->stream));
    if (n_tested > 0)
      MIFC_LAUNCH(c, mifc::launch_shapiro2_fused_levels(nx, ny, 0, undef, d_in, dst, n_tested, (long)n, g.list ? g.list + g.n_all : nullptr, c->stream));
    if (dst != d_out)
      MIFC_HIP(c, hipMemcpyAsync(d_out, dst, nb * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    return noted("shapiro_fused", 1);
  }
  if (!tmp)
    tmp = static_cast<float*>(st.scratch(nb * sizeof(float)));
  unsigned char* masks = n_tested > 0 ? static_cast<unsigned char*>(st.scratch(2 * nb)) : nullptr;
  if (!st.ok())
    return 0;
  if (d_out != d_in)
    MIFC_HIP(c, hipMemcpyAsync(d_out, d_in, nb * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
  mifc::ShapiroParams P;
  P.nx = nx;
  P.ny = ny;
  P.undef = undef;
  P.f1 = d_out;
  P.f2 = tmp;
  P.mask_x = masks;
  P.mask_y = masks ? masks + nb : nullptr;
  if (g.n_all > 0) {
    P.all_defined = 1;
    MIFC_LAUNCH(c, mifc::launch_shapiro2_levels(P, g.n_all, g.list, c->stream));
  }
  if (n_tested > 0) {
    P.all_defined = 0;
    MIFC_LAUNCH(c, mifc::launch_shapiro2_levels(P, n_tested, g.list ? g.list + g.n_all : nullptr, c->stream));
  }
  return noted("shapiro_sweeps", 1);
}

// a staged batch of any depth through the driver, the outputs home, every flag ALL_DEFINED (:2171)
int shapiro_run(mifc_ctx* c, Staging& st, int nx, int ny, int nlev, const float* d_in, float* d_out, int* fdefined, float undef)
{
  const size_t n = (size_t)nx * ny;
  FlagGroups g; // stays until finish() has synchronised; a slice behind another waits for it first
  for (int l0 = 0; l0 < nlev; l0 += kMaxLaunchLevels) {
    const int nl = nlev - l0 < kMaxLaunchLevels ? nlev - l0 : kMaxLaunchLevels;
    if (l0 > 0)
      MIFC_HIP(c, hipStreamSynchronize(c->stream));
    g = FlagGroups();
    if (!shapiro_levels(c, st, g, nx, ny, nl, d_in + (size_t)l0 * n, d_out + (size_t)l0 * n, fdefined + l0, undef))
      return 0;
  }
  if (!st.finish())
    return 0;
  for (int l = 0; l < nlev; ++l)
    fdefined[l] = MIFC_ALL_DEFINED;
  return 1;
}

} // namespace

namespace mifc_host {

// the thermalFrontParameter, plevelqvector and shapiro2_filter branches of mifc_stencil_levels_ex, which has checked
// nx, ny >= 3, nlev >= 1 and f0, out0, fdefined
int two_stage_levels_ex(mifc_ctx* c, int op, int nx, int ny, int nlev, const float* f0, const float* f1, const float* xmapr, const float* ymapr,
                        const float* fcoriolis, const float* level_scalars, int compute, float* out0, int* fdefined, float undef, int memkind)
{
  const size_t n = (size_t)nx * ny, nb = n * (size_t)nlev;
  std::vector<float> tscale, cscale;
  if (op == MIFC_OP_QVECTOR) { // :526-540, per level like the single-field call
    if (!f1 || !fcoriolis || !level_scalars)
      return 0;
    tscale.resize(nlev);
    cscale.resize(nlev);
    for (int l = 0; l < nlev; ++l) {
      if (level_scalars[l] <= 0.0 || !qvector_scales(level_scalars[l], compute, &tscale[l], &cscale[l]))
        return 0;
    }
  }
  Staging st(c, memkind);
  const float* d0 = st.in(f0, nb);
  if (op == MIFC_OP_SHAPIRO2) {
    float* dout = st.out(out0, nb);
    return st.ok() && shapiro_run(c, st, nx, ny, nlev, d0, dout, fdefined, undef);
  }
  TwoStage q = two_stage((op == MIFC_OP_TFP) ? mifc::F2_TFP : (compute < 3 ? mifc::F2_QVEC_X : mifc::F2_QVEC_Y), nx, ny, nlev, undef);
  q.F.a = d0;
  if (op == MIFC_OP_QVECTOR) {
    q.F.t = st.in(f1, nb);
    q.tscale = tscale.data();
    q.cscale = cscale.data();
  }
  q.F.xmapr = st.in(xmapr, n);
  q.F.ymapr = st.in(ymapr, n);
  if (op == MIFC_OP_QVECTOR)
    q.F.fcoriolis = st.in(fcoriolis, n);
  q.F.out = st.out(out0, nb);
  if (!st.ok() || !q.F.xmapr || !q.F.ymapr)
    return 0;
  return two_stage_levels(c, q, fdefined) && st.finish();
}

} // namespace mifc_host

extern "C" {

// thermalFrontParameter, FieldCalculations.cc:2266-2309
int mifc_thermalFrontParameter(mifc_ctx* c, int nx, int ny, const float* tx, const float* xmapr, const float* ymapr, float* tfp, int* fdefined,
                               float undef, int memkind)
{
  CTX_OR_FAIL(c);
  if (nx < 3 || ny < 3) // gradient() :2004
    return 0;
  const size_t n = (size_t)nx * ny;
  Staging st(c, memkind);
  TwoStage q = two_stage(mifc::F2_TFP, nx, ny, 1, undef);
  q.F.a = st.in(tx, n);
  q.F.xmapr = st.in(xmapr, n);
  q.F.ymapr = st.in(ymapr, n);
  q.F.out = st.out(tfp, n);
  return st.ok() && two_stage_levels(c, q, fdefined) && st.finish();
}

// plevelqvector, FieldCalculations.cc:505-595
int mifc_plevelqvector(mifc_ctx* c, int nx, int ny, const float* z, const float* t, const float* xmapr, const float* ymapr, const float* fcoriolis,
                       float p, int compute, float* qcomp, int* fdefined, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  if (p <= 0.0 || nx < 3 || ny < 3) // :526-530
    return 0;
  float tscale, cscale;
  if (!qvector_scales(p, compute, &tscale, &cscale))
    return 0;
  const size_t n = (size_t)nx * ny;
  Staging st(c, memkind);
  TwoStage q = two_stage(compute < 3 ? mifc::F2_QVEC_X : mifc::F2_QVEC_Y, nx, ny, 1, undef);
  q.tscale = &tscale;
  q.cscale = &cscale;
  q.F.a = st.in(z, n);
  q.F.t = st.in(t, n);
  q.F.xmapr = st.in(xmapr, n);
  q.F.ymapr = st.in(ymapr, n);
  q.F.fcoriolis = st.in(fcoriolis, n);
  q.F.out = st.out(qcomp, n);
  return st.ok() && two_stage_levels(c, q, fdefined) && st.finish();
}

// shapiro2_filter, FieldCalculations.cc:2076-2179: `field` and `fsmooth` may be the same array; the flag always becomes
// ALL_DEFINED (:2176)
int mifc_shapiro2_filter(mifc_ctx* c, int nx, int ny, const float* field, float* fsmooth, int* fdefined, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  if (nx < 3 || ny < 3 || !field || !fsmooth) // :2093
    return 0;
  const size_t n = (size_t)nx * (size_t)ny;
  if (n > 0x7fffffffu)
    return 0;
  Staging st(c, memkind);
  const float* d_in = st.in(field, n);
  float* d_out = st.out(fsmooth, n);
  return st.ok() && shapiro_run(c, st, nx, ny, 1, d_in, d_out, fdefined, undef);
}

} // extern "C"
