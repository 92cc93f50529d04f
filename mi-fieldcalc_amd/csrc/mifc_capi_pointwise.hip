// mifc_capi_pointwise.hip -- the extern "C" boundary of the single-field elementwise operators (mifc_ewise.hip):
// vectorabs, the *leveltemp and *levelhum families, cvhum and the two momentum coordinates.  Argument validation and
// unit / compute remaps exactly as the reference does them, one launch, the undefined count turned into the flag.

#include <cmath>
#include <cstring>

#include "mifc_ctx.h"

using namespace mifc_host;

namespace {

// ---- single-field elementwise driver --------------------------------------
int run_ewise(mifc_ctx* c, mifc::EwiseParams P, const float* in0, const float* in1, const float* in2, float* out, int* fdefined, int memkind,
              bool may_keep)
{
  const size_t n = (size_t)P.n;
  Staging st(c, memkind);
  P.in0 = st.in(in0, n);
  P.in1 = st.in(in1, n);
  P.in2 = st.in(in2, n);
  P.out = st.out(out, n, may_keep);
  if (!st.ok() || !ensure_levels(c, 1))
    return 0;
  // With an ALL_DEFINED input nothing is tested, and the operators without a saturation table cannot
  // reject a cell on their own: the count is known to be zero, no counter round trip (5 us of a 19 us call)
  const bool table_free = P.op == mifc::EW_VECTORABS || P.op == mifc::EW_MOMENTUM_X || P.op == mifc::EW_MOMENTUM_Y ||
                          (P.op == mifc::EW_TEMP && P.compute >= 1 && P.compute <= 3);
  const bool counted = P.count && !(P.all_defined && table_free);
  const int want_flag = P.count;
  if (!counted)
    P.count = 0;
  P.n_undefined = c->d_counts;
  if (counted) {
    MIFC_HIP(c, hipMemsetAsync(c->d_counts, 0, sizeof(u64), c->stream));
    P.partials = partials_for(c, n, &P.partials_cap);
  }
  MIFC_LAUNCH(c, mifc::launch_ewise(P, c->stream));
  if (counted)
    MIFC_HIP(c, hipMemcpyAsync(pinned_counts(c), c->d_counts, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (!st.finish())
    return 0;
  if (counted)
    *fdefined = mifc_classify(pinned_counts(c)[0], (u64)n);
  else if (want_flag)
    *fdefined = MIFC_ALL_DEFINED; // checkDefined(0, n)
  return 1;
}

} // namespace

extern "C" {

int mifc_vectorabs(mifc_ctx* c, int nx, int ny, const float* u, const float* v, float* ff, int* fdefined, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  if (nx * ny <= 0) { // empty loop, checkDefined(0, 0)
    *fdefined = MIFC_ALL_DEFINED;
    return 1;
  }
  mifc::EwiseParams P = ewise_base(mifc::EW_VECTORABS, nx, ny, fdefined, undef);
  return run_ewise(c, P, u, v, nullptr, ff, fdefined, memkind, false);
}

int mifc_pleveltemp(mifc_ctx* c, int nx, int ny, const float* tinp, float p, const char* unit, int compute, float* tout, int* fdefined, float undef,
                    int memkind)
{
  CTX_OR_FAIL(c);
  if (p <= 0) // FieldCalculations.cc:330
    return 0;
  compute = remap_temp_compute(unit, compute); // :340-345
  if (compute < 1 || compute > 5) // :364
    return 0;
  mifc::EwiseParams P = ewise_base(mifc::EW_TEMP, nx, ny, fdefined, undef);
  P.psrc = mifc::PS_SCALAR;
  P.compute = compute;
  P.p = p;
  P.pidcp = powf(p * K_P0INV, K_KAPPA); // :347, on the host like the reference
  P.pi = P.pidcp * K_CP;
  P.count = (compute >= 4); // compute 1..3 leave fDefined untouched (:94-122)
  if (P.n <= 0) {
    if (P.count)
      *fdefined = MIFC_ALL_DEFINED;
    return 1;
  }
  return run_ewise(c, P, tinp, nullptr, nullptr, tout, fdefined, memkind, false);
}

int mifc_hleveltemp(mifc_ctx* c, int nx, int ny, const float* tinp, const float* ps, float alevel, float blevel, const char* unit, int compute,
                    float* tout, int* fdefined, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  compute = remap_temp_compute(unit, compute); // :1060-1065
  if (bad_hlevel(alevel, blevel)) // :1070
    return 0;
  mifc::EwiseParams P = ewise_base(mifc::EW_TEMP, nx, ny, fdefined, undef);
  P.psrc = mifc::PS_HYBRID;
  P.compute = compute; // no range check in the reference: other values leave defined cells unwritten
  P.alevel = alevel;
  P.blevel = blevel;
  if (P.n <= 0) {
    *fdefined = MIFC_ALL_DEFINED; // checkDefined(0, 0)
    return 1;
  }
  return run_ewise(c, P, tinp, nullptr, ps, tout, fdefined, memkind, compute < 1 || compute > 5);
}

int mifc_aleveltemp(mifc_ctx* c, int nx, int ny, const float* tinp, const float* p, const char* unit, int compute, float* tout, int* fdefined,
                    float undef, int memkind)
{
  CTX_OR_FAIL(c);
  if (compute <= 0 || compute >= 6) // :1319
    return 0;
  compute = remap_temp_compute(unit, compute);
  mifc::EwiseParams P = ewise_base(mifc::EW_TEMP, nx, ny, fdefined, undef);
  P.psrc = mifc::PS_FIELD;
  P.compute = compute;
  if (P.n <= 0) {
    *fdefined = MIFC_ALL_DEFINED;
    return 1;
  }
  return run_ewise(c, P, tinp, nullptr, p, tout, fdefined, memkind, false);
}

int mifc_plevelhum(mifc_ctx* c, int nx, int ny, const float* t, const float* huminp, float p, const char* unit, int compute, float* humout,
                   int* fdefined, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  if (p <= 0 || compute <= 0 || compute >= 13) // :419
    return 0;
  compute = remap_hum_compute(unit, compute); // :422-425
  const int n = nx * ny;
  const bool rh_td = (compute == 5 || compute == 6 || compute == 9 || compute == 10);
  mifc::EwiseParams P = ewise_base(mifc::EW_HUM, nx, ny, fdefined, undef);
  P.psrc = mifc::PS_SCALAR;
  P.p = p;
  if (p == undef && !rh_td) { // :429-432 fillUndef (:76-82): result undef everywhere, NONE_DEFINED
    if (n > 0) {
      Staging st(c, memkind);
      float* out = st.out(humout, (size_t)n);
      if (!st.ok())
        return 0;
      unsigned int bits;
      std::memcpy(&bits, &undef, sizeof bits);
      MIFC_HIP(c, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(out), (int)bits, (size_t)n, c->stream));
      if (!st.finish())
        return 0;
    }
    *fdefined = MIFC_NONE_DEFINED;
    return 1;
  }
  const float pi = K_CP * powf(p * K_P0INV, K_KAPPA); // :434 pi_from_p, on the host
  P.pi = pi;
  P.tconv = (compute % 2 == 0) ? (pi / K_CP) : 1; // :436
  P.tdconv = hum_tdconv(compute);                 // :437
  if (compute <= 2) // numbering of plevelhum (:408-415)
    P.kind = mifc::HUM_Q_RH;
  else if (compute <= 4)
    P.kind = mifc::HUM_RH_Q;
  else if (rh_td)
    P.kind = mifc::HUM_RH_TD;
  else
    P.kind = mifc::HUM_Q_TD;
  P.ptest = mifc::PT_NONE;
  if (n <= 0) {
    *fdefined = MIFC_ALL_DEFINED;
    return 1;
  }
  return run_ewise(c, P, t, huminp, nullptr, humout, fdefined, memkind, false);
}

int mifc_hlevelhum(mifc_ctx* c, int nx, int ny, const float* t, const float* huminp, const float* ps, float alevel, float blevel, const char* unit,
                   int compute, float* humout, int* fdefined, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  if (compute <= 0 || compute >= 13) // :1168
    return 0;
  if (bad_hlevel(alevel, blevel)) // :1170
    return 0;
  compute = remap_hum_compute(unit, compute); // :1174-1177
  mifc::EwiseParams P = ewise_base(mifc::EW_HUM, nx, ny, fdefined, undef);
  P.psrc = mifc::PS_HYBRID;
  P.alevel = alevel;
  P.blevel = blevel;
  P.tdconv = hum_tdconv(compute); // :1181
  P.kind = hum_kind_ah(compute);
  P.from_theta = (compute % 2 == 0);
  const bool need_p = !(compute == 7 || compute == 11); // :1182
  P.ptest = need_p ? mifc::PT_NEQ : mifc::PT_NONE;
  if (P.n <= 0) {
    *fdefined = MIFC_ALL_DEFINED;
    return 1;
  }
  return run_ewise(c, P, t, huminp, need_p ? ps : nullptr, humout, fdefined, memkind, false);
}

int mifc_alevelhum(mifc_ctx* c, int nx, int ny, const float* t, const float* huminp, const float* p, const char* unit, int compute, float* humout,
                   int* fdefined, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  if (compute <= 0 || compute >= 13) // :1414
    return 0;
  compute = remap_hum_compute(unit, compute); // :1417-1420
  mifc::EwiseParams P = ewise_base(mifc::EW_HUM, nx, ny, fdefined, undef);
  P.psrc = mifc::PS_FIELD;
  P.tdconv = hum_tdconv(compute); // :1423
  P.kind = hum_kind_ah(compute);
  P.from_theta = (compute % 2 == 0);
  // :1429 -- p is tested (with != undef) only for compute 7/11, which do not use it
  const bool tests_p = (compute == 7 || compute == 11);
  P.ptest = tests_p ? mifc::PT_NEQ : mifc::PT_NONE;
  const bool reads_p = !tests_p || !P.all_defined;
  if (P.n <= 0) {
    *fdefined = MIFC_ALL_DEFINED;
    return 1;
  }
  return run_ewise(c, P, t, huminp, reads_p ? p : nullptr, humout, fdefined, memkind, false);
}

int mifc_cvhum(mifc_ctx* c, int nx, int ny, const float* t, const float* huminp, const char* unit, int compute, float* humout, int* fdefined,
               float undef, int memkind)
{
  CTX_OR_FAIL(c);
  float unit_scale = 100; // :1746-1750
  if (compute == 1 && unit_is(unit, "celsius"))
    compute = 2;
  if ((compute == 4 || compute == 5) && unit_is(unit, "1"))
    unit_scale = 1;
  if (compute < 1 || compute > 5) // :1813
    return 0;
  mifc::EwiseParams P = ewise_base(compute <= 3 ? mifc::EW_CVHUM_TD : mifc::EW_CVHUM_RH, nx, ny, fdefined, undef);
  P.tconv = (compute == 1 || compute == 2 || compute == 4) ? K_T0 : 0; // :1753
  P.tdconv = (compute == 1) ? K_T0 : 0;                                 // :1754
  P.unit_scale = unit_scale;
  if (P.n <= 0) {
    *fdefined = MIFC_ALL_DEFINED;
    return 1;
  }
  return run_ewise(c, P, t, huminp, nullptr, humout, fdefined, memkind, false);
}

static int momentum_coordinate(mifc_ctx* c, int op, int nx, int ny, const float* wind, const float* mapr, const float* fcoriolis, float fcoriolisMin,
                               float* out, int* fdefined, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  if (nx < 3 || ny < 3) // :2363, :2397
    return 0;
  mifc::EwiseParams P = ewise_base(op, nx, ny, fdefined, undef);
  P.nx = nx;
  P.fcormin = fabsf(fcoriolisMin); // :2366
  return run_ewise(c, P, wind, mapr, fcoriolis, out, fdefined, memkind, false);
}

int mifc_momentumXcoordinate(mifc_ctx* c, int nx, int ny, const float* v, const float* xmapr, const float* fcoriolis, float fcoriolisMin, float* mxy,
                             int* fdefined, float undef, int memkind)
{
  return momentum_coordinate(c, mifc::EW_MOMENTUM_X, nx, ny, v, xmapr, fcoriolis, fcoriolisMin, mxy, fdefined, undef, memkind);
}

int mifc_momentumYcoordinate(mifc_ctx* c, int nx, int ny, const float* u, const float* ymapr, const float* fcoriolis, float fcoriolisMin, float* nxy,
                             int* fdefined, float undef, int memkind)
{
  return momentum_coordinate(c, mifc::EW_MOMENTUM_Y, nx, ny, u, ymapr, fcoriolis, fcoriolisMin, nxy, fdefined, undef, memkind);
}

const char* mifc_last_pointwise_form(void)
{
  return mifc::last_pointwise_form();
}

} // extern "C"
