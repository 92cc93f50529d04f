// A whole mifc_htraj_levels call on the host, built from mi-fieldcalc_amd/csrc/mifc_htraj_rules.h the way the kernel and
// the C entry use it: interval after interval, a lane's work per particle, the slot an interval leaves read back as the
// start of the next (an undef there is a lost particle), counters classified at the end.  For tests/htraj_rules_shim.cc
// and tests/host/htraj_rules_main.cc; host compiler only, contraction off.
#ifndef HTRAJ_RULES_DRIVER_H
#define HTRAJ_RULES_DRIVER_H

#include <cstddef>
#include <vector>

#include "mifc_htraj_rules.h"

namespace htraj_test {

const int ALL_DEFINED = 0, NONE_DEFINED = 1, SOME_DEFINED = 2;

// u, v: [nt][nlev][ny][nx]; trace: [ntrace][nt][nlev][ny][nx]; the flag tables as the C entry takes them, or null
struct Call
{
  int nx, ny, nlev, nt;
  const float *u, *v;
  const int* fdefined_in;
  const double* times;
  const float *xmapr, *ymapr;
  int fdef_map, npos;
  const float *xpos0, *ypos0;
  int j_start, j_end, nsub, niter;
  const float* trace;
  const int* fdef_trace;
  int ntrace;
  float undef;
};

inline int classify(long n_undefined, long n)
{
  return n_undefined == 0 ? ALL_DEFINED : (n_undefined == n ? NONE_DEFINED : SOME_DEFINED);
}

// xres, yres: [nslots][nlev][npos]; tres: [ntrace][nslots][nlev][npos]; flags: [(1 + ntrace)][nslots][nlev]
template <bool TESTED>
void run_as(const Call& c, float* xres, float* yres, float* tres, int* flags)
{
  const mifc::HtrajPlan plan = mifc::htraj_plan(c.j_start, c.j_end);
  const size_t cells = (size_t)c.nx * c.ny, level = cells, slice = (size_t)c.nlev * cells, slot_size = (size_t)c.nlev * c.npos;
  const size_t nslots = (size_t)plan.nslots;
  std::vector<long> counts((1 + (size_t)c.ntrace) * nslots * c.nlev, 0);
  auto wind_all = [&](int comp, int j, int k) { return c.fdefined_in && c.fdefined_in[((size_t)comp * c.nt + j) * c.nlev + k] == ALL_DEFINED; };
  auto trace_all = [&](int f, int j, int k) { return c.fdef_trace && c.fdef_trace[((size_t)f * c.nt + j) * c.nlev + k] == ALL_DEFINED; };
  auto emit = [&](int slot, int j, int k, int p, float x, float y, bool live) {
    const size_t at = (size_t)slot * slot_size + (size_t)k * c.npos + p;
    xres[at] = live ? x : c.undef;
    yres[at] = live ? y : c.undef;
    counts[(size_t)slot * c.nlev + k] += live ? 0 : 1;
    for (int f = 0; f < c.ntrace; ++f) {
      bool hole;
      const float* plane = c.trace + ((size_t)f * c.nt + j) * slice + (size_t)k * level;
      tres[(size_t)f * nslots * slot_size + at] = mifc::htraj_trace<TESTED>(plane, x, y, live, trace_all(f, j, k), c.undef, c.nx, c.ny, hole);
      counts[((size_t)(1 + f) * nslots + slot) * c.nlev + k] += hole ? 1 : 0;
    }
  };
  for (int n = 0; n < plan.intervals; ++n) {
    const int A = mifc::htraj_slice(plan, c.j_start, n), B = A + plan.dir;
    for (int k = 0; k < c.nlev; ++k) {
      const unsigned int all = (wind_all(0, A, k) ? 1u << mifc::HTRAJ_UA_BIT : 0u) | (wind_all(0, B, k) ? 1u << mifc::HTRAJ_UB_BIT : 0u) |
                               (wind_all(1, A, k) ? 1u << mifc::HTRAJ_VA_BIT : 0u) | (wind_all(1, B, k) ? 1u << mifc::HTRAJ_VB_BIT : 0u) |
                               (c.fdef_map == ALL_DEFINED ? 1u << mifc::HTRAJ_MAP_BIT : 0u);
      const mifc::HtrajWind W = {c.u + A * slice + k * level, c.u + B * slice + k * level, c.v + A * slice + k * level, c.v + B * slice + k * level,
                                 c.xmapr, c.ymapr, TESTED ? all : ~0u, c.nx, c.ny, c.undef};
      for (int p = 0; p < c.npos; ++p) {
        const size_t from = (size_t)n * slot_size + (size_t)k * c.npos + p;
        const float x0 = n == 0 ? c.xpos0[p] : xres[from], y0 = n == 0 ? c.ypos0[p] : yres[from];
        bool live = mifc::htraj_usable(x0, y0, c.undef, c.nx, c.ny);
        if (n == 0)
          emit(0, A, k, p, x0, y0, live);
        double xd = (double)x0, yd = (double)y0;
        live = mifc::htraj_interval<TESTED>(W, c.times[B] - c.times[A], c.nsub, c.niter, xd, yd, live);
        emit(n + 1, B, k, p, live ? (float)xd : c.undef, live ? (float)yd : c.undef, live);
      }
    }
  }
  for (size_t g = 0; g < 1 + (size_t)c.ntrace; ++g)
    for (size_t j = 0; j < nslots * c.nlev; ++j)
      flags[g * nslots * c.nlev + j] = classify(counts[j] + (g > 0 ? counts[g * nslots * c.nlev + j] : 0), c.npos);
}

// the instance the C entry would launch: tested unless every plane of the used slices is flagged ALL_DEFINED
inline bool any_tested(const Call& c)
{
  bool tested = c.fdef_map != ALL_DEFINED;
  const int lo = c.j_start < c.j_end ? c.j_start : c.j_end, hi = c.j_start < c.j_end ? c.j_end : c.j_start;
  for (int j = lo; j <= hi; ++j)
    for (int k = 0; k < c.nlev; ++k) {
      for (int comp = 0; comp < 2; ++comp)
        tested |= !c.fdefined_in || c.fdefined_in[((size_t)comp * c.nt + j) * c.nlev + k] != ALL_DEFINED;
      for (int f = 0; f < c.ntrace; ++f)
        tested |= !c.fdef_trace || c.fdef_trace[((size_t)f * c.nt + j) * c.nlev + k] != ALL_DEFINED;
    }
  return tested;
}

inline void run(const Call& c, float* xres, float* yres, float* tres, int* flags)
{
  if (any_tested(c))
    run_as<true>(c, xres, yres, tres, flags);
  else
    run_as<false>(c, xres, yres, tres, flags);
}

} // namespace htraj_test

#endif // HTRAJ_RULES_DRIVER_H
