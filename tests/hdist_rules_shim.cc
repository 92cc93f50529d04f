// C entries around mifc_hdist_rules.h (mi-fieldcalc_amd/csrc) for tests/test_hdist_cpu.py: host compiler only.
#include "mifc_hdist_rules.h"

extern "C" {

void mifc_test_hdist_keys(const float* x, int n, unsigned int* order, unsigned int* bin, float* back)
{
  for (int i = 0; i < n; ++i) {
    const unsigned int b = mifc::hdist_float_bits(x[i]);
    order[i] = mifc::hdist_order_key(b);
    bin[i] = mifc::hdist_bin_key(b);
    back[i] = mifc::hdist_bits_float(mifc::hdist_key_bits(order[i]));
  }
}

int mifc_test_hdist_check_edges(const float* edges, int nedges)
{
  return mifc::hdist_check_edges(edges, nedges);
}

// the slot of every value against one field's edges (their bin keys are made here, as the host code makes them)
void mifc_test_hdist_slots(const float* edges, int nedges, const float* x, int n, int* slot)
{
  unsigned int keys[mifc::HDIST_MAX_EDGES];
  for (int e = 0; e < nedges; ++e)
    keys[e] = mifc::hdist_bin_key(mifc::hdist_float_bits(edges[e]));
  for (int i = 0; i < n; ++i)
    slot[i] = mifc::hdist_slot(keys, nedges, mifc::hdist_float_bits(x[i]));
}

void mifc_test_hdist_rank(int method, int n, float p, int* k, int* k1, double* t)
{
  const mifc::HdistRank r = mifc::hdist_rank(method, n, p);
  *k = r.k;
  *k1 = r.k1;
  *t = r.t;
}

float mifc_test_hdist_interpolate(float xk, float xk1, double t)
{
  return mifc::hdist_interpolate(mifc::hdist_float_bits(xk), mifc::hdist_float_bits(xk1), t);
}

// out: prefix_bits, passes, then (shift, width) of the three passes
void mifc_test_hdist_plan(unsigned int kmin, unsigned int kmax, int* out)
{
  const mifc::HdistPlan p = mifc::hdist_digit_plan(kmin, kmax);
  out[0] = p.prefix_bits;
  out[1] = p.passes;
  for (int j = 0; j < mifc::HDIST_MAX_PASSES; ++j) {
    out[2 + 2 * j] = p.shift[j];
    out[3 + 2 * j] = p.width[j];
  }
}

void mifc_test_hdist_scan_step(const unsigned int* hist, int nbins, unsigned int rank, int* digit, unsigned int* left)
{
  const mifc::HdistStep s = mifc::hdist_scan_step(hist, nbins, rank);
  *digit = s.digit;
  *left = s.rank;
}

// The selection as the kernels run it, on the host: the key of rank `rank` among n keys, through the plan, the prefix and
// digit extraction and the scan step; *passes: the digit passes it took.
unsigned int mifc_test_hdist_select(const unsigned int* keys, int n, unsigned int rank, int* passes)
{
  unsigned int kmin = 0xffffffffu, kmax = 0u;
  for (int i = 0; i < n; ++i) {
    kmin = keys[i] < kmin ? keys[i] : kmin;
    kmax = keys[i] > kmax ? keys[i] : kmax;
  }
  const mifc::HdistPlan plan = mifc::hdist_digit_plan(kmin, kmax);
  *passes = plan.passes;
  const unsigned int low = plan.prefix_bits >= 32 ? 0u : 0xffffffffu >> plan.prefix_bits;
  unsigned int key = kmin & ~low;
  static unsigned int hist[mifc::HDIST_DIGIT_BINS];
  for (int j = 0; j < plan.passes; ++j) {
    for (int d = 0; d < mifc::HDIST_DIGIT_BINS; ++d)
      hist[d] = 0u;
    const unsigned int above = mifc::hdist_prefix_of(key, plan.shift[j], plan.width[j]);
    for (int i = 0; i < n; ++i)
      if (mifc::hdist_prefix_of(keys[i], plan.shift[j], plan.width[j]) == above)
        hist[mifc::hdist_digit_of(keys[i], plan.shift[j], plan.width[j])] += 1u;
    const mifc::HdistStep s = mifc::hdist_scan_step(hist, 1 << plan.width[j], rank);
    key |= (unsigned int)s.digit << plan.shift[j];
    rank = s.rank;
  }
  return key;
}
}
