// The rules of mi-fieldcalc_amd/csrc/mifc_hdist_rules.h as a stand-alone host program (no HIP, no device):
// tests/test_hdist_cpu.py builds it with -fsanitize=address,undefined and runs it.  Keys, bins, ranks, digit plans and the
// selection by scan steps go through arrays of exactly the size the rules may read, against a sort and a linear count.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "mifc_hdist_rules.h"

namespace {

int failures = 0, checks = 0;

void expect(bool ok, const char* what, long where)
{
  checks += 1;
  if (!ok) {
    std::fprintf(stderr, "%s (%ld)\n", what, where);
    failures += 1;
  }
}

unsigned int next(unsigned int& state)
{
  state = state * 1664525u + 1013904223u;
  return state;
}

std::vector<float> special_values()
{
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  return {-inf, -3.4028235e38f, -1.0f, -1.0e-40f, -1.4e-45f, -0.0f, 0.0f, 1.4e-45f, 1.0e-40f, 1.0f, 3.4028235e38f, inf, nan, -nan};
}

// the total order by hand: NaN last, -0 before +0
bool total_less(float a, float b)
{
  const bool an = a != a, bn = b != b;
  if (an || bn)
    return !an && bn;
  if (a == b)
    return std::signbit(a) && !std::signbit(b);
  return a < b;
}

void keys()
{
  const std::vector<float> v = special_values();
  for (size_t i = 0; i < v.size(); ++i)
    for (size_t j = 0; j < v.size(); ++j) {
      const unsigned int ki = mifc::hdist_order_key(mifc::hdist_float_bits(v[i])), kj = mifc::hdist_order_key(mifc::hdist_float_bits(v[j]));
      expect((ki < kj) == total_less(v[i], v[j]), "order key against the total order", (long)(i * 100 + j));
      if (v[i] == v[i] && v[j] == v[j]) {
        const unsigned int bi = mifc::hdist_bin_key(mifc::hdist_float_bits(v[i])), bj = mifc::hdist_bin_key(mifc::hdist_float_bits(v[j]));
        expect((bi <= bj) == (v[i] <= v[j]), "bin key against <=", (long)(i * 100 + j));
      }
    }
  for (size_t i = 0; i < v.size(); ++i) {
    const unsigned int b = mifc::hdist_float_bits(v[i]), back = mifc::hdist_key_bits(mifc::hdist_order_key(b));
    expect(v[i] != v[i] ? back == mifc::HDIST_NAN_BITS : back == b, "key and back", (long)i);
  }
}

void bins()
{
  for (int nedges : {1, 2, 63, 64, 65, 1024}) {
    std::vector<float> edges((size_t)nedges); // exactly nedges: a read past the end is the sanitizer's
    for (int e = 0; e < nedges; ++e)
      edges[(size_t)e] = -3.0f + 0.0078125f * (float)e;
    expect(mifc::hdist_check_edges(edges.data(), nedges) == -1, "ascending edges refused", nedges);
    std::vector<unsigned int> ekeys((size_t)nedges);
    for (int e = 0; e < nedges; ++e)
      ekeys[(size_t)e] = mifc::hdist_bin_key(mifc::hdist_float_bits(edges[(size_t)e]));
    std::vector<float> xs = special_values();
    for (int e = 0; e < nedges; e += std::max(1, nedges / 7)) {
      xs.push_back(edges[(size_t)e]);
      xs.push_back(std::nextafter(edges[(size_t)e], -10.0f));
    }
    for (float x : xs) {
      int want = 0;
      for (int e = 0; e < nedges; ++e)
        want += edges[(size_t)e] <= x ? 1 : 0;
      if (x != x)
        want = nedges + 1;
      expect(mifc::hdist_slot(ekeys.data(), nedges, mifc::hdist_float_bits(x)) == want, "slot against a linear count", nedges);
    }
    if (nedges >= 2) {
      std::vector<float> bad = edges;
      bad[(size_t)nedges - 1] = bad[(size_t)nedges - 2];
      expect(mifc::hdist_check_edges(bad.data(), nedges) == nedges - 1, "equal edges pass", nedges);
      bad[0] = std::numeric_limits<float>::quiet_NaN();
      expect(mifc::hdist_check_edges(bad.data(), nedges) == 0, "a NaN edge passes", nedges);
    }
  }
  const float zeros[2] = {-0.0f, 0.0f};
  expect(mifc::hdist_check_edges(zeros, 2) == 1, "both zeros pass", 0);
}

void ranks()
{
  for (int n : {1, 2, 3, 7, 1000, 16777217, 2147483647})
    for (float p : {0.0f, 1.0f, 33.3f, 50.0f, 99.99999f, 100.0f})
      for (int method : {mifc::HDIST_LOWER, mifc::HDIST_LINEAR}) {
        const mifc::HdistRank r = mifc::hdist_rank(method, n, p);
        expect(r.k >= 0 && r.k <= r.k1 && r.k1 <= n - 1 && r.k1 - r.k <= 1 && r.t >= 0.0 && r.t < 1.0, "a rank outside the values", n);
        expect((r.t == 0.0) == (r.k == r.k1), "k1 and t", n);
      }
  expect(mifc::hdist_interpolate(mifc::hdist_float_bits(1.0f), mifc::hdist_float_bits(2.0f), 0.25) == 1.25f, "interpolation", 0);
}

void selection()
{
  unsigned int state = 777u;
  std::vector<unsigned int> hist((size_t)mifc::HDIST_DIGIT_BINS);
  for (int bit = 0; bit <= 32; ++bit) { // keys that differ in their low `bit` bits, in clusters and alone
    const int n = 300;
    std::vector<unsigned int> keys((size_t)n);
    const unsigned int base = next(state), low = bit >= 32 ? 0xffffffffu : ((1u << bit) - 1u);
    for (int i = 0; i < n; ++i)
      keys[(size_t)i] = (base & ~low) | ((i % 3 == 0 ? next(state) : (next(state) & 7u)) & low);
    std::vector<unsigned int> sorted = keys;
    std::sort(sorted.begin(), sorted.end());
    const mifc::HdistPlan plan = mifc::hdist_digit_plan(sorted.front(), sorted.back());
    int covered = 0;
    for (int j = 0; j < plan.passes; ++j) {
      expect(plan.width[j] >= 1 && plan.width[j] <= mifc::HDIST_DIGIT_BITS && plan.shift[j] == 32 - plan.prefix_bits - covered - plan.width[j], "a pass of the plan", bit);
      covered += plan.width[j];
    }
    expect(covered == 32 - plan.prefix_bits && plan.passes <= mifc::HDIST_MAX_PASSES, "the plan leaves bits", bit);
    const unsigned int left = plan.prefix_bits >= 32 ? 0u : 0xffffffffu >> plan.prefix_bits;
    for (unsigned int rank : {0u, 1u, 149u, 150u, 298u, 299u}) {
      unsigned int key = sorted.front() & ~left, r = rank;
      for (int j = 0; j < plan.passes; ++j) {
        std::fill(hist.begin(), hist.end(), 0u);
        const unsigned int above = mifc::hdist_prefix_of(key, plan.shift[j], plan.width[j]);
        for (unsigned int k : keys)
          if (mifc::hdist_prefix_of(k, plan.shift[j], plan.width[j]) == above)
            hist[mifc::hdist_digit_of(k, plan.shift[j], plan.width[j])] += 1u;
        const mifc::HdistStep s = mifc::hdist_scan_step(hist.data(), 1 << plan.width[j], r);
        key |= (unsigned int)s.digit << plan.shift[j];
        r = s.rank;
      }
      expect(key == sorted[rank], "the selected key against the sort", bit * 1000 + (long)rank);
    }
  }
}

} // namespace

int main()
{
  keys();
  bins();
  ranks();
  selection();
  std::printf("%d checks, %d failures\n", checks, failures);
  return failures == 0 ? 0 : 1;
}
