// The rules of mi-fieldcalc_amd/csrc/mifc_vregrid_rules.h as a stand-alone host program (no HIP, no device):
// tests/test_vregrid_cpu.py builds it with -fsanitize=address,undefined and runs it.  Every batch, plane and result is a
// vector of exactly the size the rules may touch, so a level index outside the column -- from the clamp of a column
// without a usable level, from a walk against the index order -- is an error of the run; the hand-computed columns of the
// Python test are checked here too.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "vregrid_rules_driver.h"

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

float uniform(unsigned int& state, float lo, float hi)
{
  return lo + (hi - lo) * (float)(next(state) >> 8) / 16777216.0f;
}

const float UNDEF = 1.0e35f;
const float NaN = std::numeric_limits<float>::quiet_NaN(), INF = std::numeric_limits<float>::infinity();

// one column (nx = ny = 1) of one field on a coordinate batch: the result per target
std::vector<float> column(const std::vector<float>& c, const std::vector<float>& x, const std::vector<float>& targets, int method, int from, int outside,
                          std::vector<int>* flags = nullptr)
{
  const int nlev = (int)c.size(), nt = (int)targets.size();
  const vregrid_test::Call call = {vregrid_test::FIELD, 1, 1, nlev, 1, nt, x.data(), nullptr, c.data(), vregrid_test::SOME_DEFINED, nullptr, nullptr, nullptr,
                                   targets.data(), nullptr, method, from, outside, UNDEF};
  std::vector<float> out((size_t)nt, -1.0f);
  std::vector<int> fl((size_t)nt, -1);
  vregrid_test::run(call, out.data(), fl.data());
  if (flags)
    *flags = fl;
  return out;
}

void by_hand()
{
  // strictly monotone, top-down and bottom-up
  const std::vector<float> down = {100, 200, 400, 800}, up = {800, 400, 200, 100}, x = {1, 2, 4, 8}, xr = {8, 4, 2, 1};
  for (int from = 0; from < 2; ++from) {
    std::vector<float> r = column(down, x, {150, 200, 600, 50, 900}, 0, from, 0);
    expect(r[0] == 1.5f && r[1] == 2.0f && r[2] == 6.0f && r[3] == UNDEF && r[4] == UNDEF, "monotone top-down", from);
    r = column(up, xr, {150, 200, 600, 50, 900}, 0, from, 1);
    expect(r[0] == 1.5f && r[1] == 2.0f && r[2] == 6.0f && r[3] == 1.0f && r[4] == 8.0f, "monotone bottom-up, clamped", from);
  }
  // FROM_FIRST at an interior level finds the pair above it (weight 1), FROM_LAST the pair below (weight 0)
  // non-monotone: 300 is bracketed by (0, 1), (1, 2) and (2, 3)
  const std::vector<float> wavy = {100, 500, 200, 400}, xw = {10, 50, 20, 40};
  expect(column(wavy, xw, {300}, 0, 0, 0)[0] == 30.0f && column(wavy, {10, 50, 0, 40}, {300}, 0, 0, 0)[0] == 30.0f, "first bracket", 0);
  expect(column(wavy, {0, 0, 20, 40}, {300}, 0, 1, 0)[0] == 30.0f && column(wavy, {10, 50, 20, 60}, {300}, 0, 1, 0)[0] == 40.0f, "last bracket", 1);
  // c_k == c_k+1: x_k, in both directions
  expect(column({100, 300, 300, 500}, {1, 2, 3, 4}, {300}, 0, 0, 0)[0] == 2.0f, "equal levels, first", 0);
  expect(column({100, 300, 300, 500}, {1, 2, 3, 4}, {300}, 0, 1, 0)[0] == 3.0f, "equal levels, last: the pair (2, 3), weight 0", 1);
  expect(column({300, 300}, {7, 9}, {300}, 0, 1, 0)[0] == 7.0f, "equal pair: x_k whichever way", 2);
  // a hole removes the only bracket: CLAMP stays undef inside the range
  expect(column({100, UNDEF, 400, 800}, x, {150}, 0, 0, 1)[0] == UNDEF, "a gap is not clamped", 0);
  expect(column({100, UNDEF, 400, 800}, x, {50}, 0, 0, 1)[0] == 1.0f && column({100, UNDEF, 400, 800}, x, {900}, 0, 1, 1)[0] == 8.0f, "beyond the ends around a gap", 1);
  expect(column({UNDEF, UNDEF}, {1, 2}, {5}, 0, 0, 1)[0] == UNDEF && column({NaN, UNDEF, NaN}, {1, 2, 3}, {5}, 0, 1, 1)[0] == UNDEF, "no usable level", 2);
  // a tie for the extreme: the lowest index, in both directions
  for (int from = 0; from < 2; ++from) {
    expect(column({100, 100, 400, 400}, x, {50, 900}, 0, from, 1)[0] == 1.0f, "tie at the minimum", from);
    expect(column({100, 100, 400, 400}, x, {50, 900}, 0, from, 1)[1] == 4.0f, "tie at the maximum", from);
    expect(column({0.0f, -0.0f, 5}, {1, 2, 3}, {-1}, 0, from, 1)[0] == 1.0f, "-0 ties with +0", from);
  }
  // -0 against +0 brackets
  expect(column({-0.0f, 10}, {1, 2}, {0.0f}, 0, 0, 0)[0] == 1.0f && column({0.0f, 10}, {1, 2}, {-0.0f}, 0, 0, 0)[0] == 1.0f, "signed zeros bracket", 0);
  // targets that are not usable
  std::vector<int> fl;
  std::vector<float> r = column(down, x, {UNDEF, NaN, 150}, 0, 0, 1, &fl);
  expect(r[0] == UNDEF && r[1] == UNDEF && r[2] == 1.5f, "undefined and NaN targets", 0);
  expect(fl[0] == vregrid_test::NONE_DEFINED && fl[1] == vregrid_test::NONE_DEFINED && fl[2] == vregrid_test::ALL_DEFINED, "their flags", 0);
  // LOG
  r = column({100, 400}, {1, 3}, {200, 0, -5, 50}, 1, 0, 1);
  expect(r[0] == 2.0f && r[1] == UNDEF && r[2] == UNDEF && r[3] == 1.0f, "log: halfway, targets <= 0, clamped below", 0);
  expect(column({-100, 400}, {1, 3}, {200}, 1, 0, 0)[0] == UNDEF && column({0, 400}, {1, 3}, {200}, 1, 0, 0)[0] == UNDEF, "log: a coordinate <= 0 at the bracket", 1);
  expect(column({0, 400}, {1, 3}, {500}, 1, 0, 1)[0] == 3.0f, "log: the clamp copies whatever the coordinates are", 2);
  expect(column({INF, 5}, {1, 3}, {7, INF}, 0, 0, 1)[0] != UNDEF, "an infinite coordinate brackets", 3);
}

// random calls of every kind with holes, NaN and infinities: sizes exact, every result a copy, an interpolation or undef
void random_calls()
{
  unsigned int state = 4711u;
  for (int round = 0; round < 24; ++round) {
    const int kind = round % 3, nx = 1 + round % 5, ny = 1 + round % 3, nlev = 2 + round % 6, nf = 1 + round % 3, nt = 1 + round % 4;
    const size_t cells = (size_t)nx * ny;
    std::vector<float> fields((size_t)nf * nlev * cells), coord(kind == vregrid_test::HYBRID ? cells : (kind == vregrid_test::FIELD ? nlev * cells : (size_t)nlev)),
        tc((size_t)nt * cells), a((size_t)nlev), b((size_t)nlev);
    for (float& v : fields)
      v = next(state) % 10 == 0 ? UNDEF : uniform(state, -5.0f, 5.0f);
    for (float& v : coord)
      v = kind == vregrid_test::HYBRID ? (next(state) % 8 == 0 ? UNDEF : uniform(state, 500.0f, 1000.0f))
                                       : (kind == vregrid_test::FIELD && next(state) % 6 == 0 ? (next(state) % 2 ? UNDEF : NaN) : std::round(uniform(state, -2.0f, 9.0f)) * 100.0f);
    for (int k = 0; k < nlev; ++k) {
      a[k] = uniform(state, 0.0f, 50.0f);
      b[k] = uniform(state, 0.0f, 1.0f);
    }
    for (float& v : tc) {
      const unsigned int pick = next(state) % 12;
      v = pick == 0 ? UNDEF : (pick == 1 ? NaN : (pick == 2 ? INF : (pick == 3 ? -INF : std::round(uniform(state, -4.0f, 11.0f)) * 100.0f)));
    }
    std::vector<int> fin((size_t)nf * nlev), fco((size_t)nlev), ftc((size_t)nt);
    for (int& f : fin)
      f = (int)(next(state) % 3);
    for (int& f : fco)
      f = (int)(next(state) % 3);
    for (int& f : ftc)
      f = (int)(next(state) % 3);
    for (int variant = 0; variant < 8; ++variant) {
      const vregrid_test::Call c = {kind, nx, ny, nlev, nf, nt, fields.data(), round % 2 ? fin.data() : nullptr, coord.data(), (int)(next(state) % 3),
                                    round % 2 ? fco.data() : nullptr, a.data(), b.data(), tc.data(), round % 2 ? ftc.data() : nullptr, variant & 1, (variant >> 1) & 1,
                                    (variant >> 2) & 1, UNDEF};
      std::vector<float> out((size_t)nf * nt * cells, -1.0f);
      std::vector<int> flags((size_t)nf * nt, -1);
      vregrid_test::run(c, out.data(), flags.data());
      for (int f : flags)
        expect(f == vregrid_test::ALL_DEFINED || f == vregrid_test::NONE_DEFINED || f == vregrid_test::SOME_DEFINED, "a flag", f);
      for (size_t j = 0; j < out.size(); ++j)
        expect(out[j] != -1.0f, "every result is written", (long)j);
    }
  }
}

void extremes()
{
  for (int descending = 0; descending < 2; ++descending) {
    const float cols[4][4] = {{3, 1, 1, 3}, {NaN, 2, NaN, 2}, {NaN, NaN, NaN, NaN}, {INF, INF, -INF, -INF}};
    const int want[4][2] = {{1, 0}, {1, 1}, {-1, -1}, {2, 0}};
    for (int n = 0; n < 4; ++n) {
      mifc::VregridExtremes e;
      mifc::vregrid_extremes_start(e);
      for (int s = 0; s < 4; ++s) {
        const int k = descending ? 3 - s : s;
        mifc::vregrid_extremes_level(e, cols[n][k], k, descending != 0);
      }
      expect(e.kmin == want[n][0] && e.kmax == want[n][1], "the lowest index of each extreme", n * 2 + descending);
      expect(mifc::vregrid_clamp_level(e, NaN) == -1, "a NaN target is not outside", n);
      expect(n != 2 || (mifc::vregrid_clamp_level(e, -1.0e30f) == -1 && mifc::vregrid_clamp_level(e, 1.0e30f) == -1), "no usable level: no clamp", n);
    }
  }
}

} // namespace

int main()
{
  by_hand();
  random_calls();
  extremes();
  std::printf("%d checks, %d failures\n", checks, failures);
  return failures == 0 ? 0 : 1;
}
