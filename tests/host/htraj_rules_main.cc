// The rules of mi-fieldcalc_amd/csrc/mifc_htraj_rules.h as a stand-alone host program (no HIP, no device):
// tests/test_htraj_cpu.py builds it with -fsanitize=address,undefined and runs it.  Every plane, position list and result
// is an array of exactly the size the rules may touch, so a read outside a plane -- from a position on the last column or
// row, outside the grid, infinite or NaN -- is an error of the run; uniform winds on an exact map are checked by hand.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "htraj_rules_driver.h"

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

// the positions that may not make the rules read outside a plane
std::vector<float> hard_positions(int n)
{
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  return {0.0f, -0.0f, (float)(n - 1), std::nextafter((float)(n - 1), inf), std::nextafter((float)(n - 1), 0.0f), -1.0e-45f, -0.5f, (float)n, 1.0e30f,
          -1.0e30f, inf, -inf, nan, UNDEF, 0.5f, (float)(n - 1) * 0.5f};
}

void cells()
{
  for (int nx : {1, 2, 5})
    for (int ny : {1, 3}) {
      std::vector<float> plane((size_t)nx * ny, 1.0f);
      for (float x : hard_positions(nx))
        for (float y : hard_positions(ny)) {
          const bool live = mifc::htraj_inside((double)x, (double)y, nx, ny);
          const mifc::HtrajCell c = mifc::htraj_cell((double)x, (double)y, nx, ny, live);
          const int n = nx * ny;
          expect(c.o00 >= 0 && c.o00 < n && c.o10 >= 0 && c.o10 < n && c.o01 >= 0 && c.o01 < n && c.o11 >= 0 && c.o11 < n, "an offset outside the plane", nx * 10 + ny);
          bool ok;
          const double r = mifc::htraj_value<true>(c, mifc::htraj_load(plane.data(), c), UNDEF, ok);
          expect(ok && r == 1.0, "a constant plane", nx * 10 + ny);
          // a cell that did NOT pass the test is clamped all the same
          const mifc::HtrajCell forced = mifc::htraj_cell(x == x && std::fabs(x) < 1.0e9f ? (double)x : 0.0, y == y && std::fabs(y) < 1.0e9f ? (double)y : 0.0, nx, ny, true);
          expect(forced.o00 >= 0 && forced.o11 < n && forced.o10 < n && forced.o01 < n, "the clamp without the test", nx * 10 + ny);
          (void)mifc::htraj_load(plane.data(), forced);
        }
    }
}

// a random call with holes, hard starts among the positions: everything the driver touches has its exact size
void random_calls()
{
  unsigned int state = 12345u;
  for (int round = 0; round < 6; ++round) {
    const int nx = round == 0 ? 1 : 3 + round, ny = round == 1 ? 1 : 4, nlev = 1 + round % 2, nt = 3, ntrace = round % 3, nsub = 1 + round, niter = round % 4;
    const size_t batch = (size_t)nt * nlev * ny * nx;
    std::vector<float> u(batch), v(batch), trace((size_t)ntrace * batch), xm((size_t)nx * ny), ym((size_t)nx * ny);
    for (float& x : u)
      x = next(state) % 50 == 0 ? UNDEF : uniform(state, -3.0f, 3.0f);
    for (float& x : v)
      x = uniform(state, -3.0f, 3.0f);
    for (float& x : trace)
      x = next(state) % 20 == 0 ? UNDEF : uniform(state, 250.0f, 300.0f);
    for (float& x : xm)
      x = 1.0e-4f * uniform(state, 0.9f, 1.1f);
    for (float& x : ym)
      x = 1.0e-4f * uniform(state, 0.9f, 1.1f);
    std::vector<float> xs = hard_positions(nx), ys = hard_positions(ny);
    for (int p = 0; p < 40; ++p) {
      xs.push_back(uniform(state, 0.0f, (float)(nx - 1)));
      ys.push_back(uniform(state, 0.0f, (float)(ny - 1)));
    }
    ys.resize(xs.size(), 0.0f);
    const int npos = (int)xs.size();
    const double times[3] = {0.0, 3000.0, 7000.0};
    for (int backward = 0; backward < 2; ++backward) {
      const htraj_test::Call c = {nx, ny, nlev, nt, u.data(), v.data(), nullptr, times, xm.data(), ym.data(), htraj_test::SOME_DEFINED, npos, xs.data(),
                                  ys.data(), backward ? 2 : 0, backward ? 0 : 2, nsub, niter, ntrace ? trace.data() : nullptr, nullptr, ntrace, UNDEF};
      const size_t out = (size_t)3 * nlev * npos;
      std::vector<float> xr(out, -1.0f), yr(out, -1.0f), tr((size_t)ntrace * out, -1.0f);
      std::vector<int> flags((size_t)(1 + ntrace) * 3 * nlev, -1);
      htraj_test::run(c, xr.data(), yr.data(), tr.data(), flags.data());
      long alive_last = 0;
      for (size_t i = 0; i < out; ++i) {
        const bool lost = xr[i] == UNDEF;
        expect(lost == (yr[i] == UNDEF), "x and y are lost together", (long)i);
        expect(lost || mifc::htraj_inside((double)xr[i], (double)yr[i], nx, ny), "a stored position is inside", (long)i);
        if (i >= out - (size_t)nlev * npos)
          alive_last += lost ? 0 : 1;
      }
      for (size_t i = (size_t)nlev * npos; i < out; ++i) // once lost, lost
        expect(xr[i - (size_t)nlev * npos] != UNDEF || xr[i] == UNDEF, "a lost particle stays lost", (long)i);
      for (int f : flags)
        expect(f == htraj_test::ALL_DEFINED || f == htraj_test::NONE_DEFINED || f == htraj_test::SOME_DEFINED, "a flag", f);
      expect(nx == 1 || ny == 1 || alive_last > 0, "some particle reaches the last slot", round);
    }
  }
}

// a uniform wind on the uniform exact map 2^-10 moves exactly h * u * m per substep
void by_hand()
{
  const int nx = 5, ny = 4;
  const float m = 1.0f / 1024.0f;
  std::vector<float> u((size_t)2 * nx * ny, 1.0f), v((size_t)2 * nx * ny, -0.5f), xm((size_t)nx * ny, m), ym((size_t)nx * ny, m);
  const double times[2] = {0.0, 1024.0};
  const float xs[3] = {3.0f, std::nextafter(3.0f, 4.0f), 0.25f}, ys[3] = {1.0f, 1.0f, 3.0f};
  for (int niter = 0; niter <= 2; ++niter)
    for (int nsub : {1, 4}) {
      const htraj_test::Call c = {nx, ny, 1, 2, u.data(), v.data(), nullptr, times, xm.data(), ym.data(), htraj_test::ALL_DEFINED, 3, xs, ys, 0, 1, nsub, niter,
                                  nullptr, nullptr, 0, UNDEF};
      float xr[6], yr[6];
      int flags[2];
      htraj_test::run(c, xr, yr, nullptr, flags);
      expect(xr[0] == 3.0f && yr[0] == 1.0f && xr[3] == 4.0f && yr[3] == 0.5f, "exactly onto the last column", niter * 10 + nsub);
      expect(xr[1] == xs[1] && xr[4] == UNDEF && yr[4] == UNDEF, "one ulp beyond the last column", niter * 10 + nsub);
      expect(xr[5] == 1.25f && yr[5] == 2.5f, "a uniform step", niter * 10 + nsub);
      expect(flags[0] == htraj_test::ALL_DEFINED && flags[1] == htraj_test::SOME_DEFINED, "the flags", niter * 10 + nsub);
    }
}

void arguments()
{
  const double t[4] = {0.0, 1.0, 2.0, 3.0}, bad[4] = {0.0, 1.0, 1.0, std::numeric_limits<double>::infinity()};
  expect(mifc::htraj_check(5, 4, 1, 4, 3, 0, 3, 4, 2, 0, t, UNDEF) == nullptr, "a good call", 0);
  expect(mifc::htraj_check(5, 4, 1, 1, 3, 0, 0, 4, 2, 0, t, UNDEF) != nullptr, "nt", 1);
  expect(mifc::htraj_check(5, 4, 1, 4, 3, 0, 4, 4, 2, 0, t, UNDEF) != nullptr, "j_end", 2);
  expect(mifc::htraj_check(5, 4, 1, 4, 3, 1, 2, 4, 2, 0, bad, UNDEF) != nullptr, "equal times", 3);
  expect(mifc::htraj_check(5, 4, 1, 4, 3, 0, 1, 4, 2, 0, bad, UNDEF) == nullptr, "the bad times are not used", 4);
  expect(mifc::htraj_check(5, 4, 1, 4, 3, 3, 2, 4, 2, 0, bad, UNDEF) != nullptr, "an infinite time", 5);
  expect(mifc::htraj_check(5, 4, 1, 4, 3, 0, 3, 4, 2, 0, t, 4.0f) != nullptr, "undef inside", 6);
  expect(mifc::htraj_check(5, 4, 1, 4, 3, 0, 3, 4, 2, 0, t, std::numeric_limits<float>::quiet_NaN()) == nullptr, "a NaN undef", 7);
  expect(mifc::htraj_check(1 << 24, 128, 1, 4, 3, 0, 3, 4, 2, 0, t, UNDEF) != nullptr, "the cell limit", 8);
  const mifc::HtrajPlan p = mifc::htraj_plan(3, 1);
  expect(p.dir == -1 && p.nslots == 3 && p.intervals == 2 && mifc::htraj_slice(p, 3, 2) == 1, "the plan of a backward run", 9);
  // (2 * 3 planes of 1000 cells and 3 planes of 3 slots of 10 particles) * 4 bytes = 24 360 bytes per level
  expect(mifc::htraj_levels_per_chunk(1u << 20, mifc::htraj_bytes_per_level(1000, 10, 3, 1), 50) == 43, "the levels of a chunk", 10);
  expect(mifc::htraj_levels_per_chunk(1u << 10, mifc::htraj_bytes_per_level(1000, 10, 3, 1), 50) == 1, "never less than a level", 11);
  expect(mifc::htraj_level_chunk(137, 0) == 1 && mifc::htraj_level_chunk(137, 50) == 50 && mifc::htraj_level_chunk(7, 50) == 7 && mifc::htraj_level_chunk(200000, 0) == 4,
         "the levels of a workgroup", 12);
}

} // namespace

int main()
{
  cells();
  random_calls();
  by_hand();
  arguments();
  std::printf("%d checks, %d failures\n", checks, failures);
  return failures == 0 ? 0 : 1;
}
