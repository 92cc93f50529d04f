// The table validation and the sliced-ELL layout of mi-fieldcalc_amd/csrc/mifc_hremap_plan.h as a stand-alone host program
// (no HIP, no device): tests/test_hremap_cpu.py builds it with -fsanitize=address,undefined and runs it.  Every row-length
// pattern of the plan tests goes through the checks and the layout, the layout is read back entry by entry against the CSR
// arrays, and every refusal is provoked with arrays of exactly the size the checks may read.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "mifc_hremap_plan.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what, int pattern)
{
  if (!ok) {
    std::fprintf(stderr, "pattern %d: %s\n", pattern, what);
    failures += 1;
  }
}

struct Table
{
  int nsrc;
  std::vector<int> rowptr, col;
  std::vector<float> w;
  int ndst() const { return (int)rowptr.size() - 1; }
};

Table make(const std::vector<int>& lengths, int nsrc)
{
  Table t;
  t.nsrc = nsrc;
  t.rowptr.push_back(0);
  unsigned int state = 12345u;
  for (int n : lengths) {
    for (int r = 0; r < n; ++r) {
      state = state * 1664525u + 1013904223u;
      t.col.push_back((int)((state >> 8) % (unsigned int)nsrc));
      t.w.push_back((float)((state >> 4) & 1023u) / 512.0f - 0.25f);
    }
    t.rowptr.push_back((int)t.col.size());
  }
  return t;
}

void run(const std::vector<int>& lengths, int nsrc, int pattern)
{
  const Table t = make(lengths, nsrc);
  long long nnz = -1;
  expect(mifc::hremap_check_rows(t.nsrc, t.ndst(), t.rowptr.data(), &nnz).empty(), "rows refused", pattern);
  expect(nnz == (long long)t.col.size(), "nnz", pattern);
  expect(mifc::hremap_check_entries(t.nsrc, nnz, t.col.data(), t.w.data()).empty(), "entries refused", pattern);
  mifc::HremapLayout L;
  mifc::hremap_layout(t.nsrc, t.ndst(), t.rowptr.data(), t.col.data(), t.w.data(), L);
  const int ndst = t.ndst();
  expect(L.nslices == (ndst + 63) / 64 && (int)L.len.size() == L.nslices * 64 && (int)L.wall.size() == L.nslices * 64, "sizes", pattern);
  int longest = 0, empty = 0;
  unsigned long long total = 0;
  for (int s = 0; s < L.nslices; ++s) {
    int width = 0;
    for (int lane = 0; lane < 64 && s * 64 + lane < ndst; ++lane)
      width = std::max(width, lengths[s * 64 + lane]);
    expect(L.slice_width[s] == width && L.slice_off[s] == total, "slice offset or width", pattern);
    for (int lane = 0; lane < 64; ++lane) {
      const int d = s * 64 + lane, n = d < ndst ? lengths[d] : 0;
      expect(L.len[d] == n, "len", pattern);
      double sum = 0.0;
      for (int r = 0; r < width; ++r) {
        const mifc::HremapEntry e = L.entries[total + (unsigned long long)r * 64 + lane];
        if (r < n) {
          expect(e.col == t.col[t.rowptr[d] + r] && std::memcmp(&e.w, &t.w[t.rowptr[d] + r], 4) == 0, "entry", pattern);
          sum = sum + (double)e.w;
        } else {
          expect(e.col == (n > 0 ? t.col[t.rowptr[d]] : 0) && e.col >= 0 && e.col < nsrc, "padding column", pattern);
        }
      }
      expect(std::memcmp(&sum, &L.wall[d], 8) == 0, "Wall", pattern);
      if (d < ndst) {
        longest = std::max(longest, n);
        empty += n == 0 ? 1 : 0;
      }
    }
    total += (unsigned long long)width * 64;
  }
  expect(L.entries.size() == total && L.max_row == longest && L.empty_rows == empty && L.nnz == nnz, "totals", pattern);
}

void refusals()
{
  long long nnz = 0;
  const int ok_rows[] = {0, 1, 2}, first[] = {1, 1, 2}, down[] = {0, 2, 1}, negative[] = {0, -1, -1};
  const int cols[] = {0, 4}, low[] = {0, -1}, high[] = {5, 0};
  const float ws[] = {0.5f, 0.5f}, nan_w[] = {0.5f, std::numeric_limits<float>::quiet_NaN()}, inf_w[] = {-std::numeric_limits<float>::infinity(), 1.f};
  expect(mifc::hremap_check_rows(0, 2, ok_rows, &nnz) == "nsrc < 1 or ndst < 1", "nsrc 0", 100);
  expect(mifc::hremap_check_rows(5, 0, ok_rows, &nnz) == "nsrc < 1 or ndst < 1", "ndst 0", 100);
  expect(mifc::hremap_check_rows(5, 2, first, &nnz) == "rowptr[0] != 0", "rowptr[0]", 100);
  expect(mifc::hremap_check_rows(5, 2, down, &nnz) == "rowptr decreases at row 1", "decreasing", 100);
  expect(mifc::hremap_check_rows(5, 2, negative, &nnz) == "nnz = rowptr[ndst] is negative", "negative nnz", 100);
  expect(mifc::hremap_check_rows(5, 2, ok_rows, &nnz).empty() && nnz == 2, "a good rowptr", 100);
  expect(mifc::hremap_check_entries(5, 2, cols, ws).empty(), "good entries", 100);
  expect(mifc::hremap_check_entries(5, 2, low, ws) == "col[1] = -1 outside [0, nsrc)", "col -1", 100);
  expect(mifc::hremap_check_entries(5, 2, high, ws) == "col[0] = 5 outside [0, nsrc)", "col nsrc", 100);
  expect(mifc::hremap_check_entries(5, 2, cols, nan_w) == "w[1] is NaN or infinite", "NaN weight", 100);
  expect(mifc::hremap_check_entries(5, 2, cols, inf_w) == "w[0] is NaN or infinite", "infinite weight", 100);
}

} // namespace

int main()
{
  std::vector<int> ramp(64), spike(130, 2);
  for (int i = 0; i < 64; ++i)
    ramp[i] = i;
  spike[70] = 300;
  const std::vector<std::vector<int>> patterns = {{0}, {1}, std::vector<int>(64, 3), std::vector<int>(65, 3), ramp, spike, std::vector<int>(70, 0)};
  for (size_t p = 0; p < patterns.size(); ++p)
    run(patterns[p], 117, (int)p);
  refusals();
  std::printf("hremap plan: %zu patterns, %d failures\n", patterns.size(), failures);
  return failures == 0 ? 0 : 1;
}
