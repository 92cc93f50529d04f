// mifc_hremap_plan.h -- what mifc_hremap_plan_create does with a caller's weight table before anything reaches the device:
// the refusals that read the table, Wall of every row, and the sliced-ELL layout the kernel of mifc_hremap.hip reads.  A
// pure host function of the three CSR arrays.  Plain C++, no HIP header: tests/test_hremap_cpu.py compiles it with the
// host compiler (tests/hremap_plan_shim.cc, tests/host/hremap_plan_main.cc under the address and undefined-behaviour
// sanitizers).  mifc_capi_hremap.hip brings the arrays to the host, calls these and uploads the result: the kernel reads
// only what was validated and laid out here, so no caller data can send a lane outside [0, nsrc).
//
// The layout: slices of HREMAP_SLICE = 64 destinations, one wave per slice, destination d = 64 * slice + lane.  Per
// slice an entry offset and a width, the longest row of the slice; the entries of a slice are interleaved [r][lane] as
// 8-byte (col, w) pairs, so the wave's trip r reads 512 contiguous bytes.  A lane whose row is shorter than the width, and
// the lanes of the last slice beyond ndst, carry padding entries with a VALID column (the row's first, 0 for an empty row)
// and weight 0; they are excluded by r < len[lane], never added as a zero (0 * inf and -0.0 would change bits).  Per
// destination (padded to whole slices): len and Wall.
#ifndef MIFC_HREMAP_PLAN_H
#define MIFC_HREMAP_PLAN_H

#include <cmath>
#include <string>
#include <vector>

namespace mifc {

const int HREMAP_SLICE = 64;

struct HremapEntry
{
  int col;
  float w;
};
static_assert(sizeof(HremapEntry) == 8, "a (col, w) pair is 8 bytes");

struct HremapLayout
{
  int nsrc = 0, ndst = 0;
  long long nnz = 0;
  int max_row = 0, empty_rows = 0;
  int nslices = 0, max_width = 0;
  std::vector<unsigned long long> slice_off; // [nslices]: the slice's first entry
  std::vector<int> slice_width;              // [nslices]: trips of the slice's wave
  std::vector<int> len;                      // [nslices * 64]
  std::vector<double> wall;                  // [nslices * 64]: the sequential double sum of the row's weights from +0.0
  std::vector<HremapEntry> entries;          // slice_off[s] + r * 64 + lane
};

// The refusals that read rowptr: "" and nnz, or the reason.
inline std::string hremap_check_rows(int nsrc, int ndst, const int* rowptr, long long* nnz)
{
  if (nsrc < 1 || ndst < 1)
    return "nsrc < 1 or ndst < 1";
  if (rowptr[0] != 0)
    return "rowptr[0] != 0";
  if (rowptr[ndst] < 0)
    return "nnz = rowptr[ndst] is negative";
  for (int d = 0; d < ndst; ++d)
    if (rowptr[d + 1] < rowptr[d])
      return "rowptr decreases at row " + std::to_string(d);
  *nnz = rowptr[ndst];
  return "";
}

// The refusals that read the entries.
inline std::string hremap_check_entries(int nsrc, long long nnz, const int* col, const float* w)
{
  for (long long e = 0; e < nnz; ++e) {
    if (col[e] < 0 || col[e] >= nsrc)
      return "col[" + std::to_string(e) + "] = " + std::to_string(col[e]) + " outside [0, nsrc)";
    if (!std::isfinite(w[e]))
      return "w[" + std::to_string(e) + "] is NaN or infinite";
  }
  return "";
}

// The layout of a table that passed both checks.  (May throw std::bad_alloc; the caller catches.)
inline void hremap_layout(int nsrc, int ndst, const int* rowptr, const int* col, const float* w, HremapLayout& L)
{
  L = HremapLayout();
  L.nsrc = nsrc;
  L.ndst = ndst;
  L.nnz = rowptr[ndst];
  L.nslices = (ndst + HREMAP_SLICE - 1) / HREMAP_SLICE;
  const size_t padded = (size_t)L.nslices * HREMAP_SLICE;
  L.slice_off.assign(L.nslices, 0);
  L.slice_width.assign(L.nslices, 0);
  L.len.assign(padded, 0);
  L.wall.assign(padded, 0.0);
  unsigned long long total = 0;
  for (int s = 0; s < L.nslices; ++s) {
    int width = 0;
    for (int lane = 0; lane < HREMAP_SLICE; ++lane) {
      const int d = s * HREMAP_SLICE + lane;
      if (d >= ndst)
        break;
      const int n = rowptr[d + 1] - rowptr[d];
      L.len[d] = n;
      L.empty_rows += n == 0 ? 1 : 0;
      width = n > width ? n : width;
      double sum = 0.0;
      for (int e = rowptr[d]; e < rowptr[d + 1]; ++e)
        sum = sum + (double)w[e];
      L.wall[d] = sum;
    }
    L.slice_off[s] = total;
    L.slice_width[s] = width;
    L.max_width = width > L.max_width ? width : L.max_width;
    total += (unsigned long long)width * HREMAP_SLICE;
  }
  L.max_row = L.max_width;
  L.entries.assign((size_t)total, HremapEntry{0, 0.f});
  for (int s = 0; s < L.nslices; ++s) {
    HremapEntry* at = L.entries.data() + L.slice_off[s];
    for (int lane = 0; lane < HREMAP_SLICE; ++lane) {
      const int d = s * HREMAP_SLICE + lane;
      const int n = d < ndst ? L.len[d] : 0;
      const int pad = n > 0 ? col[rowptr[d]] : 0;
      for (int r = 0; r < L.slice_width[s]; ++r)
        at[(size_t)r * HREMAP_SLICE + lane] = r < n ? HremapEntry{col[rowptr[d] + r], w[rowptr[d] + r]} : HremapEntry{pad, 0.f};
    }
  }
}

} // namespace mifc

#endif // MIFC_HREMAP_PLAN_H
