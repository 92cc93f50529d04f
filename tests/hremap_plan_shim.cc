// C entries around mifc_hremap_plan.h (mi-fieldcalc_amd/csrc) for tests/test_hremap_cpu.py: host compiler only.
#include <cstdio>
#include <cstring>

#include "mifc_hremap_plan.h"

namespace {
mifc::HremapLayout g_layout;
}

extern "C" {

// The refusals of mifc_hremap_plan_create that read the table: 1, or 0 with the reason in `why`.
int mifc_test_hremap_check(int nsrc, int ndst, const int* rowptr, const int* col, const float* w, char* why, int why_len)
{
  long long nnz = 0;
  std::string r = mifc::hremap_check_rows(nsrc, ndst, rowptr, &nnz);
  if (r.empty())
    r = mifc::hremap_check_entries(nsrc, nnz, col, w);
  std::snprintf(why, (size_t)why_len, "%s", r.c_str());
  return r.empty() ? 1 : 0;
}

// The layout of a table that passed; info: nnz, max_row, empty_rows, nslices, max_width, entries.
void mifc_test_hremap_layout(int nsrc, int ndst, const int* rowptr, const int* col, const float* w, long long* info)
{
  mifc::hremap_layout(nsrc, ndst, rowptr, col, w, g_layout);
  const long long v[] = {g_layout.nnz, g_layout.max_row, g_layout.empty_rows, g_layout.nslices, g_layout.max_width, (long long)g_layout.entries.size()};
  std::memcpy(info, v, sizeof v);
}

// The arrays of the last layout, each into room of the sizes `info` gave.
void mifc_test_hremap_copy(unsigned long long* slice_off, int* slice_width, int* len, double* wall, int* ent_col, float* ent_w)
{
  const mifc::HremapLayout& L = g_layout;
  std::memcpy(slice_off, L.slice_off.data(), L.slice_off.size() * sizeof(unsigned long long));
  std::memcpy(slice_width, L.slice_width.data(), L.slice_width.size() * sizeof(int));
  std::memcpy(len, L.len.data(), L.len.size() * sizeof(int));
  std::memcpy(wall, L.wall.data(), L.wall.size() * sizeof(double));
  for (size_t e = 0; e < L.entries.size(); ++e) {
    ent_col[e] = L.entries[e].col;
    ent_w[e] = L.entries[e].w;
  }
}
}
