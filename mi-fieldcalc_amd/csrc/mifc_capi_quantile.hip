// mifc_capi_quantile.hip -- C ABI of mifc_ensembleQuantiles (include/mifc.h; EXTENSION, no reference function):
// the refusals, the kernel-argument or device tables of the launch, host-memory batches staged in bounded chunks,
// outputs that alias a member routed through scratch, then the kernels of mifc_quantile.hip.
#include "mifc_ctx.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

using namespace mifc_host;

namespace {

int refuse(mifc_ctx* c, const std::string& why)
{
  c->err = "mifc_ensembleQuantiles: " + why;
  return 0;
}

} // namespace

extern "C" {

int mifc_ensembleQuantiles(mifc_ctx* c, int method, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nmem,
                           const float* percentiles, int nq, float* const* fres, int* fdefined_out, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  if (c->capturing)
    return refuse(c, "not available while a mifc_graph capture is open");
  if (method != MIFC_QUANTILE_LOWER && method != MIFC_QUANTILE_LINEAR)
    return refuse(c, "unknown method " + std::to_string(method) + " (MIFC_QUANTILE_LOWER or MIFC_QUANTILE_LINEAR)");
  if (nq < 1)
    return refuse(c, "nq < 1");
  if (nlev < 1 || nx < 0 || ny < 0 || nmem < 0)
    return refuse(c, "nlev < 1, or a negative nx, ny or nmem");
  if (memkind != MIFC_MEM_HOST && memkind != MIFC_MEM_DEVICE)
    return refuse(c, "unknown memkind " + std::to_string(memkind));
  if (!percentiles || !fres || !fdefined_out || (nmem > 0 && !fields))
    return refuse(c, "a null pointer (percentiles, fres, fdefined_out or fields)");
  for (int j = 0; j < nmem; ++j)
    if (!fields[j])
      return refuse(c, "a null pointer (fields[" + std::to_string(j) + "])");
  for (int q = 0; q < nq; ++q)
    if (!fres[q])
      return refuse(c, "a null pointer (fres[" + std::to_string(q) + "])");
  for (int q = 0; q < nq; ++q) {
    const float p = percentiles[q];
    if (!(p >= 0.f && p <= 100.f))
      return refuse(c, "percentiles[" + std::to_string(q) + "] is NaN or outside [0, 100]");
  }
  const long cells64 = (long)nx * (long)ny;
  if (cells64 > 0x7fffffffL)
    return refuse(c, "more than 2^31 - 1 cells per level");
  const size_t cells = (size_t)cells64, total = cells * (size_t)nlev, bytes = total * sizeof(float);
  {
    std::vector<uintptr_t> o((size_t)nq);
    for (int q = 0; q < nq; ++q)
      o[(size_t)q] = reinterpret_cast<uintptr_t>(fres[q]);
    std::sort(o.begin(), o.end());
    for (size_t k = 1; k < o.size(); ++k)
      if (o[k] == o[k - 1] || o[k - 1] + bytes > o[k])
        return refuse(c, "two outputs are the same array or overlap");
  }
  if (cells == 0) {
    for (int l = 0; l < nlev; ++l)
      fdefined_out[l] = nmem == 0 ? MIFC_NONE_DEFINED : MIFC_ALL_DEFINED; // checkDefined(0, 0), as meanValue
    return 1;
  }

  // per level: which members are flagged ALL_DEFINED (taken at their word, like meanValue's is_defined)
  const int words = nmem > 64 ? (nmem + 63) / 64 : 1;
  std::vector<u64> bits;
  std::vector<const float*> mem((size_t)nmem);
  std::vector<float*> out((size_t)nq);
  try { // nothing may be thrown across the C ABI
    bits.assign((size_t)nlev * (size_t)words, 0ull);
  } catch (...) {
    c->err = "out of host memory";
    return 0;
  }
  if (fdefined_in)
    for (int j = 0; j < nmem; ++j)
      for (int l = 0; l < nlev; ++l)
        if (fdefined_in[(size_t)j * (size_t)nlev + (size_t)l] == MIFC_ALL_DEFINED)
          bits[(size_t)l * (size_t)words + (size_t)(j >> 6)] |= 1ull << (j & 63);

  // device-side arrays of the launch
  const bool host = memkind == MIFC_MEM_HOST;
  Staging st(c, memkind); // blocks only: members and outputs are sub-allocated and copied chunk by chunk below
  size_t lev_chunk = (size_t)nlev, cell_chunk = cells, S = 0;
  std::vector<int> alias; // device memory: outputs that overlap a member, computed into scratch and copied back
  if (host) {
    // bounded staging: whole levels while they fit, else a range of cells of one level
    const size_t budget = (size_t)(mifc::env().quantile_chunk_mib > 0 ? mifc::env().quantile_chunk_mib : 256) << 20;
    plan_level_chunks(budget, cells, (size_t)(nmem + nq) * sizeof(float), (size_t)nlev, &lev_chunk, &cell_chunk);
    S = align_up(lev_chunk * cell_chunk, 64);
    const float* d_mem = nmem > 0 ? static_cast<const float*>(st.scratch((size_t)nmem * S * sizeof(float))) : nullptr;
    float* d_out = static_cast<float*>(st.scratch((size_t)nq * S * sizeof(float)));
    if (!st.ok())
      return 0;
    for (int j = 0; j < nmem; ++j)
      mem[(size_t)j] = d_mem + (size_t)j * S;
    for (int q = 0; q < nq; ++q)
      out[(size_t)q] = d_out + (size_t)q * S;
  } else {
    for (int q = 0; q < nq; ++q)
      for (int j = 0; j < nmem; ++j)
        if (overlaps(fres[q], bytes, fields[j], bytes)) { // (bytes > 0 here: an empty grid has returned above)
          alias.push_back(q);
          break;
        }
    float* d_alias = alias.empty() ? nullptr : static_cast<float*>(st.scratch(alias.size() * bytes));
    if (!st.ok())
      return 0;
    for (int j = 0; j < nmem; ++j)
      mem[(size_t)j] = fields[j];
    for (int q = 0; q < nq; ++q)
      out[(size_t)q] = fres[q];
    for (size_t k = 0; k < alias.size(); ++k)
      out[(size_t)alias[k]] = d_alias + k * total;
  }

  mifc::QuantileParams P;
  std::memset(&P, 0, sizeof P);
  P.nmem = nmem;
  P.nq = nq;
  P.method = method;
  P.words = words;
  P.undef = undef;
  P.inline_args = (nmem <= mifc::QUANTILE_KARG_MEM && nq <= mifc::QUANTILE_KARG_Q && nlev <= mifc::QUANTILE_KARG_LEVELS) ? 1 : 0;
  std::vector<unsigned char> tab;
  if (P.inline_args) {
    for (int j = 0; j < nmem; ++j)
      P.mem_inline[j] = mem[(size_t)j];
    for (int q = 0; q < nq; ++q) {
      P.out_inline[q] = out[(size_t)q];
      P.p_inline[q] = percentiles[q];
    }
    for (int l = 0; l < nlev; ++l)
      P.all_inline[l] = bits[(size_t)l];
  } else {
    // one scratch block: member pointers | output pointers | percentiles | ALL_DEFINED bits, uploaded once per call
    const size_t o_out = align_up((size_t)nmem * sizeof(float*), 16), o_p = o_out + align_up((size_t)nq * sizeof(float*), 16);
    const size_t o_bits = o_p + align_up((size_t)nq * sizeof(float), 16), tab_bytes = o_bits + bits.size() * sizeof(u64);
    try {
      tab.assign(tab_bytes, 0);
    } catch (...) {
      c->err = "out of host memory";
      return 0;
    }
    if (nmem > 0)
      std::memcpy(tab.data(), mem.data(), (size_t)nmem * sizeof(float*));
    std::memcpy(tab.data() + o_out, out.data(), (size_t)nq * sizeof(float*));
    std::memcpy(tab.data() + o_p, percentiles, (size_t)nq * sizeof(float));
    std::memcpy(tab.data() + o_bits, bits.data(), bits.size() * sizeof(u64));
    unsigned char* d = static_cast<unsigned char*>(st.scratch(tab_bytes));
    if (!st.ok())
      return 0;
    MIFC_HIP(c, hipMemcpyAsync(d, tab.data(), tab_bytes, hipMemcpyHostToDevice, c->stream));
    P.tab.mem = reinterpret_cast<const float* const*>(d);
    P.tab.out = reinterpret_cast<float* const*>(d + o_out);
    P.tab.p = reinterpret_cast<const float*>(d + o_p);
    P.tab.all_bits = reinterpret_cast<const u64*>(d + o_bits);
  }

  if (!ensure_levels(c, (size_t)nlev))
    return 0;
  P.n_undefined = c->d_counts;
  int cap = 0;
  P.partials = partials_for(c, (size_t)1024 * (size_t)mifc::quantile_blocks((int)cell_chunk) * lev_chunk, &cap);
  P.partials_cap = P.partials ? cap : 0;
  MIFC_HIP(c, hipMemsetAsync(c->d_counts, 0, (size_t)nlev * sizeof(u64), c->stream));
  if (host) {
    for (size_t l0 = 0; l0 < (size_t)nlev; l0 += lev_chunk) {
      for (size_t c0 = 0; c0 < cells; c0 += cell_chunk) {
        const size_t nl = std::min(lev_chunk, (size_t)nlev - l0), nc = std::min(cell_chunk, cells - c0);
        const size_t off = l0 * cells + c0, elems = nl * nc; // more than one level only when nc == cells: one range
        for (int j = 0; j < nmem; ++j)
          MIFC_HIP(c, hipMemcpyAsync(const_cast<float*>(mem[(size_t)j]), fields[j] + off, elems * sizeof(float), hipMemcpyHostToDevice, c->stream));
        P.nlev = (int)nl;
        P.lev0 = (int)l0;
        P.n = (int)nc;
        P.stride = (long)nc;
        MIFC_LAUNCH(c, mifc::launch_quantiles(P, c->stream));
        for (int q = 0; q < nq; ++q)
          MIFC_HIP(c, hipMemcpyAsync(fres[q] + off, out[(size_t)q], elems * sizeof(float), hipMemcpyDeviceToHost, c->stream));
      }
    }
  } else {
    P.nlev = nlev;
    P.lev0 = 0;
    P.n = (int)cells;
    P.stride = (long)cells;
    MIFC_LAUNCH(c, mifc::launch_quantiles(P, c->stream));
    for (int q : alias)
      MIFC_HIP(c, hipMemcpyAsync(fres[q], out[(size_t)q], bytes, hipMemcpyDeviceToDevice, c->stream));
  }
  std::vector<u64> counts((size_t)nlev);
  MIFC_HIP(c, hipMemcpyAsync(counts.data(), c->d_counts, (size_t)nlev * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (!st.finish()) // nothing to copy back (the chunks went as they were done): the synchronisation; also, `tab` was read by its copy
    return 0;
  for (int l = 0; l < nlev; ++l)
    fdefined_out[l] = nmem == 0 ? MIFC_NONE_DEFINED : mifc_classify(counts[(size_t)l], (u64)cells);
  return 1;
}

} // extern "C"
