// mifc_capi_ensemble.hip -- C ABI of mifc_ensemble_levels (include/mifc.h): the refusals, the products of the list put
// into the kernel's fixed slots, the kernel-argument or device tables of the launch, host-memory batches staged in
// bounded chunks, then the kernel of mifc_ensemble_levels.hip.
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
  c->err = "mifc_ensemble_levels: " + why;
  return 0;
}

} // namespace

extern "C" {

int mifc_ensemble_levels(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nmem,
                         const mifc_ens_product* products, int nproducts, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  if (c->capturing)
    return refuse(c, "not available while a mifc_graph capture is open");
  if (nproducts < 1)
    return refuse(c, "nproducts < 1");
  if (nproducts > mifc::ENSLV_SLOTS)
    return refuse(c, "more than " + std::to_string(mifc::ENSLV_SLOTS) + " products");
  if (nlev < 1 || nx < 0 || ny < 0 || nmem < 0)
    return refuse(c, "nlev < 1, or a negative nx, ny or nmem");
  if (memkind != MIFC_MEM_HOST && memkind != MIFC_MEM_DEVICE)
    return refuse(c, "unknown memkind " + std::to_string(memkind));
  if (!products || (nmem > 0 && !fields))
    return refuse(c, "a null pointer (products or fields)");
  for (int j = 0; j < nmem; ++j)
    if (!fields[j])
      return refuse(c, "a null pointer (fields[" + std::to_string(j) + "])");

  // the products into their slots: 0 SUM, 1 MEAN, 2 STDDEV, 2 + compute EXTREME, 7.. PROBABILITY in list order
  int slot_of[mifc::ENSLV_SLOTS];
  unsigned int live = 0;
  int nprob = 0;
  mifc::EnsLevelsParams P;
  std::memset(&P, 0, sizeof P);
  for (int k = 0; k < nproducts; ++k) {
    const mifc_ens_product& p = products[k];
    const std::string at = "products[" + std::to_string(k) + "]";
    if (!p.out || !p.fdefined)
      return refuse(c, "a null pointer (" + at + ".out or .fdefined)");
    int slot = -1;
    switch (p.stat) {
    case MIFC_ENS_SUM:
    case MIFC_ENS_MEAN:
    case MIFC_ENS_STDDEV:
      slot = p.stat;
      break;
    case MIFC_ENS_EXTREME:
      if (p.compute < 1 || p.compute > 4)
        return refuse(c, at + ": EXTREME compute " + std::to_string(p.compute) + " outside 1..4");
      if (nmem == 0)
        return refuse(c, at + ": EXTREME without members (the reference returns false)");
      slot = mifc::ENSLV_EXT0 + p.compute;
      break;
    case MIFC_ENS_PROBABILITY: {
      if (p.compute < 1 || p.compute > 6)
        return refuse(c, at + ": PROBABILITY compute " + std::to_string(p.compute) + " outside 1..6");
      if (p.nlimits < 1 || p.nlimits > 2)
        return refuse(c, at + ": PROBABILITY nlimits " + std::to_string(p.nlimits) + " outside 1..2");
      const bool between = p.compute == 3 || p.compute == 6;
      if (between && p.nlimits == 1)
        return refuse(c, at + ": PROBABILITY between two limits with one limit (the reference returns false)");
      if (nprob == mifc::ENSLV_NPROB)
        return refuse(c, "more than " + std::to_string(mifc::ENSLV_NPROB) + " PROBABILITY products");
      // FieldCalculations.cc:2821-2825
      P.check_above |= (p.compute == 1 || p.compute == 4 || between) ? 1u << nprob : 0u;
      P.check_below |= (p.compute == 2 || p.compute == 5 || between) ? 1u << nprob : 0u;
      P.value_above[nprob] = p.limits[0];
      P.value_below[nprob] = between ? p.limits[1] : p.limits[0];
      P.percent |= p.compute < 4 ? 1u << nprob : 0u;
      slot = mifc::ENSLV_PROB0 + nprob++;
      break;
    }
    default:
      return refuse(c, at + ": unknown stat " + std::to_string(p.stat));
    }
    if ((live >> slot) & 1u)
      return refuse(c, at + ": the list holds this statistic already");
    live |= 1u << slot;
    slot_of[k] = slot;
  }

  const long cells64 = (long)nx * (long)ny;
  if (cells64 > 0x7fffffffL)
    return refuse(c, "more than 2^31 - 1 cells per level");
  const size_t cells = (size_t)cells64, total = cells * (size_t)nlev, bytes = total * sizeof(float);
  for (int k = 0; k < nproducts; ++k) { // (two empty ranges never overlap)
    for (int m = 0; m < k; ++m)
      if (overlaps(products[k].out, bytes, products[m].out, bytes))
        return refuse(c, "two outputs are the same array or overlap");
    for (int j = 0; j < nmem; ++j)
      if (overlaps(products[k].out, bytes, fields[j], bytes))
        return refuse(c, "products[" + std::to_string(k) + "].out overlaps fields[" + std::to_string(j) + "]");
  }
  if (cells == 0) {
    for (int k = 0; k < nproducts; ++k)
      for (int l = 0; l < nlev; ++l)
        products[k].fdefined[l] = mifc_classify(0, 0); // n_undefined == 0 of no cells, whatever the statistic
    return 1;
  }

  // per level: the members flagged ALL_DEFINED (taken at their word) and NONE_DEFINED (probability leaves them out),
  // probability's nfields_defined, and the input flags of the SUM / EXTREME products
  const int words = nmem > 64 ? (nmem + 63) / 64 : 1;
  std::vector<u64> all_bits, none_bits;
  std::vector<int> ndef;
  std::vector<unsigned char> in_all;
  std::vector<const float*> mem;
  std::vector<u64> counts; // one per slot and level
  const size_t ncounts = (size_t)mifc::ENSLV_SLOTS * (size_t)nlev;
  try { // nothing may be thrown across the C ABI
    all_bits.assign((size_t)nlev * (size_t)words, 0ull);
    none_bits.assign((size_t)nlev * (size_t)words, 0ull);
    ndef.assign((size_t)nlev, nmem);
    in_all.assign((size_t)nlev, 0);
    mem.resize((size_t)nmem);
    counts.resize(ncounts);
  } catch (...) {
    c->err = "out of host memory";
    return 0;
  }
  if (fdefined_in)
    for (int j = 0; j < nmem; ++j)
      for (int l = 0; l < nlev; ++l) {
        const int f = fdefined_in[(size_t)j * (size_t)nlev + (size_t)l];
        const size_t w = (size_t)l * (size_t)words + (size_t)(j >> 6);
        if (f == MIFC_ALL_DEFINED)
          all_bits[w] |= 1ull << (j & 63);
        if (f == MIFC_NONE_DEFINED) {
          none_bits[w] |= 1ull << (j & 63);
          ndef[(size_t)l] -= 1;
        }
      }
  for (int k = 0; k < nproducts; ++k) {
    const int s = slot_of[k];
    if (s == 0 || (s > mifc::ENSLV_EXT0 && s < mifc::ENSLV_PROB0))
      for (int l = 0; l < nlev; ++l)
        if (products[k].fdefined[l] == MIFC_ALL_DEFINED)
          in_all[(size_t)l] |= (unsigned char)(1u << (s == 0 ? 0 : s - mifc::ENSLV_EXT0));
  }

  // device-side arrays of the launch
  const bool host = memkind == MIFC_MEM_HOST;
  Staging st(c, memkind); // blocks only: members and outputs are sub-allocated and copied chunk by chunk below
  size_t lev_chunk = (size_t)nlev, cell_chunk = cells;
  float* out[mifc::ENSLV_SLOTS]; // by product
  if (host) {
    const size_t budget = (size_t)(mifc::env().ensemble_chunk_mib > 0 ? mifc::env().ensemble_chunk_mib : 256) << 20;
    plan_level_chunks(budget, cells, (size_t)(nmem + nproducts) * sizeof(float), (size_t)nlev, &lev_chunk, &cell_chunk);
    if (cell_chunk < cells && cell_chunk >= 4)
      cell_chunk &= ~(size_t)3; // every range but the last keeps the 16-byte form
    const size_t S = align_up(lev_chunk * cell_chunk, 64);
    const float* d_mem = nmem > 0 ? static_cast<const float*>(st.scratch((size_t)nmem * S * sizeof(float))) : nullptr;
    float* d_out = static_cast<float*>(st.scratch((size_t)nproducts * S * sizeof(float)));
    if (!st.ok())
      return 0;
    for (int j = 0; j < nmem; ++j)
      mem[(size_t)j] = d_mem + (size_t)j * S;
    for (int k = 0; k < nproducts; ++k)
      out[k] = d_out + (size_t)k * S;
  } else {
    for (int j = 0; j < nmem; ++j)
      mem[(size_t)j] = fields[j];
    for (int k = 0; k < nproducts; ++k)
      out[k] = products[k].out;
  }
  bool aligned = true;
  for (int j = 0; j < nmem; ++j)
    aligned = aligned && (reinterpret_cast<uintptr_t>(mem[(size_t)j]) & 15u) == 0;
  for (int k = 0; k < nproducts; ++k)
    aligned = aligned && (reinterpret_cast<uintptr_t>(out[k]) & 15u) == 0;

  P.nmem = nmem;
  P.words = words;
  P.call_nlev = nlev;
  P.live = live;
  P.undef = undef;
  for (int k = 0; k < nproducts; ++k)
    P.out[slot_of[k]] = out[k];
  P.inline_args = (nmem <= mifc::ENSLV_KARG_MEM && nlev <= mifc::ENSLV_KARG_LEVELS) ? 1 : 0;
  std::vector<unsigned char> tab;
  if (P.inline_args) {
    for (int j = 0; j < nmem; ++j)
      P.mem_inline[j] = mem[(size_t)j];
    for (int l = 0; l < nlev; ++l) {
      P.all_inline[l] = all_bits[(size_t)l];
      P.none_inline[l] = none_bits[(size_t)l];
      P.ndef_inline[l] = (unsigned char)ndef[(size_t)l];
      P.in_all_inline[l] = in_all[(size_t)l];
    }
  } else {
    // one scratch block: member pointers | ALL_DEFINED bits | NONE_DEFINED bits | defined-member counts | input flags
    const size_t nb = all_bits.size() * sizeof(u64);
    const size_t o_all = align_up((size_t)nmem * sizeof(float*), 16), o_none = o_all + nb, o_ndef = o_none + nb;
    const size_t o_in = o_ndef + align_up((size_t)nlev * sizeof(int), 16), tab_bytes = o_in + (size_t)nlev;
    try {
      tab.assign(tab_bytes, 0);
    } catch (...) {
      c->err = "out of host memory";
      return 0;
    }
    if (nmem > 0)
      std::memcpy(tab.data(), mem.data(), (size_t)nmem * sizeof(float*));
    std::memcpy(tab.data() + o_all, all_bits.data(), nb);
    std::memcpy(tab.data() + o_none, none_bits.data(), nb);
    std::memcpy(tab.data() + o_ndef, ndef.data(), (size_t)nlev * sizeof(int));
    std::memcpy(tab.data() + o_in, in_all.data(), (size_t)nlev);
    unsigned char* d = static_cast<unsigned char*>(st.scratch(tab_bytes));
    if (!st.ok())
      return 0;
    MIFC_HIP(c, hipMemcpyAsync(d, tab.data(), tab_bytes, hipMemcpyHostToDevice, c->stream));
    P.tab.mem = reinterpret_cast<const float* const*>(d);
    P.tab.all_bits = reinterpret_cast<const u64*>(d + o_all);
    P.tab.none_bits = reinterpret_cast<const u64*>(d + o_none);
    P.tab.ndef = reinterpret_cast<const int*>(d + o_ndef);
    P.tab.in_all = d + o_in;
  }

  // 15 counters per level of the context's 5
  if (!ensure_levels(c, 3 * (size_t)nlev))
    return 0;
  P.n_undefined = c->d_counts;
  {
    P.n = (int)cell_chunk;
    P.vector_ok = aligned && (lev_chunk == 1 || (cell_chunk & 3) == 0);
    const size_t gx = (size_t)mifc::ensemble_levels_blocks(P.n, mifc::ensemble_levels_vec4(P));
    int cap = 0;
    P.partials = partials_for(c, (size_t)1024 * (size_t)mifc::ENSLV_SLOTS * gx * lev_chunk, &cap);
    P.partials_cap = P.partials ? cap : 0;
  }
  MIFC_HIP(c, hipMemsetAsync(c->d_counts, 0, ncounts * sizeof(u64), c->stream));
  for (size_t l0 = 0; l0 < (size_t)nlev; l0 += lev_chunk) {
    for (size_t c0 = 0; c0 < cells; c0 += cell_chunk) {
      const size_t nl = std::min(lev_chunk, (size_t)nlev - l0), nc = std::min(cell_chunk, cells - c0);
      const size_t off = l0 * cells + c0, elems = nl * nc; // more than one level only when nc == cells: one range
      if (host)
        for (int j = 0; j < nmem; ++j)
          MIFC_HIP(c, hipMemcpyAsync(const_cast<float*>(mem[(size_t)j]), fields[j] + off, elems * sizeof(float), hipMemcpyHostToDevice, c->stream));
      P.nlev = (int)nl;
      P.lev0 = (int)l0;
      P.n = (int)nc;
      P.stride = (long)nc;
      P.vector_ok = aligned && (nl == 1 || (nc & 3) == 0);
      MIFC_LAUNCH(c, mifc::launch_ensemble_levels(P, c->stream));
      if (host)
        for (int k = 0; k < nproducts; ++k)
          MIFC_HIP(c, hipMemcpyAsync(products[k].out + off, out[k], elems * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
  }
  MIFC_HIP(c, hipMemcpyAsync(counts.data(), c->d_counts, ncounts * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (!st.finish()) // nothing to copy back (the chunks went as they were done): the synchronisation; also, `tab` was read by its copy
    return 0;
  for (int k = 0; k < nproducts; ++k)
    for (int l = 0; l < nlev; ++l)
      products[k].fdefined[l] = mifc_classify(counts[(size_t)slot_of[k] * (size_t)nlev + (size_t)l], (u64)cells);
  return 1;
}

} // extern "C"
