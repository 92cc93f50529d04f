// mifc_capi_ensemble.hip -- C ABI of mifc_ensemble_levels (include/mifc.h) on the member-batch driver
// (mifc_memberbatch.h): its own refusals, the products of the list put into the kernel's fixed slots, the kernel
// arguments or the device table, then the kernel of mifc_ensemble_levels.hip.
#include "mifc_memberbatch.h"

#include <cstring>

using namespace mifc_host;

extern "C" {

int mifc_ensemble_levels(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nmem,
                         const mifc_ens_product* products, int nproducts, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  const MemberBatchCall a = {"mifc_ensemble_levels", nx, ny, nlev, nmem, fields, fdefined_in, undef, memkind};
  if (c->capturing)
    return refuse(c, a, "not available while a mifc_graph capture is open");
  if (nproducts < 1)
    return refuse(c, a, "nproducts < 1");
  if (nproducts > mifc::ENSLV_SLOTS)
    return refuse(c, a, "more than " + std::to_string(mifc::ENSLV_SLOTS) + " products");
  if (!check_head(c, a, !products, "products or fields"))
    return 0;

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
      return refuse(c, a, "a null pointer (" + at + ".out or .fdefined)");
    int slot = -1;
    switch (p.stat) {
    case MIFC_ENS_SUM:
    case MIFC_ENS_MEAN:
    case MIFC_ENS_STDDEV:
      slot = p.stat;
      break;
    case MIFC_ENS_EXTREME:
      if (p.compute < 1 || p.compute > 4)
        return refuse(c, a, at + ": EXTREME compute " + std::to_string(p.compute) + " outside 1..4");
      if (nmem == 0)
        return refuse(c, a, at + ": EXTREME without members (the reference returns false)");
      slot = mifc::ENSLV_EXT0 + p.compute;
      break;
    case MIFC_ENS_PROBABILITY: {
      if (p.compute < 1 || p.compute > 6)
        return refuse(c, a, at + ": PROBABILITY compute " + std::to_string(p.compute) + " outside 1..6");
      if (p.nlimits < 1 || p.nlimits > 2)
        return refuse(c, a, at + ": PROBABILITY nlimits " + std::to_string(p.nlimits) + " outside 1..2");
      const bool between = p.compute == 3 || p.compute == 6;
      if (between && p.nlimits == 1)
        return refuse(c, a, at + ": PROBABILITY between two limits with one limit (the reference returns false)");
      if (nprob == mifc::ENSLV_NPROB)
        return refuse(c, a, "more than " + std::to_string(mifc::ENSLV_NPROB) + " PROBABILITY products");
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
      return refuse(c, a, at + ": unknown stat " + std::to_string(p.stat));
    }
    if ((live >> slot) & 1u)
      return refuse(c, a, at + ": the list holds this statistic already");
    live |= 1u << slot;
    slot_of[k] = slot;
  }

  float* outs[mifc::ENSLV_SLOTS]; // by product
  for (int k = 0; k < nproducts; ++k)
    outs[k] = products[k].out;
  if (!check_outputs(c, a, outs, nproducts))
    return 0;
  const size_t cells = a.cells();
  for (int k = 0; k < nproducts; ++k)
    for (int j = 0; j < nmem; ++j)
      if (overlaps(outs[k], a.bytes(), fields[j], a.bytes()))
        return refuse(c, a, "products[" + std::to_string(k) + "].out overlaps fields[" + std::to_string(j) + "]");
  if (cells == 0) {
    for (int k = 0; k < nproducts; ++k)
      for (int l = 0; l < nlev; ++l)
        products[k].fdefined[l] = mifc_classify(0, 0); // n_undefined == 0 of no cells, whatever the statistic
    return 1;
  }

  MemberBatch b; // one counter per slot and level
  std::vector<unsigned char> in_all, tab; // the input flags of the SUM / EXTREME products per level; the device table
  if (!b.build(c, a, true, outs, nproducts, (size_t)mifc::ENSLV_SLOTS * (size_t)nlev) || !host_memory(c, [&] { in_all.assign((size_t)nlev, 0); }))
    return 0;
  for (int k = 0; k < nproducts; ++k) {
    const int s = slot_of[k];
    if (s == 0 || (s > mifc::ENSLV_EXT0 && s < mifc::ENSLV_PROB0))
      for (int l = 0; l < nlev; ++l)
        if (products[k].fdefined[l] == MIFC_ALL_DEFINED)
          in_all[(size_t)l] |= (unsigned char)(1u << (s == 0 ? 0 : s - mifc::ENSLV_EXT0));
  }

  Staging st(c, memkind); // blocks only: members and outputs are sub-allocated and copied chunk by chunk
  const int mib = mifc::env().ensemble_chunk_mib;
  if (!b.place(c, st, a, (size_t)(mib > 0 ? mib : 256) << 20, true))
    return 0;

  P.nmem = nmem;
  P.words = b.words;
  P.call_nlev = nlev;
  P.live = live;
  P.undef = undef;
  for (int k = 0; k < nproducts; ++k)
    P.out[slot_of[k]] = b.out[(size_t)k];
  P.inline_args = (nmem <= mifc::ENSLV_KARG_MEM && nlev <= mifc::ENSLV_KARG_LEVELS) ? 1 : 0;
  if (P.inline_args) {
    std::copy(b.mem.begin(), b.mem.end(), P.mem_inline);
    std::copy(b.all.begin(), b.all.end(), P.all_inline);
    std::copy(b.none.begin(), b.none.end(), P.none_inline);
    std::copy(b.ndef.begin(), b.ndef.end(), P.ndef_inline);
    std::copy(in_all.begin(), in_all.end(), P.in_all_inline);
  } else {
    const unsigned char* d[5]; // member pointers | ALL_DEFINED bits | NONE_DEFINED bits | defined-member counts | input flags
    const Section mem = {b.mem.data(), (size_t)nmem * sizeof(float*)}, all = {b.all.data(), b.all.size() * sizeof(u64)};
    const Section none = {b.none.data(), b.none.size() * sizeof(u64)}, ndef = {b.ndef.data(), (size_t)nlev * sizeof(int)};
    if (!upload_table(c, st, tab, {mem, all, none, ndef, {in_all.data(), (size_t)nlev}}, d))
      return 0;
    P.tab.mem = reinterpret_cast<const float* const*>(d[0]);
    P.tab.all_bits = reinterpret_cast<const u64*>(d[1]);
    P.tab.none_bits = reinterpret_cast<const u64*>(d[2]);
    P.tab.ndef = reinterpret_cast<const int*>(d[3]);
    P.tab.in_all = d[4];
  }

  P.n = (int)b.cell_chunk; // the largest launch sizes the partial counts
  P.vector_ok = b.aligned && (b.lev_chunk == 1 || (b.cell_chunk & 3) == 0);
  int cap = 0;
  const size_t gx = (size_t)mifc::ensemble_levels_blocks(P.n, mifc::ensemble_levels_vec4(P));
  P.partials = partials_for(c, (size_t)1024 * (size_t)mifc::ENSLV_SLOTS * gx * b.lev_chunk, &cap);
  P.partials_cap = P.partials ? cap : 0;
  EnsembleForm form; // the shape of the first launch: the ragged last range of a level may take the scalar form
  auto launch = [&]() -> int {
    P.vector_ok = b.aligned && (P.nlev == 1 || (P.n & 3) == 0);
    if (b.launches == 0) {
      const mifc::EnsLevelsShape s = mifc::ensemble_levels_shape(P);
      form.c = s.c;
      form.welford = s.welford ? 1 : 0;
      form.flagged = s.flagged ? 1 : 0;
      form.np = s.np;
      form.partials = s.partials ? 1 : 0;
    }
    MIFC_LAUNCH(c, mifc::launch_ensemble_levels(P, c->stream));
    return 1;
  };
  if (!b.run(c, a, P, 3 * (size_t)nlev, launch) || !b.finish(c, st)) // (15 counters per level of the context's 5)
    return 0;
  form.entry = EnsembleForm::LEVELS;
  form.inline_args = P.inline_args;
  form.launches = b.launches;
  form.lev_chunk = b.lev_chunk;
  form.cell_chunk = b.cell_chunk;
  note_ensemble_form(form);
  for (int k = 0; k < nproducts; ++k)
    for (int l = 0; l < nlev; ++l)
      products[k].fdefined[l] = b.classify((size_t)slot_of[k] * (size_t)nlev + (size_t)l, cells);
  return 1;
}

} // extern "C"
