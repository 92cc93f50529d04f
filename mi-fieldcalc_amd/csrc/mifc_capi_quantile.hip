// mifc_capi_quantile.hip -- C ABI of mifc_ensembleQuantiles (include/mifc.h; EXTENSION, no reference function) on the
// member-batch driver (mifc_memberbatch.h): its own refusals (method, percentiles, outputs), the kernel arguments or the
// device table, device-memory outputs that alias a member routed through scratch, then the kernels of mifc_quantile.hip.
#include "mifc_memberbatch.h"

#include <cstring>

using namespace mifc_host;

extern "C" {

int mifc_ensembleQuantiles(mifc_ctx* c, int method, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nmem,
                           const float* percentiles, int nq, float* const* fres, int* fdefined_out, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  const MemberBatchCall a = {"mifc_ensembleQuantiles", nx, ny, nlev, nmem, fields, fdefined_in, undef, memkind};
  if (c->capturing)
    return refuse(c, a, "not available while a mifc_graph capture is open");
  if (method != MIFC_QUANTILE_LOWER && method != MIFC_QUANTILE_LINEAR)
    return refuse(c, a, "unknown method " + std::to_string(method) + " (MIFC_QUANTILE_LOWER or MIFC_QUANTILE_LINEAR)");
  if (nq < 1)
    return refuse(c, a, "nq < 1");
  if (!check_head(c, a, !percentiles || !fres || !fdefined_out, "percentiles, fres, fdefined_out or fields"))
    return 0;
  for (int q = 0; q < nq; ++q)
    if (!fres[q])
      return refuse(c, a, "a null pointer (fres[" + std::to_string(q) + "])");
  for (int q = 0; q < nq; ++q) {
    const float p = percentiles[q];
    if (!(p >= 0.f && p <= 100.f))
      return refuse(c, a, "percentiles[" + std::to_string(q) + "] is NaN or outside [0, 100]");
  }
  if (!check_outputs(c, a, fres, nq))
    return 0;
  const size_t cells = a.cells();
  if (cells == 0) {
    for (int l = 0; l < nlev; ++l)
      fdefined_out[l] = nmem == 0 ? MIFC_NONE_DEFINED : MIFC_ALL_DEFINED; // checkDefined(0, 0), as meanValue
    return 1;
  }

  MemberBatch b; // one counter per level
  std::vector<int> alias; // device memory: outputs that overlap a member, computed into scratch and copied back
  std::vector<unsigned char> tab;
  auto find_aliases = [&] {
    for (int q = 0; q < (memkind == MIFC_MEM_DEVICE ? nq : 0); ++q) // (a host batch is staged, which separates them anyway)
      for (int j = 0; j < nmem; ++j)
        if (overlaps(fres[q], a.bytes(), fields[j], a.bytes())) {
          alias.push_back(q);
          break;
        }
  };
  if (!b.build(c, a, false, fres, nq, (size_t)nlev) || !host_memory(c, find_aliases))
    return 0;
  Staging st(c, memkind); // blocks only: members and outputs are sub-allocated and copied chunk by chunk
  const int mib = mifc::env().quantile_chunk_mib;
  if (!b.place(c, st, a, (size_t)(mib > 0 ? mib : 256) << 20, false))
    return 0;
  float* d_alias = alias.empty() ? nullptr : static_cast<float*>(st.scratch(alias.size() * a.bytes()));
  if (!st.ok())
    return 0;
  for (size_t k = 0; k < alias.size(); ++k)
    b.out[(size_t)alias[k]] = d_alias + k * cells * (size_t)nlev;

  mifc::QuantileParams P;
  std::memset(&P, 0, sizeof P);
  P.nmem = nmem;
  P.nq = nq;
  P.method = method;
  P.words = b.words;
  P.undef = undef;
  P.inline_args = (nmem <= mifc::QUANTILE_KARG_MEM && nq <= mifc::QUANTILE_KARG_Q && nlev <= mifc::QUANTILE_KARG_LEVELS) ? 1 : 0;
  if (P.inline_args) {
    std::copy(b.mem.begin(), b.mem.end(), P.mem_inline);
    std::copy(b.out.begin(), b.out.end(), P.out_inline);
    std::copy(percentiles, percentiles + nq, P.p_inline);
    std::copy(b.all.begin(), b.all.end(), P.all_inline);
  } else {
    const unsigned char* d[4]; // member pointers | output pointers | percentiles | ALL_DEFINED bits
    const Section mem = {b.mem.data(), (size_t)nmem * sizeof(float*)}, out = {b.out.data(), (size_t)nq * sizeof(float*)};
    if (!upload_table(c, st, tab, {mem, out, {percentiles, (size_t)nq * sizeof(float)}, {b.all.data(), b.all.size() * sizeof(u64)}}, d))
      return 0;
    P.tab.mem = reinterpret_cast<const float* const*>(d[0]);
    P.tab.out = reinterpret_cast<float* const*>(d[1]);
    P.tab.p = reinterpret_cast<const float*>(d[2]);
    P.tab.all_bits = reinterpret_cast<const u64*>(d[3]);
  }

  int cap = 0;
  P.partials = partials_for(c, (size_t)1024 * (size_t)mifc::quantile_blocks((int)b.cell_chunk) * b.lev_chunk, &cap);
  P.partials_cap = P.partials ? cap : 0;
  EnsembleForm form;
  auto launch = [&]() -> int {
    if (b.launches == 0)
      form.partials = mifc::quantile_partials(P) ? 1 : 0;
    MIFC_LAUNCH(c, mifc::launch_quantiles(P, c->stream));
    return 1;
  };
  if (!b.run(c, a, P, (size_t)nlev, launch))
    return 0;
  for (int q : alias)
    MIFC_HIP(c, hipMemcpyAsync(fres[q], b.out[(size_t)q], a.bytes(), hipMemcpyDeviceToDevice, c->stream));
  if (!b.finish(c, st)) // (the table was read by its copy)
    return 0;
  form.entry = EnsembleForm::QUANTILES;
  form.tier = mifc::quantile_tier(nmem);
  form.inline_args = P.inline_args;
  form.launches = b.launches;
  form.lev_chunk = b.lev_chunk;
  form.cell_chunk = b.cell_chunk;
  note_ensemble_form(form);
  for (int l = 0; l < nlev; ++l)
    fdefined_out[l] = nmem == 0 ? MIFC_NONE_DEFINED : b.classify((size_t)l, cells);
  return 1;
}

} // extern "C"
