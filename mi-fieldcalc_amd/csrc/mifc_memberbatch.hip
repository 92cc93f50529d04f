// mifc_memberbatch.hip -- the host driver of the member-batch entries (mifc_memberbatch.h).
#include "mifc_memberbatch.h"

#include <cstdint>
#include <cstdio>
#include <cstring>

namespace mifc_host {

namespace {
thread_local EnsembleForm t_form;
thread_local char t_form_text[192];
} // namespace

void note_ensemble_form(const EnsembleForm& form)
{
  t_form = form;
}

int refuse(mifc_ctx* c, const MemberBatchCall& a, const std::string& why)
{
  c->err = std::string(a.name) + ": " + why;
  return 0;
}

int check_head(mifc_ctx* c, const MemberBatchCall& a, bool other_null, const char* names)
{
  if (a.nlev < 1 || a.nx < 0 || a.ny < 0 || a.nmem < 0)
    return refuse(c, a, "nlev < 1, or a negative nx, ny or nmem");
  if (a.memkind != MIFC_MEM_HOST && a.memkind != MIFC_MEM_DEVICE)
    return refuse(c, a, "unknown memkind " + std::to_string(a.memkind));
  if (other_null || (a.nmem > 0 && !a.fields))
    return refuse(c, a, "a null pointer (" + std::string(names) + ")");
  for (int j = 0; j < a.nmem; ++j)
    if (!a.fields[j])
      return refuse(c, a, "a null pointer (fields[" + std::to_string(j) + "])");
  return 1;
}

int check_outputs(mifc_ctx* c, const MemberBatchCall& a, float* const* out, int nout)
{
  if ((long)a.nx * (long)a.ny > 0x7fffffffL)
    return refuse(c, a, "more than 2^31 - 1 cells per level");
  for (int k = 0; k < nout; ++k) // (two empty ranges never overlap)
    for (int m = 0; m < k; ++m)
      if (overlaps(out[k], a.bytes(), out[m], a.bytes()))
        return refuse(c, a, "two outputs are the same array or overlap");
  return 1;
}

int MemberBatch::build(mifc_ctx* c, const MemberBatchCall& a, bool with_none, float* const* out_host, int nout, size_t n_counts)
{
  const size_t nlev = (size_t)a.nlev;
  words = a.nmem > 64 ? (a.nmem + 63) / 64 : 1;
  out_host_ = out_host;
  if (!host_memory(c, [&] {
        all.assign(nlev * (size_t)words, 0ull);
        none.assign(with_none ? all.size() : 0, 0ull);
        ndef.assign(with_none ? nlev : 0, a.nmem);
        mem.assign(a.fields, a.fields + a.nmem);
        out.assign(out_host, out_host + nout);
        counts_.resize(n_counts);
      }))
    return 0;
  for (int j = 0; a.fdefined_in && j < a.nmem; ++j)
    for (size_t l = 0; l < nlev; ++l) {
      const int f = a.fdefined_in[(size_t)j * nlev + l];
      const size_t w = l * (size_t)words + (size_t)(j >> 6);
      if (f == MIFC_ALL_DEFINED)
        all[w] |= 1ull << (j & 63);
      if (with_none && f == MIFC_NONE_DEFINED) {
        none[w] |= 1ull << (j & 63);
        ndef[l] -= 1;
      }
    }
  return 1;
}

int MemberBatch::place(mifc_ctx* c, Staging& st, const MemberBatchCall& a, size_t budget, bool cells_by_4)
{
  lev_chunk = (size_t)a.nlev;
  cell_chunk = a.cells();
  if (a.memkind == MIFC_MEM_HOST) {
    plan_level_chunks(budget, a.cells(), (mem.size() + out.size()) * sizeof(float), (size_t)a.nlev, &lev_chunk, &cell_chunk);
    if (cells_by_4 && cell_chunk < a.cells() && cell_chunk >= 4)
      cell_chunk &= ~(size_t)3; // every range but the last keeps the 16-byte form
    const size_t S = align_up(lev_chunk * cell_chunk, 64);
    const float* d_mem = mem.empty() ? nullptr : static_cast<const float*>(st.scratch(mem.size() * S * sizeof(float)));
    float* d_out = static_cast<float*>(st.scratch(out.size() * S * sizeof(float)));
    if (!st.ok())
      return 0;
    for (size_t j = 0; j < mem.size(); ++j)
      mem[j] = d_mem + j * S;
    for (size_t k = 0; k < out.size(); ++k)
      out[k] = d_out + k * S;
  }
  auto on_grid = [](const float* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
  aligned = std::all_of(mem.begin(), mem.end(), on_grid) && std::all_of(out.begin(), out.end(), on_grid);
  return 1;
}

int MemberBatch::finish(mifc_ctx* c, Staging& st)
{
  MIFC_HIP(c, hipMemcpyAsync(counts_.data(), c->d_counts, counts_.size() * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  return st.finish() ? 1 : 0;
}

int upload_table(mifc_ctx* c, Staging& st, std::vector<unsigned char>& host, std::initializer_list<Section> sections,
                 const unsigned char** dev)
{
  size_t end = 0;
  for (const Section& s : sections)
    end = align_up(end, 16) + s.second;
  unsigned char* d = host_memory(c, [&] { host.assign(end, 0); }) ? static_cast<unsigned char*>(st.scratch(end)) : nullptr;
  if (!d)
    return 0;
  end = 0;
  for (const Section& s : sections) {
    const size_t at = align_up(end, 16);
    if (s.second)
      std::memcpy(host.data() + at, s.first, s.second);
    *dev++ = d + at;
    end = at + s.second;
  }
  MIFC_HIP(c, hipMemcpyAsync(d, host.data(), end, hipMemcpyHostToDevice, c->stream));
  return 1;
}

} // namespace mifc_host

extern "C" const char* mifc_last_ensemble_form(void)
{
  using mifc_host::EnsembleForm;
  const EnsembleForm& f = mifc_host::t_form;
  char* const text = mifc_host::t_form_text;
  const size_t room = sizeof mifc_host::t_form_text;
  int at = 0;
  if (f.entry == EnsembleForm::NONE)
    return "";
  if (f.entry == EnsembleForm::SINGLE)
    at = std::snprintf(text, room, "entry=single c=%d tail=%d", f.c, f.tail);
  else if (f.entry == EnsembleForm::LEVELS)
    at = std::snprintf(text, room, "entry=levels c=%d welford=%d flagged=%d np=%d", f.c, f.welford, f.flagged, f.np);
  else
    at = std::snprintf(text, room, "entry=quantiles tier=%d", f.tier);
  std::snprintf(text + at, room - (size_t)at, " inline=%d launches=%d lev_chunk=%zu cell_chunk=%zu partials=%d", f.inline_args, f.launches,
                f.lev_chunk, f.cell_chunk, f.partials);
  return text;
}
