// mifc_capi_hremap.hip -- C ABI of the mifc_hremap_* entries (include/mifc.h; EXTENSION, no reference function): the plan
// object -- a caller's CSR weight table brought to the host, validated and laid out by mifc_hremap_plan.h, then uploaded
// into device memory the plan owns -- and mifc_hremap_levels, which applies it to level batches: the refusals (the head of
// the call, the overlap rule and the level table are the ones of mifc_levelbatch.h, without a coordinate), the passes
// over the fields, four per launch of the kernel of mifc_hremap.hip, two where values are tested, and, for host memory, the chunks of levels.
// A destination may need any cell of a level, so host batches are staged whole levels at a time, as mifc_capi_hinterp.hip
// does: per chunk L levels of every field go up, the launches run and L * ndst values per field come down.
#include "mifc_hremap_plan.h"
#include "mifc_levelbatch.h"

#include <cmath>
#include <cstdio>
#include <new>

using namespace mifc_host;

static_assert(MIFC_HREMAP_STRICT == mifc::HREMAP_STRICT && MIFC_HREMAP_RENORM == mifc::HREMAP_RENORM, "HremapParams::mode");

struct mifc_hremap_plan
{
  mifc_ctx* ctx = nullptr;
  int nsrc = 0, ndst = 0, nslices = 0, max_row = 0, empty_rows = 0, max_width = 0;
  long long nnz = 0;
  unsigned char* dev = nullptr; // one block: slice_off | slice_width | len | wall | entries
  const u64* slice_off = nullptr;
  const int *slice_width = nullptr, *len = nullptr;
  const double* wall = nullptr;
  const void* entries = nullptr;
};

namespace {

// mifc_last_hremap_form: the shape of the calling thread's last launch and the launches of its call
struct HremapForm
{
  int mode = -1, nf = 0, tested = 0, blocks = 0, level_chunks = 0, chunk = 0, width = 0, launches = 0;
};
thread_local HremapForm t_form;
thread_local char t_form_text[192];

// The levels of a staged chunk of a host-memory call: what fits `budget` bytes of device memory with every field's
// input levels and output levels in it, but never less than one level.
size_t levels_per_chunk(size_t budget, size_t nfields, size_t cells, size_t ndst, size_t nlev)
{
  const size_t per_level = nfields * (cells + ndst) * sizeof(float);
  return std::max<size_t>(1, std::min<size_t>(nlev, budget / per_level));
}

mifc_hremap_plan* no_plan(mifc_ctx* c, const std::string& why)
{
  c->err = "mifc_hremap_plan_create: " + why;
  return nullptr;
}

// n items of the caller's, wherever they live, into `to` (behind whatever the caller queued on the context's stream)
template <class T>
bool to_host(mifc_ctx* c, std::vector<T>& to, const T* from, size_t n, int memkind)
{
  to.resize(n);
  if (n == 0)
    return true;
  if (memkind == MIFC_MEM_HOST) {
    std::memcpy(to.data(), from, n * sizeof(T));
    return true;
  }
  const hipError_t e = hipMemcpy(to.data(), from, n * sizeof(T), hipMemcpyDeviceToHost);
  return e == hipSuccess || fail(c, "hipMemcpy (the table to the host)", e);
}

mifc_hremap_plan* create(mifc_ctx* c, int nsrc, int ndst, const int* rowptr, const int* col, const float* w, int memkind)
{
  if (c->capturing)
    return no_plan(c, "not available while a mifc_graph capture is open");
  if (memkind != MIFC_MEM_HOST && memkind != MIFC_MEM_DEVICE)
    return no_plan(c, "unknown memkind " + std::to_string(memkind));
  if (!rowptr)
    return no_plan(c, "a null pointer (rowptr, col or w)");
  if (nsrc < 1 || ndst < 1)
    return no_plan(c, "nsrc < 1 or ndst < 1");
  if (memkind == MIFC_MEM_DEVICE && hipStreamSynchronize(c->stream) != hipSuccess)
    return no_plan(c, "the context's stream could not be synchronised");
  std::vector<int> h_rowptr, h_col;
  std::vector<float> h_w;
  mifc::HremapLayout L;
  if (!to_host(c, h_rowptr, rowptr, (size_t)ndst + 1, memkind))
    return nullptr;
  long long nnz = 0;
  std::string why = mifc::hremap_check_rows(nsrc, ndst, h_rowptr.data(), &nnz);
  if (!why.empty())
    return no_plan(c, why);
  if (nnz > 0 && (!col || !w)) // (a table without entries has no col and no w to point to)
    return no_plan(c, "a null pointer (rowptr, col or w)");
  if (!to_host(c, h_col, col, (size_t)nnz, memkind) || !to_host(c, h_w, w, (size_t)nnz, memkind))
    return nullptr;
  why = mifc::hremap_check_entries(nsrc, nnz, h_col.data(), h_w.data());
  if (!why.empty())
    return no_plan(c, why);
  mifc::hremap_layout(nsrc, ndst, h_rowptr.data(), h_col.data(), h_w.data(), L);

  mifc_hremap_plan* p = new mifc_hremap_plan;
  p->ctx = c;
  p->nsrc = nsrc;
  p->ndst = ndst;
  p->nslices = L.nslices;
  p->max_row = L.max_row;
  p->empty_rows = L.empty_rows;
  p->max_width = L.max_width;
  p->nnz = L.nnz;
  const size_t padded = (size_t)L.nslices * mifc::HREMAP_SLICE;
  const size_t o_width = align_up((size_t)L.nslices * sizeof(u64), 16), o_len = o_width + align_up((size_t)L.nslices * sizeof(int), 16);
  const size_t o_wall = o_len + align_up(padded * sizeof(int), 16), o_entries = o_wall + align_up(padded * sizeof(double), 16);
  const size_t bytes = o_entries + std::max<size_t>(L.entries.size(), 1) * sizeof(mifc::HremapEntry);
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&p->dev), bytes);
  if (e == hipSuccess)
    e = hipMemcpy(p->dev, L.slice_off.data(), (size_t)L.nslices * sizeof(u64), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(p->dev + o_width, L.slice_width.data(), (size_t)L.nslices * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(p->dev + o_len, L.len.data(), padded * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy(p->dev + o_wall, L.wall.data(), padded * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess && !L.entries.empty())
    e = hipMemcpy(p->dev + o_entries, L.entries.data(), L.entries.size() * sizeof(mifc::HremapEntry), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    fail(c, "hipMalloc / hipMemcpy (the plan's tables)", e);
    if (p->dev)
      (void)hipFree(p->dev);
    delete p;
    return nullptr;
  }
  p->slice_off = reinterpret_cast<const u64*>(p->dev);
  p->slice_width = reinterpret_cast<const int*>(p->dev + o_width);
  p->len = reinterpret_cast<const int*>(p->dev + o_len);
  p->wall = reinterpret_cast<const double*>(p->dev + o_wall);
  p->entries = p->dev + o_entries;
  return p;
}

} // namespace

extern "C" {

mifc_hremap_plan* mifc_hremap_plan_create(mifc_ctx* c, int nsrc, int ndst, const int* rowptr, const int* col, const float* w, int memkind)
{
  if (!c)
    return nullptr;
  enter(c);
  try { // nothing may be thrown across the C ABI
    return create(c, nsrc, ndst, rowptr, col, w, memkind);
  } catch (...) {
    c->err = "mifc_hremap_plan_create: out of host memory";
    return nullptr;
  }
}

void mifc_hremap_plan_destroy(mifc_hremap_plan* p)
{
  if (!p)
    return;
  enter(p->ctx);
  (void)hipStreamSynchronize(p->ctx->stream); // (a device call may still read the tables)
  (void)hipFree(p->dev);
  delete p;
}

int mifc_hremap_plan_info(const mifc_hremap_plan* p, long long* nnz, int* max_row, int* empty_rows)
{
  if (!p)
    return 0;
  if (nnz)
    *nnz = p->nnz;
  if (max_row)
    *max_row = p->max_row;
  if (empty_rows)
    *empty_rows = p->empty_rows;
  return 1;
}

int mifc_hremap_levels(mifc_ctx* c, const mifc_hremap_plan* plan, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in,
                       int nfields, int mode, double min_frac, float* const* fres, int* fdefined_out, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  // (the head of a level-batch call without a coordinate: what the shared checks and the level table read)
  const LevelBatchCall a = {"mifc_hremap_levels", COORD_LEVELS, nx, ny, nlev, fields, fdefined_in, nfields, nullptr, MIFC_SOME_DEFINED, nullptr,
                            nullptr, nullptr, undef, memkind};
  if (c->capturing)
    return refuse(c, a, "not available while a mifc_graph capture is open");
  if (!plan)
    return refuse(c, a, "a null plan");
  if (plan->ctx != c)
    return refuse(c, a, "the plan belongs to another context");
  if (nlev < 1)
    return refuse(c, a, "nlev < 1");
  if (nfields < 1 || nfields > mifc::HREMAP_MAX_FIELDS)
    return refuse(c, a, "nfields " + std::to_string(nfields) + " outside 1.." + std::to_string(mifc::HREMAP_MAX_FIELDS));
  if (nx < 1 || ny < 1 || (long long)nx * (long long)ny != (long long)plan->nsrc)
    return refuse(c, a, "nx * ny is not the plan's nsrc " + std::to_string(plan->nsrc));
  if (!check_grid(c, a)) // memkind
    return 0;
  if (mode != MIFC_HREMAP_STRICT && mode != MIFC_HREMAP_RENORM)
    return refuse(c, a, "unknown mode " + std::to_string(mode));
  if (!(min_frac >= 0.0 && min_frac <= 1.0))
    return refuse(c, a, "min_frac is NaN or outside [0, 1]");
  if (!fields || !fres || !fdefined_out)
    return refuse(c, a, "a null pointer (fields, fres or fdefined_out)");
  if (!check_field_pointers(c, a, fres))
    return 0;
  const int nf = nfields;
  const size_t cells = a.cells(), ndst = (size_t)plan->ndst, levels = (size_t)nlev;
  if (!check_overlaps(c, a, {{fres, nf, levels * ndst * sizeof(float), "fres"}}))
    return 0;

  // one counter per field and level
  const size_t n_counts = (size_t)nf * levels;
  LevelTable tab;
  Staging st(c, memkind);
  if (!tab.build(c, a, n_counts) || !tab.upload(c, st))
    return 0;
  bool tested = false;
  for (size_t j = 0; j < n_counts; ++j)
    tested |= !fdefined_in || fdefined_in[j] != MIFC_ALL_DEFINED;

  mifc::HremapParams P;
  std::memset(&P, 0, sizeof P);
  P.mode = mode;
  P.ndst = plan->ndst;
  P.nslices = plan->nslices;
  P.call_nlev = nlev;
  P.tested = tested ? 1 : 0;
  P.undef = undef;
  P.min_frac = min_frac;
  P.in_stride = (long)cells;
  P.out_stride = (long)ndst;
  P.slice_off = plan->slice_off;
  P.slice_width = plan->slice_width;
  P.len = plan->len;
  P.wall = plan->wall;
  P.entries = plan->entries;
  P.lev_bits = tab.lev_bits();
  P.n_undefined = tab.n_undefined();

  // host memory: L levels of every field in, L levels of every output, in one block
  const bool host = memkind == MIFC_MEM_HOST;
  const size_t L = host ? levels_per_chunk((size_t)(mifc::env().hremap_chunk_mib > 0 ? mifc::env().hremap_chunk_mib : 256) << 20, (size_t)nf, cells,
                                           ndst, levels)
                        : levels;
  float* staged = nullptr;
  if (host) {
    staged = static_cast<float*>(st.scratch((size_t)nf * L * (cells + ndst) * sizeof(float)));
    if (!st.ok())
      return 0;
  }
  const int pass = mifc::hremap_pass_fields(tested);
  HremapForm form;
  form.mode = mode;
  form.tested = P.tested;
  form.nf = std::min(pass, nf);
  form.width = plan->max_width;
  for (size_t k0 = 0; k0 < levels; k0 += L) {
    const size_t n = std::min(L, levels - k0);
    const float* in[mifc::HREMAP_MAX_FIELDS];
    float* out[mifc::HREMAP_MAX_FIELDS];
    for (int f = 0; f < nf; ++f) {
      if (host) {
        float* d = staged + (size_t)f * L * cells;
        MIFC_HIP(c, hipMemcpyAsync(d, fields[f] + k0 * cells, n * cells * sizeof(float), hipMemcpyHostToDevice, c->stream));
        in[f] = d;
        out[f] = staged + (size_t)nf * L * cells + (size_t)f * L * ndst;
      } else {
        in[f] = fields[f];
        out[f] = fres[f];
      }
    }
    P.nlev = (int)n;
    P.lev0 = (int)k0;
    const mifc::HremapShape shape = mifc::hremap_shape(P.nslices, P.nlev, std::min(pass, nf), tested);
    P.chunk = shape.chunk;
    for (int f0 = 0; f0 < nf; f0 += pass) {
      P.f0 = f0;
      P.nfields = std::min(pass, nf - f0);
      for (int f = 0; f < P.nfields; ++f) {
        P.fields[f] = in[f0 + f];
        P.out[f] = out[f0 + f];
      }
      MIFC_LAUNCH(c, mifc::launch_hremap(P, c->stream));
      form.launches += 1;
    }
    form.blocks = shape.blocks;
    form.level_chunks = shape.level_chunks;
    form.chunk = shape.chunk;
    if (host)
      for (int f = 0; f < nf; ++f)
        MIFC_HIP(c, hipMemcpyAsync(fres[f] + k0 * ndst, out[f], n * ndst * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  if (!tab.read_counts(c) || !st.finish()) // finish(): the one synchronisation of the call
    return 0;
  t_form = form;
  for (size_t j = 0; j < n_counts; ++j) // (the kernel counts the destinations that have a row; the empty rows are the plan's)
    fdefined_out[j] = mifc_classify(tab.count(j) + (u64)plan->empty_rows, (u64)ndst);
  return 1;
}

const char* mifc_last_hremap_form(void)
{
  static const char* const names[] = {"strict", "renorm"};
  const HremapForm& f = t_form;
  if (f.mode < 0)
    return "";
  std::snprintf(t_form_text, sizeof t_form_text, "mode=%s nf=%d tested=%d blocks=%d level_chunks=%d chunk=%d width=%d launches=%d", names[f.mode], f.nf,
                f.tested, f.blocks, f.level_chunks, f.chunk, f.width, f.launches);
  return t_form_text;
}

} // extern "C"
