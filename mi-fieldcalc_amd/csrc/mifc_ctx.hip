// mifc_ctx.hip -- what mifc_ctx.h declares: the context's error text, its per-level scratch and pinned
// mirror, and the per-call staging of host fields through the context's scratch slots.
#include "mifc_ctx.h"

#include <cstdio>

namespace mifc_host {

bool fail(mifc_ctx* c, const char* what, hipError_t e)
{
  char buf[256];
  std::snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
  if (c)
    c->err = buf;
  return false;
}


bool ensure_levels(mifc_ctx* c, size_t nlev)
{
  if (c->cap_lev >= nlev)
    return true;
  hipError_t e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess)
    return fail(c, "hipStreamSynchronize", e);
  if (c->d_flags)
    (void)hipFree(c->d_flags);
  if (c->d_counts)
    (void)hipFree(c->d_counts);
  if (c->d_ab)
    (void)hipFree(c->d_ab);
  if (c->d_levels)
    (void)hipFree(c->d_levels);
  if (c->h_pinned)
    (void)hipHostFree(c->h_pinned);
  c->d_levels = nullptr;
  c->d_flags = nullptr;
  c->d_counts = nullptr;
  c->d_ab = nullptr;
  c->h_pinned = nullptr;
  c->cap_lev = 0;
  size_t cap = 256;
  while (cap < nlev)
    cap *= 2;
  if ((e = hipMalloc((void**)&c->d_flags, 2 * cap)) != hipSuccess)
    return fail(c, "hipMalloc(flags)", e);
  if ((e = hipMalloc((void**)&c->d_counts, 5 * cap * sizeof(u64))) != hipSuccess)
    return fail(c, "hipMalloc(counts)", e);
  if ((e = hipMalloc((void**)&c->d_ab, 2 * cap * sizeof(float))) != hipSuccess)
    return fail(c, "hipMalloc(ab)", e);
  if ((e = hipMalloc((void**)&c->d_levels, cap * sizeof(int))) != hipSuccess)
    return fail(c, "hipMalloc(levels)", e);
  if ((e = hipHostMalloc(&c->h_pinned, 5 * cap * sizeof(u64) + 2 * cap + 2 * cap * sizeof(float), hipHostMallocDefault)) != hipSuccess)
    return fail(c, "hipHostMalloc", e);
  c->cap_lev = cap;
  return true;
}

unsigned int* partials_for(mifc_ctx* c, size_t n_cells, int* cap)
{
  *cap = 0;
  const size_t blocks = (n_cells / 4 + 255) / 256; // one float4 per lane, 256 lanes
  if (blocks < 2048)
    return nullptr;
  if (blocks > c->partials_cap) {
    if (c->d_partials)
      (void)hipFree(c->d_partials);
    c->d_partials = nullptr;
    c->partials_cap = 0;
    if (hipMalloc((void**)&c->d_partials, blocks * sizeof(unsigned int)) != hipSuccess)
      return nullptr; // the launch then counts with one atomic per workgroup
    c->partials_cap = blocks;
  }
  *cap = (int)c->partials_cap;
  return c->d_partials;
}

bool pinned_acquire(mifc_ctx* c)
{
  if (c->pinned_read_pending) {
    hipError_t e = hipEventSynchronize(c->pinned_read);
    if (e != hipSuccess)
      return fail(c, "hipEventSynchronize", e);
    c->pinned_read_pending = false;
  }
  return true;
}

bool pinned_release(mifc_ctx* c)
{
  hipError_t e = hipEventRecord(c->pinned_read, c->stream);
  if (e != hipSuccess)
    return fail(c, "hipEventRecord", e);
  c->pinned_read_pending = true;
  return true;
}

bool scratch_release(mifc_ctx* c)
{
  if (c->capturing && c->n_lanes > 1) {
    // the context's per-level scratch (flags, hybrid coefficients) is ONE set: calls recorded side by side would overwrite it
    // under each other's kernels
    c->err = "a call that needs the context's per-level scratch was recorded into a capture with several lanes: record level batches of at most 8 "
             "levels (their flags and coefficients travel in the kernel arguments), or use one lane";
    return false;
  }
  hipError_t e = hipEventRecord(c->scratch_read, c->stream);
  if (e != hipSuccess)
    return fail(c, "hipEventRecord", e);
  c->scratch_read_pending = true;
  return true;
}

u64* pinned_counts(mifc_ctx* c)
{
  return reinterpret_cast<u64*>(c->h_pinned);
}
unsigned char* pinned_flags(mifc_ctx* c)
{
  return reinterpret_cast<unsigned char*>(c->h_pinned) + 5 * c->cap_lev * sizeof(u64);
}
float* pinned_ab(mifc_ctx* c)
{
  return reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(c->h_pinned) + 5 * c->cap_lev * sizeof(u64) + 2 * c->cap_lev);
}

// ---- staging ------------------------------------------------------------------
// The context's next slot, at least `bytes` large.  Growing a slot synchronises the stream and frees only
// that slot: copies already enqueued into the other slots of the call stay valid.
void* Staging::take(size_t bytes)
{
  mifc_ctx* c = c_;
  if (c->slot_cursor == c->slot.size()) {
    try { // nothing may be thrown across the C ABI
      c->slot.push_back({nullptr, 0});
    } catch (...) {
      c->err = "out of host memory";
      ok_ = false;
      return nullptr;
    }
  }
  mifc_ctx::Slot& s = c->slot[c->slot_cursor++];
  if (s.bytes >= bytes)
    return s.ptr;
  if (s.ptr) {
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
      ok_ = fail(c, "hipStreamSynchronize", e);
      return nullptr;
    }
    (void)hipFree(s.ptr);
    s.ptr = nullptr;
    s.bytes = 0;
  }
  const size_t want = align_up(bytes, 256);
  hipError_t e = hipMalloc(&s.ptr, want);
  if (e != hipSuccess) {
    s.ptr = nullptr;
    ok_ = fail(c, "hipMalloc(scratch)", e);
    return nullptr;
  }
  s.bytes = want;
  return s.ptr;
}

void* Staging::scratch(size_t bytes)
{
  return take(bytes);
}

const float* Staging::in(const float* p, size_t n)
{
  if (!p || memkind_ == MIFC_MEM_DEVICE)
    return p;
  for (const mifc_ctx::HeldField& h : c_->held)
    if (h.host == p && h.n >= n)
      return h.dev; // declared constant by the caller: already resident
  void* d = take(n * sizeof(float));
  if (!ok_)
    return nullptr;
  hipError_t e = hipMemcpyAsync(d, p, n * sizeof(float), hipMemcpyHostToDevice, c_->stream);
  if (e != hipSuccess) {
    ok_ = fail(c_, "hipMemcpyAsync(H2D)", e);
    return nullptr;
  }
  return static_cast<const float*>(d);
}

float* Staging::out(float* p, size_t n, bool preload)
{
  if (!p || memkind_ == MIFC_MEM_DEVICE)
    return p;
  if (n_out_ == MAX_OUT) {
    c_->err = "staging: more host outputs than one call can carry";
    ok_ = false;
    return nullptr;
  }
  void* d = take(n * sizeof(float));
  if (!ok_)
    return nullptr;
  if (preload) {
    hipError_t e = hipMemcpyAsync(d, p, n * sizeof(float), hipMemcpyHostToDevice, c_->stream);
    if (e != hipSuccess) {
      ok_ = fail(c_, "hipMemcpyAsync(H2D)", e);
      return nullptr;
    }
  }
  outs_[n_out_++] = {p, d, n};
  return static_cast<float*>(d);
}

bool Staging::finish()
{
  for (int k = 0; k < n_out_; ++k) {
    hipError_t e = hipMemcpyAsync(outs_[k].host, outs_[k].dev, outs_[k].n * sizeof(float), hipMemcpyDeviceToHost, c_->stream);
    if (e != hipSuccess)
      return fail(c_, "hipMemcpyAsync(D2H)", e);
  }
  hipError_t e = hipStreamSynchronize(c_->stream);
  if (e != hipSuccess)
    return fail(c_, "hipStreamSynchronize(c->stream)", e);
  return true;
}

void free_slots(mifc_ctx* c)
{
  for (const mifc_ctx::Slot& s : c->slot)
    if (s.ptr)
      (void)hipFree(s.ptr);
  c->slot.clear();
}

} // namespace mifc_host
