// mifc_capi.hip -- the part of the extern "C" boundary (include/mifc.h) that is not an operator: the context's
// lifecycle and environment, streams, device memory and held host fields, the counter mode and classification, the
// level stride of padded batches, the halo copy, and the measurement build's own entries.
//
// The operators live in one mifc_capi_<family>.hip each (pointwise, stencil, derived, catalogue, neighbour, icing,
// quantile, ensemble, vinterp, vlayer, vderiv); what they share is in mifc_ctx.h.  Host-side logic only, here as there:
// argument validation exactly as the reference does it (what makes an operator `return false`), staging of legacy host
// pointers through device scratch, launching the HIP kernels and turning the per-field undefined counts into
// ValuesDefined flags.  There is no CPU compute path: every operator body runs on the GPU.

#include <new>
#include <string>

#include "mifc_ctx.h"

using namespace mifc_host;

extern "C" {

int mifc_abi_version(void)
{
  return MIFC_ABI_VERSION;
}

int mifc_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess)
    return 0;
  return n;
}

mifc_ctx* mifc_create(int device)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n)
    return nullptr;
  if (hipSetDevice(device) != hipSuccess)
    return nullptr;
  mifc_ctx* c = new (std::nothrow) mifc_ctx();
  if (!c)
    return nullptr;
  c->device = device;
  if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return nullptr;
  }
  c->stream = c->own_stream;
  if (hipEventCreateWithFlags(&c->pinned_read, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->scratch_read, hipEventDisableTiming) != hipSuccess) {
    if (c->pinned_read)
      (void)hipEventDestroy(c->pinned_read);
    (void)hipStreamDestroy(c->own_stream);
    delete c;
    return nullptr;
  }
  mifc::env_reload(); // the tuning / diagnostic environment is read here, never on a launch path
  return c;
}

int mifc_reload_env(mifc_ctx* c)
{
  if (!c)
    return 0;
  mifc::env_reload();
  return 1;
}

void mifc_destroy(mifc_ctx* c)
{
  if (!c)
    return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  (void)mifc_comm_release(c); // a communicator the library created goes with the context
  free_slots(c);
  if (c->d_flags)
    (void)hipFree(c->d_flags);
  if (c->d_counts)
    (void)hipFree(c->d_counts);
  if (c->d_ab)
    (void)hipFree(c->d_ab);
  if (c->d_partials)
    (void)hipFree(c->d_partials);
  if (c->d_levels)
    (void)hipFree(c->d_levels);
  if (c->h_pinned)
    (void)hipHostFree(c->h_pinned);
  if (c->pinned_read)
    (void)hipEventDestroy(c->pinned_read);
  if (c->scratch_read)
    (void)hipEventDestroy(c->scratch_read);
  for (hipEvent_t e : c->tev)
    if (e)
      (void)hipEventDestroy(e);
  mifc::hostpipe_destroy(c->pipe);
  for (const mifc_ctx::HeldField& h : c->held)
    (void)hipFree(h.dev);
  if (c->capture_stream)
    (void)hipStreamDestroy(c->capture_stream);
  if (c->own_stream)
    (void)hipStreamDestroy(c->own_stream);
  delete c;
}

const char* mifc_last_error(const mifc_ctx* c)
{
  return c ? c->err.c_str() : "no context (no usable HIP device)";
}

// Work already queued on the old stream may still read the context's device scratch (per-level
// flags, hybrid coefficients of an *_enqueue call): the new stream waits for it before anything
// issued there can rewrite that scratch.
static int switch_stream(mifc_ctx* c, hipStream_t s)
{
  if (s == c->stream)
    return 1;
  if (c->scratch_read_pending)
    MIFC_HIP(c, hipStreamWaitEvent(s, c->scratch_read, 0));
  c->stream = s;
  return 1;
}

int mifc_set_stream(mifc_ctx* c, void* hip_stream)
{
  CTX_OR_FAIL(c);
  if (c->capturing) {
    c->err = "mifc_set_stream: a graph capture is open on this context (mifc_graph_begin)";
    return 0;
  }
  return switch_stream(c, static_cast<hipStream_t>(hip_stream)); // null = HIP's default stream
}

int mifc_use_own_stream(mifc_ctx* c)
{
  CTX_OR_FAIL(c);
  if (c->capturing) {
    c->err = "mifc_use_own_stream: a graph capture is open on this context (mifc_graph_begin)";
    return 0;
  }
  return switch_stream(c, c->own_stream);
}

int mifc_not_built(mifc_ctx* c, const char* what)
{
  if (c)
    c->err = std::string(what ? what : "?") + ": not built on the GPU (outside the hot-path scope; there is no CPU fallback)";
  return 0;
}

int mifc_synchronize(mifc_ctx* c)
{
  CTX_OR_FAIL(c);
  MIFC_HIP(c, hipStreamSynchronize(c->stream));
  return 1;
}

void* mifc_device_alloc(mifc_ctx* c, size_t bytes)
{
  if (!c)
    return nullptr;
  void* p = nullptr;
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) {
    fail(c, "hipMalloc", e);
    return nullptr;
  }
  return p;
}

int mifc_device_free(mifc_ctx* c, void* dptr)
{
  CTX_OR_FAIL(c);
  MIFC_HIP(c, hipFree(dptr));
  return 1;
}

int mifc_copy_to_device(mifc_ctx* c, void* dst_dev, const void* src_host, size_t bytes)
{
  CTX_OR_FAIL(c);
  MIFC_HIP(c, hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, c->stream));
  MIFC_HIP(c, hipStreamSynchronize(c->stream));
  return 1;
}

int mifc_copy_to_host(mifc_ctx* c, void* dst_host, const void* src_dev, size_t bytes)
{
  CTX_OR_FAIL(c);
  MIFC_HIP(c, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, c->stream));
  MIFC_HIP(c, hipStreamSynchronize(c->stream));
  return 1;
}

// Constant host fields (map ratios, Coriolis parameter): a caller that passes
// the same host array to many calls declares it once; host-pointer calls then
// find the device copy instead of uploading it again.  The caller promises not
// to change the content while it is held (there is no cheap way to notice: a
// checksum of the field costs more host time than the upload it would save).
int mifc_hold_field(mifc_ctx* c, const float* host_field, size_t n_floats)
{
  if (!c || !host_field || n_floats == 0)
    return 0;
  enter(c);
  for (mifc_ctx::HeldField& h : c->held) {
    if (h.host == host_field) { // refresh (content or size may have changed)
      if (h.n < n_floats) {
        MIFC_HIP(c, hipStreamSynchronize(c->stream));
        (void)hipFree(h.dev);
        h.dev = nullptr;
        h.n = 0;
        MIFC_HIP(c, hipMalloc((void**)&h.dev, n_floats * sizeof(float)));
        h.n = n_floats;
      }
      MIFC_HIP(c, hipMemcpyAsync(h.dev, host_field, n_floats * sizeof(float), hipMemcpyHostToDevice, c->stream));
      MIFC_HIP(c, hipStreamSynchronize(c->stream));
      return 1;
    }
  }
  mifc_ctx::HeldField h = {host_field, n_floats, nullptr};
  MIFC_HIP(c, hipMalloc((void**)&h.dev, n_floats * sizeof(float)));
  hipError_t e = hipMemcpyAsync(h.dev, host_field, n_floats * sizeof(float), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess)
    e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    (void)hipFree(h.dev);
    fail(c, "mifc_hold_field", e);
    return 0;
  }
  c->held.push_back(h);
  return 1;
}

int mifc_release_field(mifc_ctx* c, const float* host_field)
{
  CTX_OR_FAIL(c);
  for (size_t k = 0; k < c->held.size(); ++k) {
    if (c->held[k].host == host_field) {
      MIFC_HIP(c, hipStreamSynchronize(c->stream));
      (void)hipFree(c->held[k].dev);
      c->held.erase(c->held.begin() + (long)k);
      return 1;
    }
  }
  return 0;
}

#ifdef MIFC_MEASUREMENT_BUILD // libmifc_measure.so only (include/mifc_measure.h)
// Measurement aid: between begin and end every kernel launch of this context is bracketed by a
// HIP event pair on its launch stream; end returns the summed kernel time in milliseconds
// (-1 on error, or when more than 16 launches happened in between).
int mifc_timing_begin(mifc_ctx* c)
{
  CTX_OR_FAIL(c);
  for (hipEvent_t& e : c->tev)
    if (!e)
      MIFC_HIP(c, hipEventCreate(&e));
  c->n_timed = 0;
  c->timing = true;
  return 1;
}

float mifc_timing_end_ms(mifc_ctx* c)
{
  if (!c || !c->timing)
    return -1.f;
  c->timing = false;
  float total = 0.f;
  for (int k = 0; k < c->n_timed; ++k) {
    float ms = 0.f;
    if (hipEventSynchronize(c->tev[2 * k + 1]) != hipSuccess || hipEventElapsedTime(&ms, c->tev[2 * k], c->tev[2 * k + 1]) != hipSuccess)
      return -1.f;
    total += ms;
  }
  return c->n_timed >= mifc_ctx::NTIMED ? -1.f : total;
}
#endif // MIFC_MEASUREMENT_BUILD

int mifc_counts_accumulate(mifc_ctx* c, int on)
{
  if (!c)
    return 0;
  c->counts_accumulate = on != 0;
  return 1;
}

int mifc_zero_counts_enqueue(mifc_ctx* c, unsigned long long* counts_dev, size_t n)
{
  if (!c || !counts_dev)
    return 0;
  enter(c);
  if (n)
    MIFC_HIP(c, hipMemsetAsync(counts_dev, 0, n * sizeof(u64), c->stream));
  return 1;
}

int mifc_classify(unsigned long long n_undefined, unsigned long long n)
{
  if (n_undefined == 0)
    return MIFC_ALL_DEFINED;
  if (n_undefined == n)
    return MIFC_NONE_DEFINED;
  return MIFC_SOME_DEFINED;
}

size_t mifc_batch_level_stride(int nx, int ny)
{
  if (nx <= 0 || ny <= 0)
    return 0;
  return mifc::padded_level_stride((size_t)nx * (size_t)ny);
}

int mifc_halo_copy_enqueue(mifc_ctx* dst_ctx, float* dst_dev, mifc_ctx* src_ctx, const float* src_dev, size_t n_floats)
{
  if (!dst_ctx || !src_ctx || !dst_dev || !src_dev)
    return 0;
  enter(src_ctx);
  if (n_floats == 0)
    return 1;
  // the rows must have been produced: order the copy after what is queued on the source context's stream
  if (src_ctx != dst_ctx || src_ctx->stream != dst_ctx->stream) {
    hipEvent_t ready = nullptr;
    MIFC_HIP(src_ctx, hipEventCreateWithFlags(&ready, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ready, src_ctx->stream);
    enter(dst_ctx);
    if (e == hipSuccess)
      e = hipStreamWaitEvent(dst_ctx->stream, ready, 0);
    (void)hipEventDestroy(ready); // released once the wait has consumed it
    if (e != hipSuccess) {
      fail(dst_ctx, "halo copy: event", e);
      return 0;
    }
  }
  enter(dst_ctx);
  if (src_ctx->device == dst_ctx->device)
    MIFC_HIP(dst_ctx, hipMemcpyAsync(dst_dev, src_dev, n_floats * sizeof(float), hipMemcpyDeviceToDevice, dst_ctx->stream));
  else
    MIFC_HIP(dst_ctx, hipMemcpyPeerAsync(dst_dev, dst_ctx->device, src_dev, src_ctx->device, n_floats * sizeof(float), dst_ctx->stream));
  return 1;
}

#ifdef MIFC_MEASUREMENT_BUILD // libmifc_measure.so only (include/mifc_measure.h)
int mifc_bench_stream2(mifc_ctx* c, int variant, int blocks, float* dst0, float* dst1, const float* src0, const float* src1, size_t n_floats)
{
  CTX_OR_FAIL(c);
  if (n_floats % 4 != 0)
    return 0;
  MIFC_HIP(c, mifc::launch_stream2(variant, blocks, dst0, dst1, src0, src1, n_floats, c->stream));
  return 1;
}

int mifc_diag_division(mifc_ctx* c, const float* a, const float* b, const float* g, float* shared, float* plain, size_t n)
{
  CTX_OR_FAIL(c);
  MIFC_HIP(c, mifc::launch_division_check(a, b, g, shared, plain, n, c->stream));
  return 1;
}
#endif // MIFC_MEASUREMENT_BUILD

} // extern "C"
