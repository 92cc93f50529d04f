// mifc_capi_derived.hip -- the extern "C" boundary of the fused derived variables on hybrid levels (mifc_derived.hip):
// wind speed and direction, hleveltemp and two hlevelhum variants of a level batch in one launch.

#include <cstring>

#include "mifc_ctx.h"

using namespace mifc_host;

namespace {

struct DerivedRequest
{
  const float *u, *v, *t, *h, *ps;
  const float *alevel, *blevel;
  float *ff, *temp, *hum, *hum2;
  const char *temp_unit, *hum_unit, *hum2_unit;
  int temp_compute, hum_compute, hum2_compute;
  float* dd; // extension output: wind direction
};

// the batched kernel walks the cells four at a time; `entry` keeps each entry point's own wording
bool cells_in_fours(mifc_ctx* c, int nx, int ny, const char* entry)
{
  if ((nx * ny) % 4 == 0)
    return true;
  c->err = std::string(entry) + ": nx*ny must be a multiple of 4 (use the per-field operators otherwise)";
  return false;
}

// hlevelhum's remaps (:1168-1182) for one humidity output; false = the reference returns false
bool derived_hum_variant(const char* unit, int compute, int* code, float* tdconv)
{
  if (compute <= 0 || compute >= 13) // :1168
    return false;
  compute = remap_hum_compute(unit, compute); // :1174-1177
  *tdconv = hum_tdconv(compute);              // :1181
  *code = 1 + hum_kind_ah(compute) + 4 * ((compute % 2 == 0) ? 1 : 0);
  return true;
}

// Validates like the per-level reference calls would, uploads the per-level scalars and launches (or,
// with prepared_only, hands the parameters to the host pipeline).  counts_dev: u64[5 * nlev], ff | temp | hum | hum2 | dd.
int derived_common(mifc_ctx* c, int nx, int ny, int nlev, const DerivedRequest& rq, const int* fdef_wind, const int* fdef_thermo, float undef,
                   u64* counts_dev, mifc::DerivedParams* prepared_only = nullptr)
{
  if (nlev < 1 || nx * ny <= 0)
    return 0;
  if (!rq.ff && !rq.temp && !rq.hum && !rq.hum2 && !rq.dd)
    return 0;
  const bool thermo = rq.temp || rq.hum || rq.hum2;
  const bool wind = rq.ff || rq.dd;
  mifc::DerivedParams P;
  std::memset(&P, 0, sizeof P);
  if (rq.temp) {
    const int compute = remap_temp_compute(rq.temp_unit, rq.temp_compute); // :1060-1065
    if (compute < 1 || compute > 5) { // the reference leaves such cells unwritten (:1080-1090): not offered in the batched form
      c->err = "mifc_hlevel_derived_batch: temp_compute must be 1..5";
      return 0;
    }
    P.temp_compute = compute;
  }
  if (rq.hum && !derived_hum_variant(rq.hum_unit, rq.hum_compute, &P.hum_code, &P.hum_tdconv))
    return 0;
  if (rq.hum2 && !derived_hum_variant(rq.hum2_unit, rq.hum2_compute, &P.td_code, &P.td_tdconv))
    return 0;
  if (thermo) {
    for (int l = 0; l < nlev; ++l)
      if (bad_hlevel(rq.alevel[l], rq.blevel[l])) // :1070, :1170
        return 0;
  }
  if (!ensure_levels(c, (size_t)nlev))
    return 0;
  P.n = nx * ny;
  P.nlev = nlev;
  P.u = rq.u;
  P.v = rq.v;
  P.t = rq.t;
  P.h = rq.h;
  P.ps = rq.ps;
  P.ff = rq.ff;
  P.temp = rq.temp;
  P.hum = rq.hum;
  P.td = rq.hum2;
  P.dd = rq.dd;
  P.undef = undef;
  P.cnt_ff = counts_dev;
  P.cnt_temp = counts_dev + nlev;
  P.cnt_hum = counts_dev + 2 * (size_t)nlev;
  P.cnt_td = counts_dev + 3 * (size_t)nlev;
  P.cnt_dd = counts_dev + 4 * (size_t)nlev;
  // per-level scalars: a small batch carries them in the kernel arguments, a deeper one (or the host pipeline's) in the
  // context's device scratch by way of the pinned mirror
  P.n_inline = (nlev <= 8 && !prepared_only) ? 1 : 0;
  if (!P.n_inline && !pinned_acquire(c))
    return 0;
  unsigned char *wind_flag = P.wind_inline, *thermo_flag = P.thermo_inline;
  float *a = P.a_inline, *b = P.b_inline;
  if (!P.n_inline) {
    wind_flag = pinned_flags(c);
    thermo_flag = wind_flag + c->cap_lev;
    a = pinned_ab(c);
    b = a + c->cap_lev;
  }
  bool every_all = true;
  for (int l = 0; l < nlev; ++l) {
    const bool w = !wind || (fdef_wind && fdef_wind[l] == MIFC_ALL_DEFINED);
    const bool th = !thermo || (fdef_thermo && fdef_thermo[l] == MIFC_ALL_DEFINED);
    wind_flag[l] = w ? 1 : 0;
    thermo_flag[l] = th ? 1 : 0;
    a[l] = thermo ? rq.alevel[l] : 0.f;
    b[l] = thermo ? rq.blevel[l] : 0.f;
    every_all = every_all && w && th;
  }
  if (!P.n_inline) {
    MIFC_HIP(c, hipMemcpyAsync(c->d_ab, a, 2 * c->cap_lev * sizeof(float), hipMemcpyHostToDevice, c->stream));
    MIFC_HIP(c, hipMemcpyAsync(c->d_flags, wind_flag, 2 * c->cap_lev, hipMemcpyHostToDevice, c->stream));
    if (!pinned_release(c))
      return 0;
    P.alevel = c->d_ab;
    P.blevel = c->d_ab + c->cap_lev;
    P.wind_all_defined = c->d_flags;
    P.thermo_all_defined = c->d_flags + c->cap_lev;
  }
  P.every_level_all_defined = every_all ? 1 : 0;
  if (!(c->counts_accumulate && !prepared_only && counts_dev != c->d_counts)) // (accumulate mode: the caller zeroed its counters)
    MIFC_HIP(c, hipMemsetAsync(counts_dev, 0, 5 * sizeof(u64) * (size_t)nlev, c->stream));
  if (prepared_only) { // the caller launches chunk by chunk (host pipeline)
    *prepared_only = P;
  } else {
    MIFC_LAUNCH(c, mifc::launch_derived_levels(P, c->stream));
    if (!P.n_inline && !scratch_release(c)) // the kernel reads c->d_flags and c->d_ab
      return 0;
  }
  return 1;
}

void derived_flags(const u64* cnt, int nlev, size_t n, const DerivedRequest& rq, int* fdef_ff, int* fdef_temp, int* fdef_hum, int* fdef_hum2,
                   int* fdef_dd)
{
  for (int l = 0; l < nlev; ++l) {
    if (rq.ff && fdef_ff)
      fdef_ff[l] = mifc_classify(cnt[l], (u64)n);
    if (rq.temp && fdef_temp)
      fdef_temp[l] = mifc_classify(cnt[nlev + l], (u64)n);
    if (rq.hum && fdef_hum)
      fdef_hum[l] = mifc_classify(cnt[2 * (size_t)nlev + l], (u64)n);
    if (rq.hum2 && fdef_hum2)
      fdef_hum2[l] = mifc_classify(cnt[3 * (size_t)nlev + l], (u64)n);
    if (rq.dd && fdef_dd)
      fdef_dd[l] = mifc_classify(cnt[4 * (size_t)nlev + l], (u64)n);
  }
}

int derived_sync(mifc_ctx* c, int nx, int ny, int nlev, const DerivedRequest& rq0, const int* fdef_wind, const int* fdef_thermo, int* fdef_ff,
                 int* fdef_temp, int* fdef_hum, int* fdef_hum2, int* fdef_dd, float undef, int memkind)
{
  mifc::hostpipe_note_chunks(0, 0); // mifc_last_host_chunks: hostpipe_run() reports what it does
  if (nlev < 1 || nx * ny <= 0)
    return 0;
  if (!cells_in_fours(c, nx, ny, "mifc_hlevel_derived_batch"))
    return 0;
  const size_t n = (size_t)nx * ny, nb = n * (size_t)nlev;
  const bool thermo = rq0.temp || rq0.hum || rq0.hum2;
  const bool humid = rq0.hum || rq0.hum2;
  const bool wind = rq0.ff || rq0.dd;
  DerivedRequest rq = rq0;
  Staging st(c, memkind);
  // (the chunked pipeline carries four outputs; a request with the wind direction on top is staged whole)
  if (memkind == MIFC_MEM_HOST && mifc::hostpipe_chunk_levels(n, nlev) > 0 && host_pipeline_enabled() && !(rq0.dd && rq0.ff && rq0.temp && rq0.hum && rq0.hum2)) {
    // a large batch in host memory: chunks of levels stream through the device, copies
    // in both directions overlapping the kernels (mifc_hostpipe.h)
    if (!c->pipe && !(c->pipe = mifc::hostpipe_create(c->device))) {
      c->err = "host pipeline: cannot create streams";
      return 0;
    }
    rq.ps = thermo ? st.in(rq0.ps, n) : nullptr;
    if (!st.ok() || !ensure_levels(c, (size_t)nlev))
      return 0;
    mifc::DerivedParams base;
    // the host pointers are placeholders that mark which fields take part; the chunk launcher substitutes device buffers
    rq.u = wind ? rq0.u : nullptr;
    rq.v = wind ? rq0.v : nullptr;
    rq.t = thermo ? rq0.t : nullptr;
    rq.h = humid ? rq0.h : nullptr;
    if (!derived_common(c, nx, ny, nlev, rq, fdef_wind, fdef_thermo, undef, c->d_counts, &base))
      return 0;
    MIFC_HIP(c, hipStreamSynchronize(c->stream)); // ps, flags, level coefficients, zeroed counters are in place
    const float* h_in[4];
    int slot_u = -1, slot_v = -1, slot_t = -1, slot_h = -1, n_in = 0;
    if (wind) {
      slot_u = n_in;
      h_in[n_in++] = rq0.u;
      slot_v = n_in;
      h_in[n_in++] = rq0.v;
    }
    if (thermo) {
      slot_t = n_in;
      h_in[n_in++] = rq0.t;
    }
    if (humid) {
      slot_h = n_in;
      h_in[n_in++] = rq0.h;
    }
    // the (at most four) requested outputs share the pipeline's four output slots
    float* all_out[5] = {rq0.ff, rq0.temp, rq0.hum, rq0.hum2, rq0.dd};
    float* h_out[4] = {nullptr, nullptr, nullptr, nullptr};
    int out_slot[5] = {-1, -1, -1, -1, -1}, n_out = 0;
    for (int k = 0; k < 5; ++k)
      if (all_out[k]) {
        out_slot[k] = n_out;
        h_out[n_out++] = all_out[k];
      }
    const mifc::ChunkLaunch launch = [&](int l0, int nl, const float* const* d_in, float* const* d_out, hipStream_t stream) {
      mifc::DerivedParams p = base;
      p.nlev = nl;
      p.u = slot_u >= 0 ? d_in[slot_u] : nullptr;
      p.v = slot_v >= 0 ? d_in[slot_v] : nullptr;
      p.t = slot_t >= 0 ? d_in[slot_t] : nullptr;
      p.h = slot_h >= 0 ? d_in[slot_h] : nullptr;
      p.ff = out_slot[0] >= 0 ? d_out[out_slot[0]] : nullptr;
      p.temp = out_slot[1] >= 0 ? d_out[out_slot[1]] : nullptr;
      p.hum = out_slot[2] >= 0 ? d_out[out_slot[2]] : nullptr;
      p.td = out_slot[3] >= 0 ? d_out[out_slot[3]] : nullptr;
      p.dd = out_slot[4] >= 0 ? d_out[out_slot[4]] : nullptr;
      p.alevel = base.alevel + l0;
      p.blevel = base.blevel + l0;
      p.wind_all_defined = base.wind_all_defined + l0;
      p.thermo_all_defined = base.thermo_all_defined + l0;
      p.cnt_ff = base.cnt_ff + l0;
      p.cnt_temp = base.cnt_temp + l0;
      p.cnt_hum = base.cnt_hum + l0;
      p.cnt_td = base.cnt_td + l0;
      p.cnt_dd = base.cnt_dd + l0;
      return mifc::launch_derived_levels(p, stream);
    };
    if (!mifc::hostpipe_run(c->pipe, n, nlev, n_in, h_in, 4, h_out, launch, &c->err))
      return 0;
  } else {
    rq.u = wind ? st.in(rq0.u, nb) : nullptr;
    rq.v = wind ? st.in(rq0.v, nb) : nullptr;
    rq.t = thermo ? st.in(rq0.t, nb) : nullptr;
    rq.h = humid ? st.in(rq0.h, nb) : nullptr;
    rq.ps = thermo ? st.in(rq0.ps, n) : nullptr;
    rq.ff = st.out(rq0.ff, nb);
    rq.temp = st.out(rq0.temp, nb);
    rq.hum = st.out(rq0.hum, nb);
    rq.hum2 = st.out(rq0.hum2, nb);
    rq.dd = st.out(rq0.dd, nb);
    if (!st.ok() || !ensure_levels(c, (size_t)nlev))
      return 0;
    if (!derived_common(c, nx, ny, nlev, rq, fdef_wind, fdef_thermo, undef, c->d_counts))
      return 0;
  }
  MIFC_HIP(c, hipMemcpyAsync(pinned_counts(c), c->d_counts, 5 * sizeof(u64) * (size_t)nlev, hipMemcpyDeviceToHost, c->stream));
  if (!st.finish())
    return 0;
  derived_flags(pinned_counts(c), nlev, n, rq0, fdef_ff, fdef_temp, fdef_hum, fdef_hum2, fdef_dd);
  return 1;
}

} // namespace

extern "C" {

int mifc_hlevel_derived_batch(mifc_ctx* c, int nx, int ny, int nlev, const float* u, const float* v, const float* t, const float* h, const float* ps,
                              const float* alevel, const float* blevel, float* ff, float* temp, const char* temp_unit, int temp_compute, float* hum,
                              const char* hum_unit, int hum_compute, float* hum2, const char* hum2_unit, int hum2_compute, float* dd,
                              const int* fdef_wind, const int* fdef_thermo, int* fdef_ff, int* fdef_temp, int* fdef_hum, int* fdef_hum2, int* fdef_dd,
                              float undef, int memkind)
{
  CTX_OR_FAIL(c);
  const DerivedRequest rq = {u, v, t, h, ps, alevel, blevel, ff, temp, hum, hum2, temp_unit, hum_unit, hum2_unit, temp_compute, hum_compute, hum2_compute, dd};
  return derived_sync(c, nx, ny, nlev, rq, fdef_wind, fdef_thermo, fdef_ff, fdef_temp, fdef_hum, fdef_hum2, fdef_dd, undef, memkind);
}

int mifc_hlevel_derived_batch_enqueue(mifc_ctx* c, int nx, int ny, int nlev, const float* u, const float* v, const float* t, const float* h,
                                      const float* ps, const float* alevel, const float* blevel, float* ff, float* temp, const char* temp_unit,
                                      int temp_compute, float* hum, const char* hum_unit, int hum_compute, float* hum2, const char* hum2_unit,
                                      int hum2_compute, float* dd, const int* fdef_wind, const int* fdef_thermo, float undef,
                                      unsigned long long* n_undefined_dev)
{
  if (!c || !n_undefined_dev)
    return 0;
  enter(c);
  if (!cells_in_fours(c, nx, ny, "mifc_hlevel_derived_batch"))
    return 0;
  const DerivedRequest rq = {u, v, t, h, ps, alevel, blevel, ff, temp, hum, hum2, temp_unit, hum_unit, hum2_unit, temp_compute, hum_compute, hum2_compute, dd};
  return derived_common(c, nx, ny, nlev, rq, fdef_wind, fdef_thermo, undef, n_undefined_dev);
}

// The original trio: ff, RH (hlevelhum compute 1), theta (hleveltemp compute 3).  n_undefined_dev keeps its
// documented layout u64[3 * nlev] = ff | rh | theta: the counters are collected in the context's own
// 4-array scratch and copied out in that order on the stream.
int mifc_hlevel_derived_levels_enqueue(mifc_ctx* c, int nx, int ny, int nlev, const float* u, const float* v, const float* t, const float* q,
                                       const float* ps, const float* alevel, const float* blevel, float* ff, float* rh, float* theta,
                                       const int* fdef_wind, const int* fdef_thermo, float undef, unsigned long long* n_undefined_dev)
{
  if (!c || !n_undefined_dev)
    return 0;
  enter(c);
  if (!cells_in_fours(c, nx, ny, "mifc_hlevel_derived_levels"))
    return 0;
  if (nlev < 1 || !ensure_levels(c, (size_t)nlev))
    return 0;
  const DerivedRequest rq = {u, v, t, q, ps, alevel, blevel, ff, theta, rh, nullptr, "", "", "", 3, 1, 0, nullptr};
  if (!derived_common(c, nx, ny, nlev, rq, fdef_wind, fdef_thermo, undef, c->d_counts))
    return 0;
  const size_t row = sizeof(u64) * (size_t)nlev;
  MIFC_HIP(c, hipMemcpyAsync(n_undefined_dev, c->d_counts, row, hipMemcpyDeviceToDevice, c->stream));                      // ff
  MIFC_HIP(c, hipMemcpyAsync(n_undefined_dev + nlev, c->d_counts + 2 * (size_t)nlev, row, hipMemcpyDeviceToDevice, c->stream)); // rh  <- hum
  MIFC_HIP(c, hipMemcpyAsync(n_undefined_dev + 2 * (size_t)nlev, c->d_counts + nlev, row, hipMemcpyDeviceToDevice, c->stream)); // theta <- temp
  return scratch_release(c) ? 1 : 0; // the copies read c->d_counts
}

int mifc_hlevel_derived_levels(mifc_ctx* c, int nx, int ny, int nlev, const float* u, const float* v, const float* t, const float* q, const float* ps,
                               const float* alevel, const float* blevel, float* ff, float* rh, float* theta, const int* fdef_wind,
                               const int* fdef_thermo, int* fdef_ff, int* fdef_rh, int* fdef_theta, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  const DerivedRequest rq = {u, v, t, q, ps, alevel, blevel, ff, theta, rh, nullptr, "", "", "", 3, 1, 0, nullptr};
  return derived_sync(c, nx, ny, nlev, rq, fdef_wind, fdef_thermo, fdef_ff, fdef_theta, fdef_rh, nullptr, nullptr, undef, memkind);
}

} // extern "C"
