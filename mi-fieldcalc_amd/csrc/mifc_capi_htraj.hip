// mifc_capi_htraj.hip -- C ABI of mifc_htraj_levels (include/mifc.h; EXTENSION, no reference function): its refusals
// (the ones that read only the scalars and `times` are mifc_htraj_rules.h's htraj_check), the table of the flags per
// interval and level, the launches of mifc_htraj.hip -- one per interval and level chunk, queued one behind the other on
// the context's stream, the slot an interval leaves being the one the next starts from -- and the flags from the
// counters.  Device memory is used where it is.  Levels are independent, so host memory runs chunk of whole levels by
// chunk: two slice buffers (slice B goes up while A stays), every slot of the chunk on the device until the last
// interval, then one strided copy per output.  The map planes and the start positions go up once.
#include "mifc_htraj_rules.h"
#include "mifc_levelbatch.h"

#include <cstdio>

using namespace mifc_host;

namespace {

// mifc_last_htraj_form: the shape of the calling thread's last call
struct HtrajForm
{
  int niter = -1, nsub = 0, ntrace = 0, tested = 0, blocks = 0, level_chunks = 0, chunk = 0, intervals = 0, launches = 0, staged = 0;
};
thread_local HtrajForm t_form;
thread_local char t_form_text[224];

int refuse(mifc_ctx* c, const std::string& why)
{
  c->err = "mifc_htraj_levels: " + why;
  return 0;
}

struct NamedRange
{
  const void* p;
  size_t bytes;
  std::string name;
};

} // namespace

extern "C" {

int mifc_htraj_levels(mifc_ctx* c, int nx, int ny, int nlev, int nt, const float* const* u, const float* const* v, const int* fdefined_in,
                      const double* times, const float* xmapr, const float* ymapr, int fdef_map, int npos, const float* xpos0, const float* ypos0,
                      int j_start, int j_end, int nsub, int niter, const float* const* trace, const int* fdef_trace, int ntrace, float* xres,
                      float* yres, float* const* tres, int* fdefined_out, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  if (c->capturing)
    return refuse(c, "not available while a mifc_graph capture is open");
  if (const char* why = mifc::htraj_check(nx, ny, nlev, nt, npos, j_start, j_end, nsub, niter, ntrace, times, undef))
    return refuse(c, why);
  if (memkind != MIFC_MEM_HOST && memkind != MIFC_MEM_DEVICE)
    return refuse(c, "unknown memkind " + std::to_string(memkind));
  if (!u || !v || !xmapr || !ymapr || !xpos0 || !ypos0 || !xres || !yres || !fdefined_out)
    return refuse(c, "a null pointer (u, v, xmapr, ymapr, xpos0, ypos0, xres, yres or fdefined_out)");
  if (ntrace > 0 && (!trace || !tres))
    return refuse(c, "a null pointer (trace or tres)");
  const mifc::HtrajPlan plan = mifc::htraj_plan(j_start, j_end);
  const int j_lo = std::min(j_start, j_end), j_hi = std::max(j_start, j_end);
  for (int j = j_lo; j <= j_hi; ++j) {
    if (!u[j] || !v[j])
      return refuse(c, "a null pointer (u[" + std::to_string(j) + "] or v[" + std::to_string(j) + "])");
    for (int f = 0; f < ntrace; ++f)
      if (!trace[(size_t)f * nt + j])
        return refuse(c, "a null pointer (trace[" + std::to_string((size_t)f * nt + j) + "])");
  }
  for (int f = 0; f < ntrace; ++f)
    if (!tres[f])
      return refuse(c, "a null pointer (tres[" + std::to_string(f) + "])");

  const size_t cells = (size_t)nx * (size_t)ny, points = (size_t)npos, levels = (size_t)nlev, nslots = (size_t)plan.nslots;
  const size_t n_out = 2 + (size_t)ntrace, out_floats = nslots * levels * points;
  try { // nothing may be thrown across the C ABI
    std::vector<NamedRange> ins, outs;
    for (int j = j_lo; j <= j_hi; ++j) {
      ins.push_back({u[j], levels * cells * sizeof(float), "u[" + std::to_string(j) + "]"});
      ins.push_back({v[j], levels * cells * sizeof(float), "v[" + std::to_string(j) + "]"});
      for (int f = 0; f < ntrace; ++f)
        ins.push_back({trace[(size_t)f * nt + j], levels * cells * sizeof(float), "trace[" + std::to_string((size_t)f * nt + j) + "]"});
    }
    ins.push_back({xmapr, cells * sizeof(float), "xmapr"});
    ins.push_back({ymapr, cells * sizeof(float), "ymapr"});
    ins.push_back({xpos0, points * sizeof(float), "xpos0"});
    ins.push_back({ypos0, points * sizeof(float), "ypos0"});
    outs.push_back({xres, out_floats * sizeof(float), "xres"});
    outs.push_back({yres, out_floats * sizeof(float), "yres"});
    for (int f = 0; f < ntrace; ++f)
      outs.push_back({tres[f], out_floats * sizeof(float), "tres[" + std::to_string(f) + "]"});
    for (const NamedRange& o : outs) {
      for (const NamedRange& i : ins)
        if (overlaps(o.p, o.bytes, i.p, i.bytes))
          return refuse(c, o.name + " overlaps " + i.name);
      for (const NamedRange& q : outs)
        if (&q != &o && overlaps(o.p, o.bytes, q.p, q.bytes))
          return refuse(c, o.name + " overlaps " + q.name);
    }
  } catch (...) {
    c->err = "out of host memory";
    return 0;
  }

  // the word of every (interval, level): the planes flagged ALL_DEFINED there; tested: any plane of the call that is not
  const size_t intervals = (size_t)plan.intervals, n_counts = n_out - 1; // (x and y share the counter of the lost particles)
  std::vector<unsigned int> bits;
  std::vector<u64> counts;
  try {
    bits.assign(intervals * levels, 0u);
    counts.assign(n_counts * nslots * levels, 0);
  } catch (...) {
    c->err = "out of host memory";
    return 0;
  }
  bool tested = fdef_map != MIFC_ALL_DEFINED;
  auto wind_all = [&](int comp, int j, size_t k) { return fdefined_in && fdefined_in[((size_t)comp * nt + j) * levels + k] == MIFC_ALL_DEFINED; };
  auto trace_all = [&](int f, int j, size_t k) { return fdef_trace && fdef_trace[((size_t)f * nt + j) * levels + k] == MIFC_ALL_DEFINED; };
  for (size_t n = 0; n < intervals; ++n) {
    const int A = mifc::htraj_slice(plan, j_start, (int)n), B = A + plan.dir;
    for (size_t k = 0; k < levels; ++k) {
      unsigned int w = (wind_all(0, A, k) ? 1u << mifc::HTRAJ_UA_BIT : 0u) | (wind_all(0, B, k) ? 1u << mifc::HTRAJ_UB_BIT : 0u) |
                       (wind_all(1, A, k) ? 1u << mifc::HTRAJ_VA_BIT : 0u) | (wind_all(1, B, k) ? 1u << mifc::HTRAJ_VB_BIT : 0u) |
                       (fdef_map == MIFC_ALL_DEFINED ? 1u << mifc::HTRAJ_MAP_BIT : 0u);
      tested |= (w & 0xfu) != 0xfu;
      for (int f = 0; f < ntrace; ++f) {
        w |= (trace_all(f, A, k) ? 1u << (mifc::HTRAJ_TRACE_A_BIT + f) : 0u) | (trace_all(f, B, k) ? 1u << (mifc::HTRAJ_TRACE_B_BIT + f) : 0u);
        tested |= !trace_all(f, A, k) || !trace_all(f, B, k);
      }
      bits[n * levels + k] = w;
    }
  }

  Staging st(c, memkind);
  unsigned int* d_bits = static_cast<unsigned int*>(st.scratch(bits.size() * sizeof(unsigned int)));
  u64* d_counts = static_cast<u64*>(st.scratch(counts.size() * sizeof(u64)));
  const float *d_xmapr = st.in(xmapr, cells), *d_ymapr = st.in(ymapr, cells), *d_xpos0 = st.in(xpos0, points), *d_ypos0 = st.in(ypos0, points);
  if (!st.ok())
    return 0;
  MIFC_HIP(c, hipMemcpyAsync(d_bits, bits.data(), bits.size() * sizeof(unsigned int), hipMemcpyHostToDevice, c->stream));
  MIFC_HIP(c, hipMemsetAsync(d_counts, 0, counts.size() * sizeof(u64), c->stream));

  // host memory: L levels at a time -- two slice buffers of u, v and the trace fields, every slot of every output
  const bool host = memkind == MIFC_MEM_HOST;
  const size_t budget = (size_t)(mifc::env().htraj_chunk_mib > 0 ? mifc::env().htraj_chunk_mib : 256) << 20;
  const size_t L = host ? (size_t)mifc::htraj_levels_per_chunk(budget, mifc::htraj_bytes_per_level(cells, points, plan.nslots, ntrace), nlev) : levels;
  float* staged = nullptr;
  if (host) {
    staged = static_cast<float*>(st.scratch(L * (size_t)mifc::htraj_bytes_per_level(cells, points, plan.nslots, ntrace)));
    if (!st.ok())
      return 0;
  }
  const size_t buffer = n_out * L * cells;                     // one slice buffer: u | v | trace 0 ..., L levels each
  float* const staged_out = host ? staged + 2 * buffer : nullptr; // x | y | t 0 ..., [nslots][L][npos] each
  auto plane_of = [&](int g, int j) { return g == 0 ? u[j] : (g == 1 ? v[j] : trace[(size_t)(g - 2) * nt + j]); };
  float* const out_of[2 + mifc::HTRAJ_MAX_TRACE] = {xres, yres, ntrace > 0 ? tres[0] : nullptr, ntrace > 1 ? tres[1] : nullptr,
                                                    ntrace > 2 ? tres[2] : nullptr, ntrace > 3 ? tres[3] : nullptr};

  mifc::HtrajParams P;
  std::memset(&P, 0, sizeof P);
  P.nx = nx;
  P.ny = ny;
  P.npos = npos;
  P.call_nlev = nlev;
  P.nslots = plan.nslots;
  P.nsub = nsub;
  P.niter = niter;
  P.ntrace = ntrace;
  P.tested = tested ? 1 : 0;
  P.undef = undef;
  P.in_stride = (long)cells;
  P.slot_stride = (long)(L * points);
  P.xmapr = d_xmapr;
  P.ymapr = d_ymapr;
  P.xpos0 = d_xpos0;
  P.ypos0 = d_ypos0;

  HtrajForm form;
  form.niter = niter;
  form.nsub = nsub;
  form.ntrace = ntrace;
  form.tested = P.tested;
  form.intervals = plan.intervals;
  form.blocks = (int)((points + 255) / 256);
  for (size_t k0 = 0; k0 < levels; k0 += L) {
    const size_t n = std::min(L, levels - k0);
    // where plane g of slice j is for this chunk: the caller's, or the slice buffer `b` after the upload
    auto upload = [&](int j, size_t b) {
      for (size_t g = 0; g < n_out; ++g)
        MIFC_HIP(c, hipMemcpyAsync(staged + b * buffer + g * L * cells, plane_of((int)g, j) + k0 * cells, n * cells * sizeof(float), hipMemcpyHostToDevice,
                                   c->stream));
      return 1;
    };
    auto plane_at = [&](int g, int j, size_t b) -> const float* { return host ? staged + b * buffer + (size_t)g * L * cells : plane_of(g, j); };
    if (host && !upload(j_start, 0))
      return 0;
    P.nlev = (int)n;
    for (size_t i = 0; i < intervals; ++i) {
      const int A = mifc::htraj_slice(plan, j_start, (int)i), B = A + plan.dir;
      const size_t bA = i & 1, bB = bA ^ 1;
      if (host && !upload(B, bB)) // (the launch before has read this buffer as its slice A: stream order)
        return 0;
      P.first = i == 0 ? 1 : 0;
      P.tau = times[B] - times[A];
      P.uA = plane_at(0, A, bA);
      P.uB = plane_at(0, B, bB);
      P.vA = plane_at(1, A, bA);
      P.vB = plane_at(1, B, bB);
      for (int f = 0; f < ntrace; ++f) {
        P.trace[f] = plane_at(2 + f, A, bA);
        P.trace[mifc::HTRAJ_MAX_TRACE + f] = plane_at(2 + f, B, bB);
      }
      const size_t slot_at = i * L * points; // slot i, level 0 of the chunk
      for (size_t g = 0; g < n_out; ++g) {
        float* const base = host ? staged_out + g * nslots * L * points : out_of[g] + k0 * points;
        (g == 0 ? P.x : (g == 1 ? P.y : P.t[g - 2])) = base + slot_at;
      }
      P.bits = d_bits + i * levels + k0;
      P.counts = d_counts + i * levels + k0;
      MIFC_LAUNCH(c, mifc::launch_htraj(P, c->stream));
      form.launches += 1;
    }
    form.chunk = mifc::htraj_level_chunk((int)n, mifc::env().htraj_level_chunk);
    form.level_chunks = ((int)n + form.chunk - 1) / form.chunk;
    form.staged += host ? 1 : 0;
    if (host)
      for (size_t g = 0; g < n_out; ++g)
        MIFC_HIP(c, hipMemcpy2DAsync(out_of[g] + k0 * points, levels * points * sizeof(float), staged_out + g * nslots * L * points,
                                     L * points * sizeof(float), n * points * sizeof(float), nslots, hipMemcpyDeviceToHost, c->stream));
  }
  MIFC_HIP(c, hipMemcpyAsync(counts.data(), d_counts, counts.size() * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (!st.finish()) // the one synchronisation of the call
    return 0;
  t_form = form;
  // rule 8: the lost particles for the positions; the lost particles and the holes for a trace field
  for (size_t g = 0; g < n_counts; ++g)
    for (size_t j = 0; j < nslots * levels; ++j)
      fdefined_out[g * nslots * levels + j] = mifc_classify(counts[j] + (g > 0 ? counts[g * nslots * levels + j] : 0), (u64)points);
  return 1;
}

const char* mifc_last_htraj_form(void)
{
  const HtrajForm& f = t_form;
  if (f.niter < 0)
    return "";
  std::snprintf(t_form_text, sizeof t_form_text, "niter=%d nsub=%d ntrace=%d tested=%d blocks=%d level_chunks=%d chunk=%d intervals=%d launches=%d staged=%d",
                f.niter, f.nsub, f.ntrace, f.tested, f.blocks, f.level_chunks, f.chunk, f.intervals, f.launches, f.staged);
  return t_form_text;
}

} // extern "C"
