// mifc_capi_vinterp.hip -- C ABI of mifc_vinterp_hlevels / mifc_vinterp_fields (include/mifc.h; EXTENSION, no reference
// function): the refusals, the device table of the per-level scalars, host-memory batches staged a band of rows at a
// time (columns are independent, so a band of every level is a complete problem), up to 32 targets per launch of the
// kernel of mifc_vinterp.hip.
#include "mifc_ctx.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

using namespace mifc_host;

namespace {

struct Call
{
  const char* name;
  bool hybrid;
  int nx, ny, nlev;
  const float* const* fields;
  const int* fdefined_in;
  int nfields;
  const float* coord; // ps [ny][nx] (hybrid) or the coordinate batch [nlev][ny][nx]
  int fdef_ps;
  const int* fdef_coord;
  const float *alevel, *blevel;
  const float* targets;
  int ntargets, method;
  float* const* fres;
  int* fdefined_out;
  float undef;
  int memkind;
};

int refuse(mifc_ctx* c, const Call& a, const std::string& why)
{
  c->err = std::string(a.name) + ": " + why;
  return 0;
}

int run(mifc_ctx* c, const Call& a)
{
  CTX_OR_FAIL(c);
  if (c->capturing)
    return refuse(c, a, "not available while a mifc_graph capture is open");
  if (a.nlev < 2)
    return refuse(c, a, "nlev < 2");
  if (a.nfields < 1 || a.nfields > mifc::VINTERP_MAX_FIELDS)
    return refuse(c, a, "nfields " + std::to_string(a.nfields) + " outside 1.." + std::to_string(mifc::VINTERP_MAX_FIELDS));
  if (a.ntargets < 1 || a.ntargets > mifc::VINTERP_MAX_TARGETS)
    return refuse(c, a, "ntargets " + std::to_string(a.ntargets) + " outside 1.." + std::to_string(mifc::VINTERP_MAX_TARGETS));
  if (a.nx < 0 || a.ny < 0)
    return refuse(c, a, "a negative nx or ny");
  if (a.memkind != MIFC_MEM_HOST && a.memkind != MIFC_MEM_DEVICE)
    return refuse(c, a, "unknown memkind " + std::to_string(a.memkind));
  if (a.method != MIFC_VINTERP_LINEAR && a.method != MIFC_VINTERP_LOG)
    return refuse(c, a, "unknown method " + std::to_string(a.method) + " (MIFC_VINTERP_LINEAR or MIFC_VINTERP_LOG)");
  if (!a.fields || !a.fres || !a.fdefined_out || !a.targets || !a.coord || (a.hybrid && (!a.alevel || !a.blevel)))
    return refuse(c, a, a.hybrid ? "a null pointer (fields, ps, alevel, blevel, targets, fres or fdefined_out)"
                                 : "a null pointer (fields, coord, targets, fres or fdefined_out)");
  const int nf = a.nfields, nt = a.ntargets, nlev = a.nlev;
  for (int f = 0; f < nf; ++f)
    if (!a.fields[f] || !a.fres[f])
      return refuse(c, a, "a null pointer (fields[" + std::to_string(f) + "] or fres[" + std::to_string(f) + "])");
  for (int t = 0; t < nt; ++t) {
    if (a.targets[t] != a.targets[t])
      return refuse(c, a, "targets[" + std::to_string(t) + "] is NaN");
    if (a.method == MIFC_VINTERP_LOG && !(a.targets[t] > 0.f))
      return refuse(c, a, "MIFC_VINTERP_LOG with targets[" + std::to_string(t) + "] <= 0");
  }
  if (a.hybrid)
    for (int k = 0; k < nlev; ++k)
      if (bad_hlevel(a.alevel[k], a.blevel[k]))
        return refuse(c, a, "level " + std::to_string(k) + ": alevel / blevel are no hybrid level (FieldCalculations.cc:298)");
  const long cells64 = (long)a.nx * (long)a.ny;
  if (cells64 > 0x7fffffffL)
    return refuse(c, a, "more than 2^31 - 1 cells per level");
  const size_t cells = (size_t)cells64, nx = (size_t)a.nx;
  const size_t in_bytes = cells * (size_t)nlev * sizeof(float), out_bytes = cells * (size_t)nt * sizeof(float);
  const size_t coord_bytes = a.hybrid ? cells * sizeof(float) : in_bytes;
  for (int f = 0; f < nf; ++f) {
    if (overlaps(a.fres[f], out_bytes, a.coord, coord_bytes))
      return refuse(c, a, std::string("fres[") + std::to_string(f) + "] overlaps " + (a.hybrid ? "ps" : "coord"));
    for (int g = 0; g < nf; ++g) {
      if (overlaps(a.fres[f], out_bytes, a.fields[g], in_bytes))
        return refuse(c, a, "fres[" + std::to_string(f) + "] overlaps fields[" + std::to_string(g) + "]");
      if (g != f && overlaps(a.fres[f], out_bytes, a.fres[g], out_bytes))
        return refuse(c, a, "fres[" + std::to_string(f) + "] overlaps fres[" + std::to_string(g) + "]");
    }
  }
  if (cells == 0) {
    for (int j = 0; j < nf * nt; ++j)
      a.fdefined_out[j] = MIFC_ALL_DEFINED; // checkDefined(0, 0)
    return 1;
  }

  // one device block, uploaded once: the counters (zero) | alevel, blevel | the per-level ALL_DEFINED bits
  const size_t n_counts = (size_t)nf * (size_t)nt;
  const size_t o_ab = align_up(n_counts * sizeof(u64), 16), o_bits = o_ab + align_up(2 * (size_t)nlev * sizeof(float), 16);
  const size_t tab_bytes = o_bits + (size_t)nlev * sizeof(unsigned int);
  std::vector<unsigned char> tab;
  std::vector<u64> counts;
  try { // nothing may be thrown across the C ABI
    tab.assign(tab_bytes, 0);
    counts.assign(n_counts, 0);
  } catch (...) {
    c->err = "out of host memory";
    return 0;
  }
  if (a.hybrid) {
    std::memcpy(tab.data() + o_ab, a.alevel, (size_t)nlev * sizeof(float));
    std::memcpy(tab.data() + o_ab + (size_t)nlev * sizeof(float), a.blevel, (size_t)nlev * sizeof(float));
  }
  {
    unsigned int* bits = reinterpret_cast<unsigned int*>(tab.data() + o_bits);
    for (int k = 0; k < nlev; ++k) {
      unsigned int b = 0;
      if (a.fdefined_in)
        for (int f = 0; f < nf; ++f)
          if (a.fdefined_in[(size_t)f * (size_t)nlev + (size_t)k] == MIFC_ALL_DEFINED)
            b |= 1u << f;
      if (!a.hybrid && a.fdef_coord && a.fdef_coord[k] == MIFC_ALL_DEFINED)
        b |= 1u << mifc::VINTERP_COORD_BIT;
      bits[k] = b;
    }
  }

  const bool host = a.memkind == MIFC_MEM_HOST;
  Staging st(c, a.memkind); // blocks only: a host batch is sub-allocated and copied band by band below
  unsigned char* d_tab = static_cast<unsigned char*>(st.scratch(tab_bytes));
  if (!st.ok())
    return 0;
  MIFC_HIP(c, hipMemcpyAsync(d_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, c->stream));

  mifc::VinterpParams P;
  std::memset(&P, 0, sizeof P);
  P.hybrid = a.hybrid ? 1 : 0;
  P.method = a.method;
  P.nfields = nf;
  P.nlev = nlev;
  P.nt_call = nt;
  P.ps_all = a.fdef_ps == MIFC_ALL_DEFINED ? 1 : 0;
  P.undef = a.undef;
  P.n_undefined = reinterpret_cast<u64*>(d_tab);
  P.ab = reinterpret_cast<const float*>(d_tab + o_ab);
  P.lev_bits = reinterpret_cast<const unsigned int*>(d_tab + o_bits);

  // the launches of one problem of n columns: 32 targets each
  auto launch_passes = [&]() -> int {
    for (int t0 = 0; t0 < nt; t0 += mifc::VINTERP_PASS) {
      P.t0 = t0;
      P.nt = std::min(mifc::VINTERP_PASS, nt - t0);
      for (int t = 0; t < mifc::VINTERP_PASS; ++t) {
        const float ct = t < P.nt ? a.targets[t0 + t] : 1.f, ckey = ct + 0.f; // the key of -0 is that of +0 (the same target)
        int bits;
        std::memcpy(&bits, &ckey, sizeof bits);
        P.target[t] = ct;
        P.target_key[t] = mifc::vinterp_key(bits);
        P.target_log[t] = (a.method == MIFC_VINTERP_LOG && t < P.nt) ? std::log((double)ct) : 0.0;
      }
      MIFC_LAUNCH(c, mifc::launch_vinterp(P, c->stream));
    }
    return 1;
  };

  if (host) {
    // a band of rows of every level, field, and target at a time
    const size_t planes = (size_t)nf * (size_t)nlev + (a.hybrid ? 1 : (size_t)nlev) + (size_t)nf * (size_t)nt;
    const size_t budget = (size_t)(mifc::env().vinterp_chunk_mib > 0 ? mifc::env().vinterp_chunk_mib : 256) << 20;
    size_t rows = std::max<size_t>(1, std::min<size_t>((size_t)a.ny, budget / (planes * nx * sizeof(float))));
    while (rows > 1 && planes * align_up(rows * nx, 64) * sizeof(float) > budget)
      rows -= 1;
    const size_t S = align_up(rows * nx, 64); // floats between the planes of the staged band: every plane on the 16-byte grid
    float* d = static_cast<float*>(st.scratch(planes * S * sizeof(float)));
    if (!st.ok())
      return 0;
    float* d_in = d;
    float* d_coord = d_in + (size_t)nf * (size_t)nlev * S;
    float* d_out = d_coord + (a.hybrid ? 1 : (size_t)nlev) * S;
    for (int f = 0; f < nf; ++f) {
      P.fields[f] = d_in + (size_t)f * (size_t)nlev * S;
      P.out[f] = d_out + (size_t)f * (size_t)nt * S;
    }
    P.coord = d_coord;
    P.in_stride = (long)S;
    P.out_stride = (long)S;
    P.vec4 = 1; // a lane's four floats may straddle the end of the band: they stay inside the padded plane
    const size_t pitch = cells * sizeof(float), dpitch = S * sizeof(float);
    for (size_t r0 = 0; r0 < (size_t)a.ny; r0 += rows) {
      const size_t nr = std::min(rows, (size_t)a.ny - r0), n = nr * nx, width = n * sizeof(float), off = r0 * nx;
      for (int f = 0; f < nf; ++f)
        MIFC_HIP(c, hipMemcpy2DAsync(const_cast<float*>(P.fields[f]), dpitch, a.fields[f] + off, pitch, width, (size_t)nlev, hipMemcpyHostToDevice,
                                     c->stream));
      MIFC_HIP(c, hipMemcpy2DAsync(d_coord, dpitch, a.coord + off, pitch, width, a.hybrid ? 1 : (size_t)nlev, hipMemcpyHostToDevice, c->stream));
      P.n = (int)n;
      if (!launch_passes())
        return 0;
      for (int f = 0; f < nf; ++f)
        MIFC_HIP(c, hipMemcpy2DAsync(a.fres[f] + off, pitch, P.out[f], dpitch, width, (size_t)nt, hipMemcpyDeviceToHost, c->stream));
    }
  } else {
    bool aligned = (cells & 3) == 0 && (reinterpret_cast<uintptr_t>(a.coord) & 15) == 0;
    for (int f = 0; f < nf; ++f) {
      P.fields[f] = a.fields[f];
      P.out[f] = a.fres[f];
      aligned = aligned && ((reinterpret_cast<uintptr_t>(a.fields[f]) | reinterpret_cast<uintptr_t>(a.fres[f])) & 15) == 0;
    }
    P.coord = a.coord;
    P.in_stride = (long)cells;
    P.out_stride = (long)cells;
    P.vec4 = aligned ? 1 : 0;
    P.n = (int)cells;
    if (!launch_passes())
      return 0;
  }
  MIFC_HIP(c, hipMemcpyAsync(counts.data(), d_tab, n_counts * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (!st.finish()) // nothing to copy back (the bands went as they were done): the synchronisation; `tab` was read by its copy
    return 0;
  for (size_t j = 0; j < n_counts; ++j)
    a.fdefined_out[j] = mifc_classify(counts[j], (u64)cells);
  return 1;
}

} // namespace

extern "C" {

int mifc_vinterp_hlevels(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields, const float* ps,
                         int fdef_ps, const float* alevel, const float* blevel, const float* targets, int ntargets, int method,
                         float* const* fres, int* fdefined_out, float undef, int memkind)
{
  const Call a = {"mifc_vinterp_hlevels", true, nx, ny, nlev, fields, fdefined_in, nfields, ps, fdef_ps, nullptr, alevel, blevel, targets, ntargets,
                  method, fres, fdefined_out, undef, memkind};
  return run(c, a);
}

int mifc_vinterp_fields(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields, const float* coord,
                        const int* fdef_coord, const float* targets, int ntargets, int method, float* const* fres, int* fdefined_out,
                        float undef, int memkind)
{
  const Call a = {"mifc_vinterp_fields", false, nx, ny, nlev, fields, fdefined_in, nfields, coord, MIFC_SOME_DEFINED, fdef_coord, nullptr, nullptr,
                  targets, ntargets, method, fres, fdefined_out, undef, memkind};
  return run(c, a);
}

} // extern "C"
