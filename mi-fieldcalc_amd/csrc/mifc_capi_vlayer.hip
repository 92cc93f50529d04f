// mifc_capi_vlayer.hip -- C ABI of mifc_vlayer_hlevels / mifc_vlayer_fields (include/mifc.h; EXTENSION, no reference
// function): the refusals, the device table of the per-level scalars, host-memory batches staged a band of rows at a
// time (columns are independent, so a band of every level is a complete problem), two or four fields per launch of the
// kernel of mifc_vlayer.hip (vlayer_pass_fields).
#include "mifc_ctx.h"

#include <algorithm>
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
  float lo, hi;
  const float *lo_field, *hi_field;
  const int* products;
  int nproducts;
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
  if (a.nfields < 1 || a.nfields > mifc::VLAYER_MAX_FIELDS)
    return refuse(c, a, "nfields " + std::to_string(a.nfields) + " outside 1.." + std::to_string(mifc::VLAYER_MAX_FIELDS));
  if (a.nproducts < 1 || a.nproducts > mifc::VLAYER_PRODUCTS)
    return refuse(c, a, "nproducts " + std::to_string(a.nproducts) + " outside 1.." + std::to_string(mifc::VLAYER_PRODUCTS));
  if (a.nx < 0 || a.ny < 0)
    return refuse(c, a, "a negative nx or ny");
  if (a.memkind != MIFC_MEM_HOST && a.memkind != MIFC_MEM_DEVICE)
    return refuse(c, a, "unknown memkind " + std::to_string(a.memkind));
  if (!a.fields || !a.fres || !a.fdefined_out || !a.products || !a.coord || (a.hybrid && (!a.alevel || !a.blevel)))
    return refuse(c, a, a.hybrid ? "a null pointer (fields, ps, alevel, blevel, products, fres or fdefined_out)"
                                 : "a null pointer (fields, coord, products, fres or fdefined_out)");
  const int nf = a.nfields, np = a.nproducts, nlev = a.nlev;
  for (int f = 0; f < nf; ++f)
    if (!a.fields[f] || !a.fres[f])
      return refuse(c, a, "a null pointer (fields[" + std::to_string(f) + "] or fres[" + std::to_string(f) + "])");
  int slot[mifc::VLAYER_PRODUCTS], group = 0;
  std::fill(slot, slot + mifc::VLAYER_PRODUCTS, -1);
  for (int p = 0; p < np; ++p) {
    const int code = a.products[p];
    if (code < MIFC_VLAYER_INTEGRAL || code > MIFC_VLAYER_COORD_OF_MIN)
      return refuse(c, a, "products[" + std::to_string(p) + "] = " + std::to_string(code) + " is no MIFC_VLAYER_* product");
    if (slot[code - 1] >= 0)
      return refuse(c, a, "product " + std::to_string(code) + " asked for twice");
    slot[code - 1] = p;
    group |= code <= MIFC_VLAYER_MEAN ? mifc::VLAYER_SUMS : mifc::VLAYER_EXTREMES;
  }
  // a scalar bound in use: against the other scalar, or at least a number (the per-cell test of rule 2 does the rest)
  if (!a.lo_field && !a.hi_field && !(a.lo < a.hi))
    return refuse(c, a, "the layer is empty: not lo < hi");
  if ((!a.lo_field && a.lo != a.lo) || (!a.hi_field && a.hi != a.hi))
    return refuse(c, a, "a NaN bound");
  if (a.hybrid)
    for (int k = 0; k < nlev; ++k)
      if (bad_hlevel(a.alevel[k], a.blevel[k]))
        return refuse(c, a, "level " + std::to_string(k) + ": alevel / blevel are no hybrid level (FieldCalculations.cc:298)");
  const long cells64 = (long)a.nx * (long)a.ny;
  if (cells64 > 0x7fffffffL)
    return refuse(c, a, "more than 2^31 - 1 cells per level");
  const size_t cells = (size_t)cells64, nx = (size_t)a.nx;
  const size_t plane = cells * sizeof(float), in_bytes = plane * (size_t)nlev, out_bytes = plane * (size_t)np;
  const size_t coord_bytes = a.hybrid ? plane : in_bytes;
  for (int f = 0; f < nf; ++f) {
    const std::string me = "fres[" + std::to_string(f) + "]";
    if (overlaps(a.fres[f], out_bytes, a.coord, coord_bytes))
      return refuse(c, a, me + " overlaps " + (a.hybrid ? "ps" : "coord"));
    if (a.lo_field && overlaps(a.fres[f], out_bytes, a.lo_field, plane))
      return refuse(c, a, me + " overlaps lo_field");
    if (a.hi_field && overlaps(a.fres[f], out_bytes, a.hi_field, plane))
      return refuse(c, a, me + " overlaps hi_field");
    for (int g = 0; g < nf; ++g) {
      if (overlaps(a.fres[f], out_bytes, a.fields[g], in_bytes))
        return refuse(c, a, me + " overlaps fields[" + std::to_string(g) + "]");
      if (g != f && overlaps(a.fres[f], out_bytes, a.fres[g], out_bytes))
        return refuse(c, a, me + " overlaps fres[" + std::to_string(g) + "]");
    }
  }
  if (cells == 0) {
    for (int j = 0; j < nf * np; ++j)
      a.fdefined_out[j] = MIFC_ALL_DEFINED; // checkDefined(0, 0)
    return 1;
  }

  // one device block, uploaded once: the counters (zero) | alevel, blevel | the per-level ALL_DEFINED bits
  const size_t o_ab = align_up((size_t)nf * sizeof(u64), 16), o_bits = o_ab + align_up(2 * (size_t)nlev * sizeof(float), 16);
  const size_t tab_bytes = o_bits + (size_t)nlev * sizeof(unsigned int);
  std::vector<unsigned char> tab;
  try { // nothing may be thrown across the C ABI
    tab.assign(tab_bytes, 0);
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

  mifc::VlayerParams P;
  std::memset(&P, 0, sizeof P);
  P.hybrid = a.hybrid ? 1 : 0;
  P.group = group;
  P.nlev = nlev;
  P.ps_all = a.fdef_ps == MIFC_ALL_DEFINED ? 1 : 0;
  P.undef = a.undef;
  P.lo = a.lo;
  P.hi = a.hi;
  P.n_undefined = reinterpret_cast<u64*>(d_tab);
  P.ab = reinterpret_cast<const float*>(d_tab + o_ab);
  P.lev_bits = reinterpret_cast<const unsigned int*>(d_tab + o_bits);
  std::copy(slot, slot + mifc::VLAYER_PRODUCTS, P.slot);

  // the launches of one problem of P.n columns: vlayer_pass_fields(group) fields each, field f at in[f], its products at out[f]
  const float* in[mifc::VLAYER_MAX_FIELDS];
  float* out[mifc::VLAYER_MAX_FIELDS];
  auto launch_passes = [&]() -> int {
    const int pass = mifc::vlayer_pass_fields(group);
    for (int f0 = 0; f0 < nf; f0 += pass) {
      P.f0 = f0;
      P.nfields = std::min(pass, nf - f0);
      for (int f = 0; f < P.nfields; ++f) {
        P.fields[f] = in[f0 + f];
        P.out[f] = out[f0 + f];
      }
      MIFC_LAUNCH(c, mifc::launch_vlayer(P, c->stream));
    }
    return 1;
  };

  if (host) {
    // a band of rows of every level, field, bound and product at a time
    const size_t n_coord = a.hybrid ? 1 : (size_t)nlev, n_bounds = (a.lo_field ? 1 : 0) + (a.hi_field ? 1 : 0);
    const size_t planes = (size_t)nf * (size_t)nlev + n_coord + n_bounds + (size_t)nf * (size_t)np;
    const size_t budget = (size_t)(mifc::env().vlayer_chunk_mib > 0 ? mifc::env().vlayer_chunk_mib : 256) << 20;
    size_t rows = std::max<size_t>(1, std::min<size_t>((size_t)a.ny, budget / (planes * nx * sizeof(float))));
    while (rows > 1 && planes * align_up(rows * nx, 64) * sizeof(float) > budget)
      rows -= 1;
    const size_t S = align_up(rows * nx, 64); // floats between the planes of the staged band: every plane on the 16-byte grid
    float* d = static_cast<float*>(st.scratch(planes * S * sizeof(float)));
    if (!st.ok())
      return 0;
    float* d_in = d;
    float* d_coord = d_in + (size_t)nf * (size_t)nlev * S;
    float* d_lo = d_coord + n_coord * S;
    float* d_hi = d_lo + (a.lo_field ? S : 0);
    float* d_out = d_coord + (n_coord + n_bounds) * S;
    for (int f = 0; f < nf; ++f) {
      in[f] = d_in + (size_t)f * (size_t)nlev * S;
      out[f] = d_out + (size_t)f * (size_t)np * S;
    }
    P.coord = d_coord;
    P.lo_field = a.lo_field ? d_lo : nullptr;
    P.hi_field = a.hi_field ? d_hi : nullptr;
    P.in_stride = (long)S;
    P.out_stride = (long)S;
    P.vec4 = 1; // a lane's four floats may straddle the end of the band: they stay inside the padded plane
    const size_t pitch = cells * sizeof(float), dpitch = S * sizeof(float);
    for (size_t r0 = 0; r0 < (size_t)a.ny; r0 += rows) {
      const size_t nr = std::min(rows, (size_t)a.ny - r0), n = nr * nx, width = n * sizeof(float), off = r0 * nx;
      for (int f = 0; f < nf; ++f)
        MIFC_HIP(c, hipMemcpy2DAsync(const_cast<float*>(in[f]), dpitch, a.fields[f] + off, pitch, width, (size_t)nlev, hipMemcpyHostToDevice, c->stream));
      MIFC_HIP(c, hipMemcpy2DAsync(d_coord, dpitch, a.coord + off, pitch, width, n_coord, hipMemcpyHostToDevice, c->stream));
      if (a.lo_field)
        MIFC_HIP(c, hipMemcpyAsync(d_lo, a.lo_field + off, width, hipMemcpyHostToDevice, c->stream));
      if (a.hi_field)
        MIFC_HIP(c, hipMemcpyAsync(d_hi, a.hi_field + off, width, hipMemcpyHostToDevice, c->stream));
      P.n = (int)n;
      if (!launch_passes())
        return 0;
      for (int f = 0; f < nf; ++f)
        MIFC_HIP(c, hipMemcpy2DAsync(a.fres[f] + off, pitch, out[f], dpitch, width, (size_t)np, hipMemcpyDeviceToHost, c->stream));
    }
  } else {
    uintptr_t all = reinterpret_cast<uintptr_t>(a.coord) | reinterpret_cast<uintptr_t>(a.lo_field) | reinterpret_cast<uintptr_t>(a.hi_field);
    for (int f = 0; f < nf; ++f) {
      in[f] = a.fields[f];
      out[f] = a.fres[f];
      all |= reinterpret_cast<uintptr_t>(a.fields[f]) | reinterpret_cast<uintptr_t>(a.fres[f]);
    }
    P.coord = a.coord;
    P.lo_field = a.lo_field;
    P.hi_field = a.hi_field;
    P.in_stride = (long)cells;
    P.out_stride = (long)cells;
    P.vec4 = ((cells & 3) == 0 && (all & 15) == 0) ? 1 : 0;
    P.n = (int)cells;
    if (!launch_passes())
      return 0;
  }
  u64 counts[mifc::VLAYER_MAX_FIELDS] = {0};
  MIFC_HIP(c, hipMemcpyAsync(counts, d_tab, (size_t)nf * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (!st.finish()) // nothing to copy back (the bands went as they were done): the synchronisation; `tab` was read by its copy
    return 0;
  for (int f = 0; f < nf; ++f)
    for (int p = 0; p < np; ++p)
      a.fdefined_out[f * np + p] = mifc_classify(counts[f], (u64)cells);
  return 1;
}

} // namespace

extern "C" {

int mifc_vlayer_hlevels(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields, const float* ps,
                        int fdef_ps, const float* alevel, const float* blevel, float lo, float hi, const float* lo_field, const float* hi_field,
                        const int* products, int nproducts, float* const* fres, int* fdefined_out, float undef, int memkind)
{
  const Call a = {"mifc_vlayer_hlevels", true, nx, ny, nlev, fields, fdefined_in, nfields, ps, fdef_ps, nullptr, alevel, blevel, lo, hi, lo_field,
                  hi_field, products, nproducts, fres, fdefined_out, undef, memkind};
  return run(c, a);
}

int mifc_vlayer_fields(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields, const float* coord,
                       const int* fdef_coord, float lo, float hi, const float* lo_field, const float* hi_field, const int* products,
                       int nproducts, float* const* fres, int* fdefined_out, float undef, int memkind)
{
  const Call a = {"mifc_vlayer_fields", false, nx, ny, nlev, fields, fdefined_in, nfields, coord, MIFC_SOME_DEFINED, fdef_coord, nullptr, nullptr,
                  lo, hi, lo_field, hi_field, products, nproducts, fres, fdefined_out, undef, memkind};
  return run(c, a);
}

} // extern "C"
