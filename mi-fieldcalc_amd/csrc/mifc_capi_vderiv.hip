// mifc_capi_vderiv.hip -- C ABI of mifc_vderiv_hlevels / mifc_vderiv_fields / mifc_vderiv_levels (include/mifc.h;
// EXTENSION, no reference function): the refusals, the device table of the per-level scalars (for the `levels` form also
// the weights, divided here once per level), host-memory batches staged a band of rows at a time (columns are
// independent, so a band of every level is a complete problem), two or four fields per launch of the kernel of
// mifc_vderiv.hip (vderiv_pass_fields).
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
  int kind; // mifc::VDERIV_HYBRID / _FIELD / _LEVELS
  int nx, ny, nlev;
  const float* const* fields;
  const int* fdefined_in;
  int nfields;
  const float* coord; // ps [ny][nx] (hybrid), the coordinate batch [nlev][ny][nx] (field) or HOST levels[nlev]
  int fdef_ps;
  const int* fdef_coord;
  const float *alevel, *blevel;
  int method;
  float* const* fres;
  int* fdefined_out;
  float* const* fmag;
  int* fdefined_mag;
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
  const bool hybrid = a.kind == mifc::VDERIV_HYBRID, by_level = a.kind == mifc::VDERIV_LEVELS;
  if (c->capturing)
    return refuse(c, a, "not available while a mifc_graph capture is open");
  if (a.nlev < 2)
    return refuse(c, a, "nlev < 2");
  if (a.nfields < 1 || a.nfields > mifc::VDERIV_MAX_FIELDS)
    return refuse(c, a, "nfields " + std::to_string(a.nfields) + " outside 1.." + std::to_string(mifc::VDERIV_MAX_FIELDS));
  if (a.nx < 0 || a.ny < 0)
    return refuse(c, a, "a negative nx or ny");
  if (a.method != MIFC_VDERIV_CENTRED && a.method != MIFC_VDERIV_WEIGHTED)
    return refuse(c, a, "unknown method " + std::to_string(a.method));
  if (a.memkind != MIFC_MEM_HOST && a.memkind != MIFC_MEM_DEVICE)
    return refuse(c, a, "unknown memkind " + std::to_string(a.memkind));
  if (!a.fields || !a.coord || (hybrid && (!a.alevel || !a.blevel)))
    return refuse(c, a, hybrid ? "a null pointer (fields, ps, alevel or blevel)" : (by_level ? "a null pointer (fields or levels)" : "a null pointer (fields or coord)"));
  if (!a.fres && !a.fmag)
    return refuse(c, a, "fres and fmag are both null: nothing to write");
  if (a.fmag && (a.nfields & 1) != 0)
    return refuse(c, a, "fmag with an odd nfields: a magnitude takes the fields 2j and 2j + 1");
  if (a.fmag && !a.fdefined_mag)
    return refuse(c, a, "fmag without fdefined_mag");
  if (a.fres && !a.fdefined_out)
    return refuse(c, a, "fres without fdefined_out");
  const int nf = a.nfields, nm = a.fmag ? nf / 2 : 0, nlev = a.nlev;
  for (int f = 0; f < nf; ++f)
    if (!a.fields[f] || (a.fres && !a.fres[f]))
      return refuse(c, a, "a null pointer (fields[" + std::to_string(f) + "] or fres[" + std::to_string(f) + "])");
  for (int j = 0; j < nm; ++j)
    if (!a.fmag[j])
      return refuse(c, a, "a null pointer (fmag[" + std::to_string(j) + "])");
  if (hybrid)
    for (int k = 0; k < nlev; ++k)
      if (bad_hlevel(a.alevel[k], a.blevel[k]))
        return refuse(c, a, "level " + std::to_string(k) + ": alevel / blevel are no hybrid level (FieldCalculations.cc:298)");
  if (by_level)
    for (int k = 0; k < nlev; ++k)
      if (a.coord[k] != a.coord[k])
        return refuse(c, a, "levels[" + std::to_string(k) + "] is NaN");
  const long cells64 = (long)a.nx * (long)a.ny;
  if (cells64 > 0x7fffffffL)
    return refuse(c, a, "more than 2^31 - 1 cells per level");
  const size_t cells = (size_t)cells64, nx = (size_t)a.nx;
  const size_t plane = cells * sizeof(float), batch = plane * (size_t)nlev;
  const size_t coord_bytes = by_level ? 0 : (hybrid ? plane : batch);
  // in-place is not offered: every output against every input, the coordinate and every other output, by byte range
  struct Out
  {
    const float* p;
    std::string name;
  };
  std::vector<Out> outs;
  try { // nothing may be thrown across the C ABI
    for (int f = 0; a.fres && f < nf; ++f)
      outs.push_back({a.fres[f], "fres[" + std::to_string(f) + "]"});
    for (int j = 0; j < nm; ++j)
      outs.push_back({a.fmag[j], "fmag[" + std::to_string(j) + "]"});
  } catch (...) {
    c->err = "out of host memory";
    return 0;
  }
  for (size_t o = 0; o < outs.size(); ++o) {
    if (coord_bytes != 0 && overlaps(outs[o].p, batch, a.coord, coord_bytes))
      return refuse(c, a, outs[o].name + " overlaps " + (hybrid ? "ps" : "coord"));
    for (int g = 0; g < nf; ++g)
      if (overlaps(outs[o].p, batch, a.fields[g], batch))
        return refuse(c, a, outs[o].name + " overlaps fields[" + std::to_string(g) + "]");
    for (size_t q = 0; q < outs.size(); ++q)
      if (q != o && overlaps(outs[o].p, batch, outs[q].p, batch))
        return refuse(c, a, outs[o].name + " overlaps " + outs[q].name);
  }
  if (cells == 0) {
    for (int j = 0; a.fres && j < nf * nlev; ++j)
      a.fdefined_out[j] = MIFC_ALL_DEFINED; // checkDefined(0, 0)
    for (int j = 0; j < nm * nlev; ++j)
      a.fdefined_mag[j] = MIFC_ALL_DEFINED;
    return 1;
  }

  // one device block, uploaded once: the counters (zero) | alevel, blevel | the per-level bits | the per-level weights
  const size_t ncount = (size_t)(nf + nm) * (size_t)nlev;
  const size_t o_ab = align_up(ncount * sizeof(u64), 16), o_bits = o_ab + align_up(2 * (size_t)nlev * sizeof(float), 16);
  const size_t o_w = o_bits + align_up((size_t)nlev * sizeof(unsigned int), 16);
  const size_t tab_bytes = o_w + (by_level ? 4 * (size_t)nlev * sizeof(double) : 0);
  std::vector<unsigned char> tab;
  try {
    tab.assign(tab_bytes, 0);
  } catch (...) {
    c->err = "out of host memory";
    return 0;
  }
  if (hybrid) {
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
      if (a.kind == mifc::VDERIV_FIELD && a.fdef_coord && a.fdef_coord[k] == MIFC_ALL_DEFINED)
        b |= 1u << mifc::VINTERP_COORD_BIT;
      bits[k] = b;
    }
    if (by_level) {
      // rules 3 to 5 for a coordinate that is the same in every cell of a level: the sides that exist and the weights, in
      // double, every operation rounded on its own (this file is compiled without contraction like the kernels)
      double* w = reinterpret_cast<double*>(tab.data() + o_w);
      const float* lv = a.coord;
      for (int k = 0; k < nlev; ++k) {
        const bool lower = k > 0 && lv[k - 1] != lv[k], upper = k < nlev - 1 && lv[k + 1] != lv[k];
        const double d0 = (double)lv[k], dm = k > 0 ? (double)lv[k - 1] : 0.0, dp = k < nlev - 1 ? (double)lv[k + 1] : 0.0;
        const double h1 = d0 - dm, h2 = dp - d0;
        if (lower)
          w[4 * k] = 1.0 / h1;
        if (upper)
          w[4 * k + 1] = 1.0 / h2;
        bool fold = false;
        if (lower && upper) {
          if (a.method == MIFC_VDERIV_WEIGHTED) {
            const double s = h1 + h2;
            fold = s == 0.0;
            if (!fold) {
              const double p1 = h1 * s, p2 = h2 * s;
              w[4 * k + 2] = h2 / p1;
              w[4 * k + 3] = h1 / p2;
            }
          } else {
            const double dc = dp - dm;
            fold = dc == 0.0;
            if (!fold)
              w[4 * k + 2] = 1.0 / dc;
          }
        }
        bits[k] |= (lower ? 1u << mifc::VDERIV_LOWER_BIT : 0u) | (upper ? 1u << mifc::VDERIV_UPPER_BIT : 0u) |
                   (fold ? 1u << mifc::VDERIV_FOLD_BIT : 0u);
      }
    }
  }

  const bool host = a.memkind == MIFC_MEM_HOST;
  Staging st(c, a.memkind); // blocks only: a host batch is sub-allocated and copied band by band below
  unsigned char* d_tab = static_cast<unsigned char*>(st.scratch(tab_bytes));
  if (!st.ok())
    return 0;
  MIFC_HIP(c, hipMemcpyAsync(d_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice, c->stream));

  mifc::VderivParams P;
  std::memset(&P, 0, sizeof P);
  P.kind = a.kind;
  P.what = (a.fres ? mifc::VDERIV_DERIV : 0) | (a.fmag ? mifc::VDERIV_MAG : 0);
  P.method = a.method;
  P.nlev = nlev;
  P.ps_all = a.fdef_ps == MIFC_ALL_DEFINED ? 1 : 0;
  P.undef = a.undef;
  P.n_undefined = reinterpret_cast<u64*>(d_tab);
  P.n_undefined_mag = P.n_undefined + (size_t)nf * (size_t)nlev;
  P.ab = reinterpret_cast<const float*>(d_tab + o_ab);
  P.lev_bits = reinterpret_cast<const unsigned int*>(d_tab + o_bits);
  P.lev_w = reinterpret_cast<const double*>(d_tab + o_w);

  // the launches of one problem of P.n columns: four fields each, two where both the derivatives and the magnitudes are
  // written (an even number: a vector stays in one launch)
  const float* in[mifc::VDERIV_MAX_FIELDS];
  float* out[mifc::VDERIV_MAX_FIELDS] = {nullptr};
  float* mag[mifc::VDERIV_MAX_FIELDS / 2] = {nullptr};
  auto launch_passes = [&]() -> int {
    const int pass = mifc::vderiv_pass_fields(P.what);
    for (int f0 = 0; f0 < nf; f0 += pass) {
      P.f0 = f0;
      P.nfields = std::min(pass, nf - f0);
      for (int f = 0; f < P.nfields; ++f) {
        P.fields[f] = in[f0 + f];
        P.out[f] = out[f0 + f];
      }
      for (int j = 0; j < P.nfields / 2; ++j)
        P.mag[j] = mag[f0 / 2 + j];
      MIFC_LAUNCH(c, mifc::launch_vderiv(P, c->stream));
    }
    return 1;
  };

  if (host) {
    // a band of rows of every level, field, coordinate level and output at a time
    const size_t n_coord = by_level ? 0 : (hybrid ? 1 : (size_t)nlev);
    const size_t n_in = (size_t)nf * (size_t)nlev, n_out = a.fres ? n_in : 0, n_mag = (size_t)nm * (size_t)nlev;
    const size_t planes = n_in + n_coord + n_out + n_mag;
    const size_t budget = (size_t)(mifc::env().vderiv_chunk_mib > 0 ? mifc::env().vderiv_chunk_mib : 256) << 20;
    size_t rows = std::max<size_t>(1, std::min<size_t>((size_t)a.ny, budget / (planes * nx * sizeof(float))));
    while (rows > 1 && planes * align_up(rows * nx, 64) * sizeof(float) > budget)
      rows -= 1;
    const size_t S = align_up(rows * nx, 64); // floats between the planes of the staged band: every plane on the 16-byte grid
    float* d = static_cast<float*>(st.scratch(planes * S * sizeof(float)));
    if (!st.ok())
      return 0;
    float* d_in = d;
    float* d_coord = d_in + n_in * S;
    float* d_out = d_coord + n_coord * S;
    float* d_mag = d_out + n_out * S;
    for (int f = 0; f < nf; ++f) {
      in[f] = d_in + (size_t)f * (size_t)nlev * S;
      out[f] = a.fres ? d_out + (size_t)f * (size_t)nlev * S : nullptr;
    }
    for (int j = 0; j < nm; ++j)
      mag[j] = d_mag + (size_t)j * (size_t)nlev * S;
    P.coord = by_level ? nullptr : d_coord;
    P.in_stride = (long)S;
    P.out_stride = (long)S;
    P.vec4 = 1; // a lane's four floats may straddle the end of the band: they stay inside the padded plane
    const size_t pitch = cells * sizeof(float), dpitch = S * sizeof(float);
    for (size_t r0 = 0; r0 < (size_t)a.ny; r0 += rows) {
      const size_t nr = std::min(rows, (size_t)a.ny - r0), n = nr * nx, width = n * sizeof(float), off = r0 * nx;
      for (int f = 0; f < nf; ++f)
        MIFC_HIP(c, hipMemcpy2DAsync(const_cast<float*>(in[f]), dpitch, a.fields[f] + off, pitch, width, (size_t)nlev, hipMemcpyHostToDevice, c->stream));
      if (n_coord != 0)
        MIFC_HIP(c, hipMemcpy2DAsync(d_coord, dpitch, a.coord + off, pitch, width, n_coord, hipMemcpyHostToDevice, c->stream));
      P.n = (int)n;
      if (!launch_passes())
        return 0;
      for (int f = 0; a.fres && f < nf; ++f)
        MIFC_HIP(c, hipMemcpy2DAsync(a.fres[f] + off, pitch, out[f], dpitch, width, (size_t)nlev, hipMemcpyDeviceToHost, c->stream));
      for (int j = 0; j < nm; ++j)
        MIFC_HIP(c, hipMemcpy2DAsync(a.fmag[j] + off, pitch, mag[j], dpitch, width, (size_t)nlev, hipMemcpyDeviceToHost, c->stream));
    }
  } else {
    uintptr_t all = by_level ? 0 : reinterpret_cast<uintptr_t>(a.coord);
    for (int f = 0; f < nf; ++f) {
      in[f] = a.fields[f];
      out[f] = a.fres ? a.fres[f] : nullptr;
      all |= reinterpret_cast<uintptr_t>(in[f]) | reinterpret_cast<uintptr_t>(out[f]);
    }
    for (int j = 0; j < nm; ++j) {
      mag[j] = a.fmag[j];
      all |= reinterpret_cast<uintptr_t>(mag[j]);
    }
    P.coord = by_level ? nullptr : a.coord;
    P.in_stride = (long)cells;
    P.out_stride = (long)cells;
    P.vec4 = ((cells & 3) == 0 && (all & 15) == 0) ? 1 : 0;
    P.n = (int)cells;
    if (!launch_passes())
      return 0;
  }
  std::vector<u64> counts;
  try {
    counts.assign(ncount, 0);
  } catch (...) {
    c->err = "out of host memory";
    return 0;
  }
  MIFC_HIP(c, hipMemcpyAsync(counts.data(), d_tab, ncount * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  if (!st.finish()) // nothing to copy back (the bands went as they were done): the synchronisation; `tab` was read by its copy
    return 0;
  for (size_t j = 0; a.fres && j < (size_t)nf * (size_t)nlev; ++j)
    a.fdefined_out[j] = mifc_classify(counts[j], (u64)cells);
  for (size_t j = 0; j < (size_t)nm * (size_t)nlev; ++j)
    a.fdefined_mag[j] = mifc_classify(counts[(size_t)nf * (size_t)nlev + j], (u64)cells);
  return 1;
}

} // namespace

extern "C" {

int mifc_vderiv_hlevels(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields, const float* ps,
                        int fdef_ps, const float* alevel, const float* blevel, int method, float* const* fres, int* fdefined_out,
                        float* const* fmag, int* fdefined_mag, float undef, int memkind)
{
  const Call a = {"mifc_vderiv_hlevels", mifc::VDERIV_HYBRID, nx, ny, nlev, fields, fdefined_in, nfields, ps, fdef_ps, nullptr, alevel, blevel,
                  method, fres, fdefined_out, fmag, fdefined_mag, undef, memkind};
  return run(c, a);
}

int mifc_vderiv_fields(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields, const float* coord,
                       const int* fdef_coord, int method, float* const* fres, int* fdefined_out, float* const* fmag, int* fdefined_mag,
                       float undef, int memkind)
{
  const Call a = {"mifc_vderiv_fields", mifc::VDERIV_FIELD, nx, ny, nlev, fields, fdefined_in, nfields, coord, MIFC_SOME_DEFINED, fdef_coord,
                  nullptr, nullptr, method, fres, fdefined_out, fmag, fdefined_mag, undef, memkind};
  return run(c, a);
}

int mifc_vderiv_levels(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields, const float* levels,
                       int method, float* const* fres, int* fdefined_out, float* const* fmag, int* fdefined_mag, float undef, int memkind)
{
  const Call a = {"mifc_vderiv_levels", mifc::VDERIV_LEVELS, nx, ny, nlev, fields, fdefined_in, nfields, levels, MIFC_SOME_DEFINED, nullptr,
                  nullptr, nullptr, method, fres, fdefined_out, fmag, fdefined_mag, undef, memkind};
  return run(c, a);
}

} // extern "C"
