// mifc_capi_icing.hip -- C ABI of the iterative vessel-icing models, vesselIcingModStall
// (FieldCalculationsVesselIcing.cc:182-337) and vesselIcingMincog (:677-705): the reference's argument checks, the
// per-call constants on the host (mifc_icing_cell.h), then the kernel of mifc_icing.hip.
#include "mifc_ctx.h"
#include "mifc_icing_cell.h"

#include <cstring>
#include <string>
#include <vector>

using namespace mifc_host;

namespace {

const int ICING_NIN = 11;

// fdefined[nlev] in/out.  Returns 1 on success, 0 for the reference's `false` (c->err empty) or a refusal / HIP failure
// (c->err says which).  Nothing is written unless every check passed.
int icing_run(mifc_ctx* c, const char* fn, int model, int nlev, int nx, int ny, const float* const* in, unsigned shared_mask, float vs, float alpha,
              float zmin, float zmax, int alt, float* out, int* fdefined, float undef, int memkind)
{
  const long cells64 = (long)nx * (long)ny;
  if (nx < 0 || ny < 0 || cells64 > 0x7fffffffL || !out || !fdefined || nlev < 1)
    return 0;
  for (int k = 0; k < ICING_NIN; ++k)
    if (!in[k])
      return 0;
  mifc_icing::IcingConsts C;
  const int rc = mifc_icing::icing_consts(model, vs, alpha, zmin, zmax, alt, &C);
  if (rc == 0) // :195-201, :688
    return 0;
  if (rc < 0) {
    c->err = std::string(fn) + ": (zmax - zmin) * 2 + 1 levels do not fit an int (the reference's conversion is undefined)";
    return 0;
  }
  if (cells64 > 0 && (long)nlev > 0x7fffffffL / cells64) {
    c->err = std::string(fn) + ": the batch holds more than 2^31 - 1 cells";
    return 0;
  }
  const size_t cells = (size_t)cells64, n = cells * (size_t)nlev;
  if (memkind == MIFC_MEM_DEVICE && nlev > 1)
    for (int k = 0; k < ICING_NIN; ++k)
      if (((shared_mask >> k) & 1u) && overlaps(out, n * sizeof(float), in[k], cells * sizeof(float))) {
        c->err = std::string(fn) + ": out overlaps an input shared by every level (other levels still read it)";
        return 0;
      }
  if (cells == 0) {
    for (int l = 0; l < nlev; ++l)
      fdefined[l] = MIFC_ALL_DEFINED; // checkDefined(0, 0)
    return 1;
  }

  mifc::IcingParams P;
  std::memset(&P, 0, sizeof P);
  P.nlev = nlev;
  P.n = (int)cells;
  P.level_stride = (long)cells;
  P.undef = undef;
  P.model = C.model;
  P.alt = C.alt;
  P.number = C.number;
  P.bisect_iter = C.bisect_iter;
  P.vs = C.vs;
  P.cos_alpha = C.cos_alpha;
  P.sin_beta = C.sin_beta;
  P.drag = C.drag;
  P.Swdown = C.Swdown;
  P.vs_cos_d = C.vs_cos_d;
  P.cos_d = C.cos_d;
  for (int k = 0; k < 2; ++k) {
    P.br_sin2[k] = C.br_sin2[k];
    P.br_cos[k] = C.br_cos[k];
    P.br_cos2[k] = C.br_cos2[k];
  }

  // one scratch block: counts (u64 [nlev]), level factors (double [number], only past the kernel-argument table), flags (uchar [nlev])
  const bool buf = C.number > mifc::ICING_KARG_LEVELS;
  const size_t tab_bytes = buf ? (size_t)C.number * sizeof(double) : 0;
  const size_t cnt_bytes = (size_t)nlev * sizeof(u64);
  std::vector<unsigned char> host(tab_bytes + (size_t)nlev);
  for (int k = 0; k < C.number; ++k) {
    const double e = mifc_icing::icing_level_factor(zmin, k);
    if (buf)
      std::memcpy(host.data() + (size_t)k * sizeof(double), &e, sizeof e);
    else
      P.lev[k] = e;
  }
  for (int l = 0; l < nlev; ++l)
    host[tab_bytes + (size_t)l] = fdefined[l] == MIFC_ALL_DEFINED ? 1 : 0;
  Staging st(c, memkind);
  unsigned char* d_tab = static_cast<unsigned char*>(st.scratch(cnt_bytes + host.size()));
  if (!st.ok())
    return 0;
  P.n_undefined = reinterpret_cast<u64*>(d_tab);
  P.lev_buf = buf ? reinterpret_cast<const double*>(d_tab + cnt_bytes) : nullptr;
  P.all_defined = d_tab + cnt_bytes + tab_bytes;

  for (int k = 0; k < ICING_NIN; ++k) {
    const bool shared = (shared_mask >> k) & 1u;
    P.in[k] = st.in(in[k], shared ? cells : n);
    P.in_stride[k] = shared ? 0 : (long)cells;
  }
  P.out = st.out(out, n);
  if (!st.ok())
    return 0;
  MIFC_HIP(c, hipMemcpyAsync(d_tab + cnt_bytes, host.data(), host.size(), hipMemcpyHostToDevice, c->stream));
  MIFC_HIP(c, hipMemsetAsync(d_tab, 0, cnt_bytes, c->stream));
  MIFC_LAUNCH(c, mifc::launch_vessel_icing(P, c->stream));
  std::vector<u64> counts((size_t)nlev);
  MIFC_HIP(c, hipMemcpyAsync(counts.data(), d_tab, cnt_bytes, hipMemcpyDeviceToHost, c->stream));
  if (!st.finish())
    return 0;
  for (int l = 0; l < nlev; ++l)
    fdefined[l] = mifc_classify(counts[(size_t)l], (u64)cells); // :335, :703
  return 1;
}

} // namespace

extern "C" {

int mifc_vesselIcingModStall(mifc_ctx* c, int nx, int ny, const float* sal, const float* wave, const float* x_wind, const float* y_wind,
                             const float* airtemp, const float* rh, const float* sst, const float* p, const float* Pw, const float* aice,
                             const float* depth, float vs, float alpha, float zmin, float zmax, float* icing, int* fdefined, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  const float* in[ICING_NIN] = {sal, wave, x_wind, y_wind, airtemp, rh, sst, p, Pw, aice, depth};
  return icing_run(c, "vesselIcingModStall", mifc_icing::MODSTALL, 1, nx, ny, in, 0u, vs, alpha, zmin, zmax, 1, icing, fdefined, undef, memkind);
}

int mifc_vesselIcingMincog(mifc_ctx* c, int nx, int ny, const float* sal, const float* wave, const float* x_wind, const float* y_wind,
                           const float* airtemp, const float* rh, const float* sst, const float* p, const float* Pw, const float* aice,
                           const float* depth, float vs, float alpha, float zmin, float zmax, int alt, float* icing, int* fdefined, float undef,
                           int memkind)
{
  CTX_OR_FAIL(c);
  const float* in[ICING_NIN] = {sal, wave, x_wind, y_wind, airtemp, rh, sst, p, Pw, aice, depth};
  return icing_run(c, "vesselIcingMincog", mifc_icing::MINCOG, 1, nx, ny, in, 0u, vs, alpha, zmin, zmax, alt, icing, fdefined, undef, memkind);
}

int mifc_vesselIcing_levels(mifc_ctx* c, int model, int nlev, int nx, int ny, const float* sal, const float* wave, const float* x_wind,
                            const float* y_wind, const float* airtemp, const float* rh, const float* sst, const float* p, const float* Pw,
                            const float* aice, const float* depth, unsigned int shared_mask, float vs, float alpha, float zmin, float zmax, int alt,
                            float* icing, int* fdefined, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  if (model != MIFC_ICING_MODSTALL && model != MIFC_ICING_MINCOG) {
    c->err = "mifc_vesselIcing_levels: model must be MIFC_ICING_MODSTALL or MIFC_ICING_MINCOG";
    return 0;
  }
  const float* in[ICING_NIN] = {sal, wave, x_wind, y_wind, airtemp, rh, sst, p, Pw, aice, depth};
  const int m = model == MIFC_ICING_MODSTALL ? mifc_icing::MODSTALL : mifc_icing::MINCOG;
  return icing_run(c, model == MIFC_ICING_MODSTALL ? "vesselIcingModStall" : "vesselIcingMincog", m, nlev, nx, ny, in, shared_mask, vs, alpha, zmin,
                   zmax, alt, icing, fdefined, undef, memkind);
}

} // extern "C"
