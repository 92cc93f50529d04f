// mifc_capi_hinterp.hip -- C ABI of mifc_hinterp_levels and mifc_hinterp_vector_levels (include/mifc.h; EXTENSION, no
// reference function), one driver for both -- the vector form samples pairs and rotates them by rule R in the same
// launch (the ROTATE form of the kernel; the coefficients go up once, with the positions): its refusals
// (the head of the call, the overlap rule and the level table are the ones of mifc_levelbatch.h), the passes over the
// fields -- four per launch of the kernel of mifc_hinterp.hip, two with the bicubic method -- and, for host memory, the
// chunks of levels.  Levels are independent and a point may need any cell of a level, so host batches are staged whole
// levels at a time (the bands of rows of mifc_levelbatch.h's BandPlan cut through what a point reads): the positions go
// up once, then per chunk L levels of every field go up, the launches run and L * npos values per field come down.
#include "mifc_levelbatch.h"

#include <cstdio>

using namespace mifc_host;

static_assert(MIFC_HINTERP_NEAREST == mifc::HINTERP_NEAREST && MIFC_HINTERP_BILINEAR == mifc::HINTERP_BILINEAR &&
                  MIFC_HINTERP_BICUBIC == mifc::HINTERP_BICUBIC,
              "HinterpParams::method");

namespace {

// mifc_last_hinterp_form: the shape of the calling thread's last launch and the launches of its call
struct HinterpForm
{
  int method = -1, nf = 0, tested = 0, blocks = 0, level_chunks = 0, chunk = 0, launches = 0;
};
thread_local HinterpForm t_form;
thread_local char t_form_text[160];

// The levels of a staged chunk of a host-memory call: what fits `budget` bytes of device memory with every field's
// input levels and output levels in it, but never less than one level.
size_t levels_per_chunk(size_t budget, size_t nfields, size_t cells, size_t npos, size_t nlev)
{
  const size_t per_level = nfields * (cells + npos) * sizeof(float);
  return std::max<size_t>(1, std::min<size_t>(nlev, budget / per_level));
}

// the vector form: the fields are pairs u0, v0, u1, v1 ..., rotated with cosa[p], sina[p] (null: the plain form)
struct Rotation
{
  int npairs;
  const float *cosa, *sina;
  int fdef_rot;
};

int run(mifc_ctx* c, const char* name, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields, int npos,
        const float* xpos, const float* ypos, const Rotation* rot, int method, float* const* fres, int* fdefined_out, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  // (the head of a level-batch call without a coordinate: what the shared checks and the level table read)
  const LevelBatchCall a = {name, COORD_LEVELS, nx, ny, nlev, fields, fdefined_in, nfields, nullptr, MIFC_SOME_DEFINED, nullptr,
                            nullptr, nullptr, undef, memkind};
  if (c->capturing)
    return refuse(c, a, "not available while a mifc_graph capture is open");
  if (nlev < 1)
    return refuse(c, a, "nlev < 1");
  if (rot && nfields == 0)
    return refuse(c, a, "npairs " + std::to_string(rot->npairs) + " outside 1.." + std::to_string(mifc::HINTERP_MAX_FIELDS / 2));
  if (nfields < 1 || nfields > mifc::HINTERP_MAX_FIELDS)
    return refuse(c, a, "nfields " + std::to_string(nfields) + " outside 1.." + std::to_string(mifc::HINTERP_MAX_FIELDS));
  if (npos < 1)
    return refuse(c, a, "npos < 1");
  if (nx < 1 || ny < 1)
    return refuse(c, a, "nx < 1 or ny < 1");
  if (!check_grid(c, a) || !check_levels(c, a)) // memkind; the cell limit
    return 0;
  if (method != MIFC_HINTERP_NEAREST && method != MIFC_HINTERP_BILINEAR && method != MIFC_HINTERP_BICUBIC)
    return refuse(c, a, "unknown method " + std::to_string(method));
  if (rot && (!fields || !xpos || !ypos || !rot->cosa || !rot->sina || !fres || !fdefined_out))
    return refuse(c, a, "a null pointer (fields, xpos, ypos, cosa, sina, fres or fdefined_out)");
  if (!fields || !xpos || !ypos || !fres || !fdefined_out)
    return refuse(c, a, "a null pointer (fields, xpos, ypos, fres or fdefined_out)");
  if (!check_field_pointers(c, a, fres))
    return 0;
  const int nf = nfields;
  const size_t cells = a.cells(), points = (size_t)npos, levels = (size_t)nlev;
  if (!check_overlaps(c, a, {{fres, nf, levels * points * sizeof(float), "fres"}},
                      {{xpos, points * sizeof(float), "xpos"},
                       {ypos, points * sizeof(float), "ypos"},
                       {rot ? rot->cosa : nullptr, points * sizeof(float), "cosa"},
                       {rot ? rot->sina : nullptr, points * sizeof(float), "sina"}}))
    return 0;

  // one counter per field and level -- per PAIR and level in the vector form --, then the one of the unusable positions
  const size_t n_results = rot ? (size_t)(nf / 2) : (size_t)nf, n_counts = n_results * levels;
  LevelTable tab;
  Staging st(c, memkind);
  if (!tab.build(c, a, n_counts + 1) || !tab.upload(c, st))
    return 0;
  bool tested = false;
  for (size_t j = 0; j < (size_t)nf * levels; ++j)
    tested |= !fdefined_in || fdefined_in[j] != MIFC_ALL_DEFINED;

  mifc::HinterpRotateParams P; // (the plain form launches its HinterpParams part)
  std::memset(&P, 0, sizeof P);
  P.method = method;
  P.nx = nx;
  P.ny = ny;
  P.npos = npos;
  P.call_nlev = nlev;
  P.tested = tested ? 1 : 0;
  P.undef = undef;
  P.in_stride = (long)cells;
  P.out_stride = (long)npos;
  P.lev_bits = tab.lev_bits();
  P.n_undefined = tab.n_undefined();
  P.n_unusable = tab.n_undefined() + n_counts;
  P.xpos = st.in(xpos, points);
  P.ypos = st.in(ypos, points);
  if (rot) {
    P.cosa = st.in(rot->cosa, points);
    P.sina = st.in(rot->sina, points);
    P.rot_all = rot->fdef_rot == MIFC_ALL_DEFINED ? 1 : 0;
  }
  if (!st.ok())
    return 0;

  // host memory: L levels of every field in, L levels of every output, in one block
  const bool host = memkind == MIFC_MEM_HOST;
  const size_t L = host ? levels_per_chunk((size_t)(mifc::env().hinterp_chunk_mib > 0 ? mifc::env().hinterp_chunk_mib : 256) << 20, (size_t)nf,
                                           cells, points, levels)
                        : levels;
  float* staged = nullptr;
  if (host) {
    staged = static_cast<float*>(st.scratch((size_t)nf * L * (cells + points) * sizeof(float)));
    if (!st.ok())
      return 0;
  }
  const int pass = mifc::hinterp_pass_fields(method);
  HinterpForm form;
  form.method = method;
  form.tested = P.tested;
  form.nf = std::min(pass, nf);
  for (size_t k0 = 0; k0 < levels; k0 += L) {
    const size_t n = std::min(L, levels - k0);
    const float* in[mifc::HINTERP_MAX_FIELDS];
    float* out[mifc::HINTERP_MAX_FIELDS];
    for (int f = 0; f < nf; ++f) {
      if (host) {
        float* d = staged + (size_t)f * L * cells;
        MIFC_HIP(c, hipMemcpyAsync(d, fields[f] + k0 * cells, n * cells * sizeof(float), hipMemcpyHostToDevice, c->stream));
        in[f] = d;
        out[f] = staged + (size_t)nf * L * cells + (size_t)f * L * points;
      } else {
        in[f] = fields[f];
        out[f] = fres[f];
      }
    }
    P.nlev = (int)n;
    P.lev0 = (int)k0;
    const mifc::HinterpPlan plan = mifc::hinterp_plan(npos, P.nlev);
    for (int f0 = 0; f0 < nf; f0 += pass) {
      P.f0 = f0;
      P.nfields = std::min(pass, nf - f0);
      P.count_unusable = (k0 == 0 && f0 == 0) ? 1 : 0;
      for (int f = 0; f < P.nfields; ++f) {
        P.fields[f] = in[f0 + f];
        P.out[f] = out[f0 + f];
      }
      if (rot)
        MIFC_LAUNCH(c, mifc::launch_hinterp_rotate(P, c->stream));
      else
        MIFC_LAUNCH(c, mifc::launch_hinterp(P, c->stream));
      form.launches += 1;
    }
    form.blocks = plan.blocks;
    form.level_chunks = plan.level_chunks;
    form.chunk = plan.chunk;
    if (host)
      for (int f = 0; f < nf; ++f)
        MIFC_HIP(c, hipMemcpyAsync(fres[f] + k0 * points, out[f], n * points * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  }
  if (!tab.read_counts(c) || !st.finish()) // finish(): the one synchronisation of the call
    return 0;
  t_form = form;
  const u64 unusable = tab.count(n_counts);
  for (size_t j = 0; j < n_counts; ++j) {
    const int flag = mifc_classify(tab.count(j) + unusable, (u64)points);
    if (rot) { // R4: both components of a pair carry the pair's flag
      const size_t q = j / levels, k = j % levels;
      fdefined_out[(2 * q) * levels + k] = fdefined_out[(2 * q + 1) * levels + k] = flag;
    } else {
      fdefined_out[j] = flag;
    }
  }
  return 1;
}

} // namespace

extern "C" {

int mifc_hinterp_levels(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields, int npos,
                        const float* xpos, const float* ypos, int method, float* const* fres, int* fdefined_out, float undef, int memkind)
{
  return run(c, "mifc_hinterp_levels", nx, ny, nlev, fields, fdefined_in, nfields, npos, xpos, ypos, nullptr, method, fres, fdefined_out, undef, memkind);
}

int mifc_hinterp_vector_levels(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int npairs, int npos,
                               const float* xpos, const float* ypos, const float* cosa, const float* sina, int fdef_rot, int method,
                               float* const* fres, int* fdefined_out, float undef, int memkind)
{
  const Rotation rot = {npairs, cosa, sina, fdef_rot};
  const int nfields = npairs >= 1 && npairs <= mifc::HINTERP_MAX_FIELDS / 2 ? 2 * npairs : 0; // (0: refused by name)
  return run(c, "mifc_hinterp_vector_levels", nx, ny, nlev, fields, fdefined_in, nfields, npos, xpos, ypos, &rot, method, fres, fdefined_out, undef,
             memkind);
}

const char* mifc_last_hinterp_form(void)
{
  static const char* const names[] = {"nearest", "bilinear", "bicubic"};
  const HinterpForm& f = t_form;
  if (f.method < 0)
    return "";
  std::snprintf(t_form_text, sizeof t_form_text, "method=%s nf=%d tested=%d blocks=%d level_chunks=%d chunk=%d launches=%d", names[f.method], f.nf,
                f.tested, f.blocks, f.level_chunks, f.chunk, f.launches);
  return t_form_text;
}

} // extern "C"
