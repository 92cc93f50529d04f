// mifc_capi_vrotate.hip -- C ABI of mifc_vrotate_levels (include/mifc.h, rule R; EXTENSION, no reference function) on the
// level-batch driver (mifc_levelbatch.h): its own refusals, the head, the overlap rule and the level table of the
// siblings, every pair of the call in one launch of the kernel of mifc_vrotate.hip.  Cells are independent, so a host
// batch goes band by band (BandPlan), the two coefficient planes as groups of one plane; the band budget is the one of
// the other vector product of level batches, the magnitude of mifc_vderiv_* (MIFC_VDERIV_CHUNK_MIB).
#include "mifc_levelbatch.h"

#include <cstdio>

using namespace mifc_host;

namespace {

// mifc_last_vrotate_form: the shape of the calling thread's last launch and the launches of its call
struct VrotateForm
{
  int v = 0, np = 0, tested = 0, blocks = 0, level_chunks = 0, chunk = 0, launches = 0;
};
thread_local VrotateForm t_form;
thread_local char t_form_text[160];

} // namespace

extern "C" {

int mifc_vrotate_levels(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int npairs, const float* cosa,
                        const float* sina, int fdef_rot, float* const* fres, int* fdefined_out, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  // (the head of a level-batch call without a coordinate: what the shared checks and the level table read; the fields
  // are u0, v0, u1, v1 ...)
  const bool counted = npairs >= 1 && npairs <= mifc::VROTATE_MAX_PAIRS;
  const LevelBatchCall a = {"mifc_vrotate_levels", COORD_LEVELS, nx, ny, nlev, fields, fdefined_in, counted ? 2 * npairs : 0, nullptr, MIFC_SOME_DEFINED,
                            nullptr, nullptr, nullptr, undef, memkind};
  if (c->capturing)
    return refuse(c, a, "not available while a mifc_graph capture is open");
  if (nlev < 1)
    return refuse(c, a, "nlev < 1");
  if (!counted)
    return refuse(c, a, "npairs " + std::to_string(npairs) + " outside 1.." + std::to_string(mifc::VROTATE_MAX_PAIRS));
  if (nx < 1 || ny < 1)
    return refuse(c, a, "nx < 1 or ny < 1");
  if (!check_grid(c, a) || !check_levels(c, a)) // memkind; the cell limit
    return 0;
  if (!fields || !cosa || !sina || !fres || !fdefined_out)
    return refuse(c, a, "a null pointer (fields, cosa, sina, fres or fdefined_out)");
  if (!check_field_pointers(c, a, fres))
    return 0;
  const int nf = a.nfields;
  const size_t cells = a.cells(), levels = (size_t)nlev;
  if (!check_overlaps(c, a, {{fres, nf, levels * cells * sizeof(float), "fres"}},
                      {{cosa, cells * sizeof(float), "cosa"}, {sina, cells * sizeof(float), "sina"}}))
    return 0;

  const size_t n_counts = (size_t)npairs * levels; // one counter per pair and level
  LevelTable tab;
  Staging st(c, memkind); // blocks only: a host batch is staged band by band
  if (!tab.build(c, a, n_counts) || !tab.upload(c, st))
    return 0;
  const bool rot_all = fdef_rot == MIFC_ALL_DEFINED;
  bool tested = !rot_all;
  for (size_t j = 0; j < (size_t)nf * levels; ++j)
    tested |= !fdefined_in || fdefined_in[j] != MIFC_ALL_DEFINED;

  BandPlan plan;
  PlaneGroup *in[2 * mifc::VROTATE_MAX_PAIRS], *out[2 * mifc::VROTATE_MAX_PAIRS];
  for (int f = 0; f < nf; ++f)
    in[f] = plan.in(fields[f], levels);
  PlaneGroup *pc = plan.in(cosa, 1), *ps = plan.in(sina, 1);
  for (int f = 0; f < nf; ++f)
    out[f] = plan.out(fres[f], levels);
  if (!plan.place(c, st, a, (size_t)(mifc::env().vderiv_chunk_mib > 0 ? mifc::env().vderiv_chunk_mib : 256) << 20))
    return 0;

  mifc::VrotateParams P;
  std::memset(&P, 0, sizeof P);
  P.npairs = npairs;
  P.nlev = nlev;
  P.tested = tested ? 1 : 0;
  P.rot_all = rot_all ? 1 : 0;
  P.vec4 = plan.vec4;
  P.undef = undef;
  P.in_stride = P.out_stride = plan.stride;
  for (int f = 0; f < nf; ++f) {
    P.fields[f] = in[f]->dev;
    P.out[f] = out[f]->dev;
  }
  P.cosa = pc->dev;
  P.sina = ps->dev;
  P.lev_bits = tab.lev_bits();
  P.n_undefined = tab.n_undefined();

  VrotateForm form;
  form.v = plan.vec4 ? 4 : 1;
  form.np = npairs;
  form.tested = P.tested;
  auto launch = [&](const BandRows& rows) -> int { // one problem of rows.n() cells
    P.n = rows.n();
    MIFC_LAUNCH(c, mifc::launch_vrotate(P, c->stream));
    const mifc::VrotatePlan shape = mifc::vrotate_plan(P.n, nlev, P.vec4);
    form.blocks = shape.blocks;
    form.level_chunks = shape.level_chunks;
    form.chunk = shape.chunk;
    form.launches += 1;
    return 1;
  };
  if (!plan.run(c, a, launch) || !tab.read_counts(c) || !st.finish()) // finish(): the one synchronisation of the call
    return 0;
  t_form = form;
  for (size_t j = 0; j < n_counts; ++j) { // R4: both components of a pair carry the pair's flag
    const size_t q = j / levels, k = j % levels;
    fdefined_out[(2 * q) * levels + k] = fdefined_out[(2 * q + 1) * levels + k] = tab.classify(j, cells);
  }
  return 1;
}

const char* mifc_last_vrotate_form(void)
{
  const VrotateForm& f = t_form;
  if (f.launches == 0)
    return "";
  std::snprintf(t_form_text, sizeof t_form_text, "v=%d np=%d tested=%d blocks=%d level_chunks=%d chunk=%d launches=%d", f.v, f.np, f.tested, f.blocks,
                f.level_chunks, f.chunk, f.launches);
  return t_form_text;
}

} // extern "C"
