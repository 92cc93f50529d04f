// mifc_capi_fexpr.hip -- C ABI of mifc_fexpr_levels (include/mifc.h; EXTENSION, no reference function) on the level-batch
// driver (mifc_levelbatch.h): the head checks, the overlap rule and the level table of the siblings -- the table's tail
// carries the level scalars --, the program check of mifc_fexpr_prog.h, and one launch of the interpreter of
// mifc_fexpr.hip per problem.  Cells are independent, so a host batch goes band by band (BandPlan, halo 0), the planes as
// groups of one plane; the band budget is MIFC_FEXPR_CHUNK_MIB.
#include "mifc_fexpr_prog.h"
#include "mifc_levelbatch.h"

#include <cstdio>

using namespace mifc_host;

namespace {

// mifc_last_fexpr_form: the shape of the calling thread's last launch and the problems of its call
struct FexprForm
{
  int vector = 0, grid = 0, nlev = 0, ncode = 0, nregs = 0, nout = 0, tail = 0, tables = 0, bands = 0;
};
thread_local FexprForm t_form;
thread_local char t_form_text[192];

} // namespace

extern "C" {

int mifc_fexpr_levels(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, int nfields, const float* const* planes, int nplanes,
                      const float* level_scalars, int nscalars, const float* consts, int nconsts, const mifc_fexpr_ins* code, int ncode,
                      const int* out_regs, int nout, float* const* fres, int* fdefined_out, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  // (the head of a level-batch call without a coordinate: what the shared checks and the level table read)
  const bool counted = nfields >= 0 && nfields <= MIFC_FEXPR_MAX_FIELDS;
  const LevelBatchCall a = {"mifc_fexpr_levels", COORD_LEVELS, nx, ny, nlev, fields, nullptr, counted ? nfields : 0, nullptr, MIFC_SOME_DEFINED,
                            nullptr, nullptr, nullptr, undef, memkind};
  if (c->capturing)
    return refuse(c, a, "not available while a mifc_graph capture is open");
  if (nlev < 1)
    return refuse(c, a, "nlev < 1");
  mifc_fexpr::Program prog;
  char why[128];
  if (!mifc_fexpr::check(nfields, nplanes, nscalars, nconsts, code, ncode, out_regs, nout, &prog, why, sizeof why))
    return refuse(c, a, why);
  if (!check_grid(c, a) || !check_levels(c, a)) // a negative nx or ny, memkind; the cell limit
    return 0;
  if ((nfields > 0 && !fields) || (nplanes > 0 && !planes) || (nscalars > 0 && !level_scalars) || (nconsts > 0 && !consts) || !fres || !fdefined_out)
    return refuse(c, a, "a null pointer (fields, planes, level_scalars, consts, fres or fdefined_out)");
  if (!check_field_pointers(c, a, nullptr))
    return 0;
  for (int p = 0; p < nplanes; ++p)
    if (!planes[p])
      return refuse(c, a, "a null pointer (planes[" + std::to_string(p) + "])");
  for (int o = 0; o < nout; ++o)
    if (!fres[o])
      return refuse(c, a, "a null pointer (fres[" + std::to_string(o) + "])");
  const size_t cells = a.cells(), levels = (size_t)nlev;
  const float* pl[MIFC_FEXPR_MAX_PLANES] = {nullptr, nullptr, nullptr, nullptr};
  for (int p = 0; p < nplanes; ++p)
    pl[p] = planes[p];
  if (!check_overlaps(c, a, {{fres, nout, levels * cells * sizeof(float), "fres"}},
                      {{pl[0], cells * sizeof(float), "planes[0]"},
                       {pl[1], cells * sizeof(float), "planes[1]"},
                       {pl[2], cells * sizeof(float), "planes[2]"},
                       {pl[3], cells * sizeof(float), "planes[3]"}}))
    return 0;
  const size_t n_counts = (size_t)nout * levels; // one counter per output and level
  if (cells == 0) {                              // nothing to compute: flags only
    for (size_t j = 0; j < n_counts; ++j)
      fdefined_out[j] = mifc_classify(0, 0);
    return 1;
  }

  LevelTable tab;
  Staging st(c, memkind); // blocks only: a host batch is staged band by band
  const size_t scalar_bytes = (size_t)nscalars * levels * sizeof(float);
  if (!tab.build(c, a, n_counts, scalar_bytes))
    return 0;
  if (scalar_bytes != 0)
    std::memcpy(tab.tail(), level_scalars, scalar_bytes);
  if (!tab.upload(c, st))
    return 0;

  BandPlan plan;
  PlaneGroup *in[mifc::FEXPR_MAX_IN], *out[mifc::FEXPR_MAX_OUT];
  for (int f = 0; f < nfields; ++f)
    in[f] = plan.in(fields[f], levels);
  for (int p = 0; p < nplanes; ++p)
    in[nfields + p] = plan.in(planes[p], 1);
  for (int o = 0; o < nout; ++o)
    out[o] = plan.out(fres[o], levels);
  if (!plan.place(c, st, a, (size_t)(mifc::env().fexpr_chunk_mib > 0 ? mifc::env().fexpr_chunk_mib : 256) << 20))
    return 0;

  mifc::FexprParams P;
  std::memset(&P, 0, sizeof P);
  P.nlev_all = nlev;
  P.ncode = ncode;
  P.nfields = nfields;
  P.nplanes = nplanes;
  P.nout = nout;
  P.undef = undef;
  P.stride = plan.stride;
  for (int i = 0; i < nfields + nplanes; ++i)
    P.in[i] = in[i]->dev;
  for (int o = 0; o < nout; ++o) {
    P.out[o] = out[o]->dev;
    P.out_regs |= (unsigned int)prog.out_regs[o] << (8 * o);
  }
  P.level_scalars = static_cast<const float*>(tab.dev_tail());
  P.n_undefined = tab.n_undefined();
  for (int i = 0; i < ncode; ++i) {
    const mifc_fexpr_ins& w = prog.code[i];
    P.code[2 * i] = (unsigned int)w.op | (unsigned int)w.dst << 8 | (unsigned int)w.a << 16 | (unsigned int)w.b << 24;
    P.code[2 * i + 1] = w.c;
  }
  for (int j = 0; j < nconsts; ++j)
    P.consts[j] = consts[j];

  FexprForm form;
  form.nlev = nlev;
  form.ncode = ncode;
  form.nregs = prog.nregs;
  form.nout = nout;
  form.tables = prog.tables;
  auto launch = [&](const BandRows& rows) -> int { // one problem of rows.n() cells
    P.n = rows.n();
    MIFC_LAUNCH(c, mifc::launch_fexpr(P, nlev, prog.tables, c->stream));
    const mifc::FexprShape shape = mifc::fexpr_shape(P);
    form.vector = shape.vector;
    form.grid = shape.grid;
    form.tail = shape.tail;
    form.bands += 1;
    return 1;
  };
  if (!plan.run(c, a, launch) || !tab.read_counts(c) || !st.finish()) // finish(): the one synchronisation of the call
    return 0;
  t_form = form;
  for (size_t j = 0; j < n_counts; ++j) // rule 5
    fdefined_out[j] = tab.classify(j, cells);
  return 1;
}

const char* mifc_last_fexpr_form(void)
{
  const FexprForm& f = t_form;
  if (f.bands == 0)
    return "";
  std::snprintf(t_form_text, sizeof t_form_text, "family=fexpr form=%s grid=%d nlev=%d ncode=%d nregs=%d nout=%d tail=%d partials=0 tables=%d bands=%d",
                f.vector ? "vector" : "scalar", f.grid, f.nlev, f.ncode, f.nregs, f.nout, f.tail, f.tables, f.bands);
  return t_form_text;
}

} // extern "C"
