// mifc_stencil_host.h -- the host-side description of a stencil request, shared by the stencil boundary
// (mifc_capi_stencil.hip, which implements what is declared here unless noted), the two-stage operators and the Shapiro
// filter (mifc_capi_twostage.hip) and the row-slab plan (mifc_slab.hip).  Not installed.
#ifndef MIFC_STENCIL_HOST_H
#define MIFC_STENCIL_HOST_H

#include "mifc_ctx.h"

namespace mifc_host {

// One stencil request on the fields as the kernels see them.  The members after o1 default to zero: a whole field
// (no slab, no row range), scalars unused.
struct StencilCall
{
  int op;
  int nx, ny, nlev; // ny: rows of the whole field
  const float *f0, *f1, *xm, *ym, *fc;
  float *o0, *o1;
  const float* f2; // third input field (advection)
  float scale;     // advection, Q-vector
  float scale2;    // Q-vector
  const float* scale_lev;  // Q-vector over a level batch: per-level tables on the device (or null)
  const float* scale2_lev;
  int j0, ny_local;                       // row slab: first owned global row, owned rows (0: all ny rows, from row 0)
  long in_level_stride, out_level_stride; // elements between levels (run_stencil() fills in nx * ny itself)
  int row_begin, row_end;                 // owned output rows of this launch (0, 0: all)
  float* out_ff;                          // ST_VORTDIV: the wind speed as a third output (or null)
};

// The request as kernel parameters: every field of StencilParams that describes the request (flags, counters and
// partials are the launch's own business: prepare_levels, stencil_partials).  ST_VORTDIV with one output missing
// becomes ST_DIVERGENCE / ST_RELVORT.
mifc::StencilParams stencil_params(const StencilCall& sc, float undef);

// One tested level of a big field through the one-shot stencil kernels: room for their workgroups' counts
// (StencilParams::partials) in the context's buffer.
void stencil_partials(mifc_ctx* c, mifc::StencilParams& P);

// The synchronous stencil driver, single field or level batch: stages the request's fields (memkind), launches, reads the
// counts back and classifies.  fdefined[nlev]: the input flags, then the output flags.  Notes its kernel form.
int run_stencil(mifc_ctx* c, const StencilCall& sc, int* fdefined, float undef, int memkind);

// mifc_capi_twostage.hip: the MIFC_OP_TFP, MIFC_OP_QVECTOR and MIFC_OP_SHAPIRO2 branches of mifc_stencil_levels_ex, after its
// checks of nx, ny, nlev, f0, out0 and fdefined
int two_stage_levels_ex(mifc_ctx* c, int op, int nx, int ny, int nlev, const float* f0, const float* f1, const float* xmapr, const float* ymapr,
                        const float* fcoriolis, const float* level_scalars, int compute, float* out0, int* fdefined, float undef, int memkind);

} // namespace mifc_host

#endif // MIFC_STENCIL_HOST_H
