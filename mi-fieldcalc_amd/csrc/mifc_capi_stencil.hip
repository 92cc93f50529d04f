// mifc_capi_stencil.hip -- the extern "C" boundary of the stencil operators (mifc_stencil*.hip, mifc_vortdiv.hip,
// mifc_advection.hip): the single-field entries, the level batches in their synchronous and *_enqueue forms and the
// row-slab launches, on ONE preparation path: a StencilCall becomes StencilParams in
// stencil_params() and the per-level flags and counters are put in place by prepare_levels().  The two-stage operators and
// the Shapiro filter live in mifc_capi_twostage.hip; their passes come back here through run_stencil().

#include <cstring>

#include "mifc_stencil_host.h"

namespace mifc_host {

// Not while a capture is recorded (the buffer is the context's ONE, calls recorded side by side would share it; and growing
// it frees memory): those launches keep one atomic per workgroup.
void stencil_partials(mifc_ctx* c, mifc::StencilParams& P)
{
  P.partials = nullptr;
  P.partials_cap = 0;
  if (P.every_level_all_defined || c->capturing)
    return;
  // the forms' units per level: 4-row (one-input one-shot), 8-row (wind one-shot tiles) or 8- to 14-row (level-walking tiles)
  // blocks x 256-column segments; bounded from above.  Small levels keep their atomics (a few hundred per counter).
  const size_t per_level = (size_t)(P.ny_local / 4 + 2) * (size_t)(P.nx / 256 + 1);
  const size_t units = per_level * (size_t)P.nlev;
  if (per_level < 2048 || units > ((size_t)1 << 24))
    return;
  int cap = 0;
  P.partials = partials_for(c, units * 1024, &cap);
  P.partials_cap = P.partials ? cap : 0;
}

mifc::StencilParams stencil_params(const StencilCall& sc, float undef)
{
  mifc::StencilParams P;
  std::memset(&P, 0, sizeof P);
  P.op = sc.op;
  P.out0 = sc.o0;
  P.out1 = sc.o1;
  if (sc.op == mifc::ST_VORTDIV && !sc.o0 && sc.o1) { // only divergence requested
    P.op = mifc::ST_DIVERGENCE;
    P.out0 = sc.o1;
    P.out1 = nullptr;
  } else if (sc.op == mifc::ST_VORTDIV && !sc.o1) {
    P.op = mifc::ST_RELVORT;
  }
  P.out_ff = sc.out_ff;
  P.nx = sc.nx;
  P.ny_global = sc.ny;
  P.j0 = sc.j0;
  P.ny_local = sc.ny_local ? sc.ny_local : sc.ny;
  P.nlev = sc.nlev;
  P.f0 = sc.f0;
  P.f1 = sc.f1;
  P.f2 = sc.f2;
  P.xmapr = sc.xm;
  P.ymapr = sc.ym;
  P.fcoriolis = sc.fc;
  P.scale = sc.scale;
  P.scale2 = sc.scale2;
  P.scale_lev = sc.scale_lev;
  P.scale2_lev = sc.scale2_lev;
  P.in_level_stride = sc.in_level_stride;
  P.out_level_stride = sc.out_level_stride;
  P.row_begin = sc.row_begin;
  P.row_end = sc.row_end;
  P.undef = undef;
  return P;
}

} // namespace mifc_host

using namespace mifc_host;

namespace {

// ---- operator classes --------------------------------------------------------
enum
{
  OPC_TAKES_F1 = 1,      // reads a second input field f1
  OPC_NEEDS_FC = 2,      // reads the Coriolis parameter
  OPC_TWO_OUTPUTS = 4,
  OPC_ALWAYS_COUNTS = 8, // rejects cells even when the input flag is ALL_DEFINED: the second pass of thermalFrontParameter
                         // (|grad T| == 0) and the last pass of plevelqvector (:570) always run the counting variant
};

unsigned op_class(int op)
{
  unsigned k = 0;
  if (op <= mifc::ST_VORTDIV || op >= mifc::ST_ADVECTION) // the wind pair; advection, jacobian, the TFP and Q-vector passes
    k |= OPC_TAKES_F1;
  if (op == mifc::ST_ABSVORT || (op >= mifc::ST_GWIND_X && op <= mifc::ST_IGWIND))
    k |= OPC_NEEDS_FC;
  if (op == mifc::ST_VORTDIV || op == mifc::ST_IGWIND)
    k |= OPC_TWO_OUTPUTS;
  if (op == mifc::ST_TFP || op == mifc::ST_QVEC_X || op == mifc::ST_QVEC_Y)
    k |= OPC_ALWAYS_COUNTS;
  return k;
}

// what mifc_stencil_levels and mifc_stencil_levels_enqueue offer
bool is_level_batch_op(int op)
{
  return (op >= mifc::ST_RELVORT && op <= mifc::ST_IGWIND) || op == mifc::ST_JACOBIAN;
}

// count range of the raw loop -> what the flag is classified against
u64 stencil_denominator(int op, int nx, int ny)
{
  const u64 n = (u64)nx * (u64)ny;
  if (op == mifc::ST_IGWIND)
    return n; // FieldCalculations.cc:1543
  return n - 2 * (u64)nx; // :1868 and friends, also gradient compute 1 (:2068)
}

// ---- per-level flags and counters in front of a launch ----------------------------
inline bool level_all_defined(const int* fdefined, int l)
{
  return fdefined && fdefined[l] == MIFC_ALL_DEFINED;
}

// nlev counters zeroed on the stream: by the small kernel, very deep batches by a fill
int zero_level_counts(mifc_ctx* c, u64* counts, int nlev)
{
  if (nlev <= mifc::kPrepMaxLevels)
    MIFC_HIP(c, mifc::launch_prep_levels(nullptr, nlev, nullptr, counts, nlev, c->stream));
  else
    MIFC_HIP(c, hipMemsetAsync(counts, 0, sizeof(u64) * (size_t)nlev, c->stream));
  return 1;
}

enum ZeroCounts
{
  COUNTS_KEEP,
  COUNTS_ZERO_IF_TESTED,
  COUNTS_ZERO
};

// What a launch over P.nlev levels needs in place: which levels are ALL_DEFINED (fdefined per level, null: none is) in
// c->d_flags, and the counters zeroed.  Fills in P's flag and counter members.  A batch with a tested level needs its
// counter arrays (counts, and counts_ff when P.out_ff is wanted): without them the call is refused with `missing`.
// An untested batch needs no flags.
//   zero             COUNTS_KEEP: they accumulate; COUNTS_ZERO_IF_TESTED: a tested batch starts them from zero;
//                    COUNTS_ZERO: so does an untested one, whose counters then classify as ALL_DEFINED
//   null_when_none   the kernels read a null flag array as "no level is ALL_DEFINED": no upload when none is
// *scratch_read: the launch will read c->d_flags (an asynchronous caller has to scratch_release() behind it).
// Up to kPrepMaxLevels the flags travel bit-packed in the arguments of ONE small kernel that also zeroes the counters;
// very deep batches copy (through the pinned mirror) and fill.
int prepare_levels(mifc_ctx* c, mifc::StencilParams& P, const int* fdefined, u64* counts, u64* counts_ff, const char* missing, ZeroCounts zero_mode,
                   bool null_when_none, bool* scratch_read)
{
  const bool zero = zero_mode != COUNTS_KEEP;
  const int nlev = P.nlev;
  bool every_all = (fdefined != nullptr), any_all = false;
  for (int l = 0; l < nlev; ++l) {
    const bool a = level_all_defined(fdefined, l);
    every_all = every_all && a;
    any_all = any_all || a;
  }
  if (op_class(P.op) & OPC_ALWAYS_COUNTS)
    every_all = false;
  const bool upload = !every_all && (any_all || !null_when_none);
  P.every_level_all_defined = every_all ? 1 : 0;
  P.all_defined = (any_all || !null_when_none) ? c->d_flags : nullptr;
  P.n_undefined = counts;
  P.n_undefined_ff = counts_ff;
  *scratch_read = upload;
  if (every_all)
    return (zero_mode == COUNTS_ZERO && counts) ? zero_level_counts(c, counts, nlev) : 1;
  if (!counts || (P.out_ff && !counts_ff)) {
    c->err = missing;
    return 0;
  }
  if (nlev <= mifc::kPrepMaxLevels) {
    unsigned char hf[mifc::kPrepMaxLevels];
    for (int l = 0; upload && l < nlev; ++l)
      hf[l] = level_all_defined(fdefined, l) ? 1 : 0;
    MIFC_HIP(c, mifc::launch_prep_levels(upload ? hf : nullptr, nlev, c->d_flags, zero ? counts : nullptr, nlev, c->stream));
  } else {
    if (upload) {
      if (!pinned_acquire(c))
        return 0;
      for (int l = 0; l < nlev; ++l)
        pinned_flags(c)[l] = level_all_defined(fdefined, l) ? 1 : 0;
      MIFC_HIP(c, hipMemcpyAsync(c->d_flags, pinned_flags(c), (size_t)nlev, hipMemcpyHostToDevice, c->stream));
      if (!pinned_release(c))
        return 0;
    }
    if (zero)
      MIFC_HIP(c, hipMemsetAsync(counts, 0, sizeof(u64) * (size_t)nlev, c->stream));
  }
  if (zero && counts_ff)
    return zero_level_counts(c, counts_ff, nlev);
  return 1;
}

} // namespace

// ---- single-field / batched stencil driver ---------------------------------
int mifc_host::run_stencil(mifc_ctx* c, const StencilCall& sc, int* fdefined /* [nlev] */, float undef, int memkind)
{
  mifc::hostpipe_note_chunks(0, 0); // mifc_last_host_chunks: hostpipe_run() reports what it does
  if (sc.nx < 3 || sc.ny < 3 || sc.nlev < 1)
    return 0;
  const size_t n = (size_t)sc.nx * sc.ny;
  const size_t nb = n * (size_t)sc.nlev;
  Staging st(c, memkind);
  // A large level batch in host memory is streamed through the device in
  // chunks, copies in both directions overlapping the kernels (mifc_hostpipe.h);
  // everything else is staged whole.
  const bool piped = memkind == MIFC_MEM_HOST && !sc.f2 && sc.f0 && (sc.o0 || sc.o1) && mifc::hostpipe_chunk_levels(n, sc.nlev) > 0 && host_pipeline_enabled();
  StencilCall d = sc; // the request on device pointers
  d.in_level_stride = d.out_level_stride = (long)n;
  if (piped) {
    if (!c->pipe && !(c->pipe = mifc::hostpipe_create(c->device))) {
      c->err = "host pipeline: cannot create streams";
      return 0;
    }
    // the level fields stay placeholders (non-null where the operator has the field); the chunk launcher substitutes device buffers
  } else {
    d.f0 = st.in(sc.f0, nb);
    d.f1 = st.in(sc.f1, nb);
    d.o0 = st.out(sc.o0, nb);
    d.o1 = st.out(sc.o1, nb);
    d.f2 = st.in(sc.f2, nb);
  }
  d.xm = st.in(sc.xm, n);
  d.ym = st.in(sc.ym, n);
  d.fc = st.in(sc.fc, n);
  if (!st.ok() || !ensure_levels(c, (size_t)sc.nlev))
    return 0;
  mifc::StencilParams P = stencil_params(d, undef);
  if (!pinned_acquire(c)) // the counts come back through the pinned mirror
    return 0;
  // (a batch deeper than kPrepMaxLevels sends its flags through the mirror too and records a release behind that copy; the
  // mirror stays this call's all the same: nothing else uses it before st.finish() has synchronised)
  bool scratch_read;
  if (!prepare_levels(c, P, fdefined, c->d_counts, nullptr, "", COUNTS_ZERO_IF_TESTED, /*null_when_none*/ true, &scratch_read))
    return 0;
  const bool every_all = P.every_level_all_defined != 0;
  if (piped) {
    MIFC_HIP(c, hipStreamSynchronize(c->stream)); // maps, flags and zeroed counters are in place
    // P.out0 / P.out1 may have been swapped (only one of the two wanted)
    const float* h_in[2] = {sc.f0, sc.f1};
    float* h_out[2] = {P.out0, P.out1};
    const int n_in = sc.f1 ? 2 : 1;
    const mifc::StencilParams base = P;
    const mifc::ChunkLaunch launch = [&base](int l0, int nl, const float* const* d_in, float* const* d_out, hipStream_t stream) {
      mifc::StencilParams q = base;
      q.nlev = nl;
      q.f0 = d_in[0];
      q.f1 = base.f1 ? d_in[1] : nullptr;
      q.out0 = d_out[0];
      q.out1 = d_out[1];
      q.all_defined = base.all_defined ? base.all_defined + l0 : nullptr;
      q.n_undefined = base.n_undefined + l0;
      return mifc::launch_stencil(q, stream);
    };
    if (!mifc::hostpipe_run(c->pipe, n, sc.nlev, n_in, h_in, 2, h_out, launch, &c->err))
      return 0;
  } else {
    stencil_partials(c, P);
    MIFC_LAUNCH(c, mifc::launch_stencil(P, c->stream));
  }
  if (!every_all)
    MIFC_HIP(c, hipMemcpyAsync(pinned_counts(c), c->d_counts, sizeof(u64) * (size_t)sc.nlev, hipMemcpyDeviceToHost, c->stream));
  if (!st.finish()) // (the chunked pipeline has delivered its outputs itself: nothing was staged for them)
    return 0;
  const u64 denom = stencil_denominator(sc.op, sc.nx, sc.ny);
  for (int l = 0; l < sc.nlev; ++l) {
    if (sc.op == mifc::ST_GWIND_X)
      fdefined[l] = mifc_classify(denom, denom); // FieldCalculations.cc:664: every cell is counted
    else
      fdefined[l] = every_all ? MIFC_ALL_DEFINED : mifc_classify(pinned_counts(c)[l], denom);
  }
  return 1;
}

extern "C" {

// ---------------------------------------------------------------- stencils

int mifc_relvort(mifc_ctx* c, int nx, int ny, const float* u, const float* v, const float* xmapr, const float* ymapr, float* rvort, int* fdefined,
                 float undef, int memkind)
{
  CTX_OR_FAIL(c);
  const StencilCall sc = {mifc::ST_RELVORT, nx, ny, 1, u, v, xmapr, ymapr, nullptr, rvort, nullptr};
  return run_stencil(c, sc, fdefined, undef, memkind);
}

int mifc_absvort(mifc_ctx* c, int nx, int ny, const float* u, const float* v, const float* xmapr, const float* ymapr, const float* fcoriolis,
                 float* avort, int* fdefined, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  const StencilCall sc = {mifc::ST_ABSVORT, nx, ny, 1, u, v, xmapr, ymapr, fcoriolis, avort, nullptr};
  return run_stencil(c, sc, fdefined, undef, memkind);
}

int mifc_divergence(mifc_ctx* c, int nx, int ny, const float* u, const float* v, const float* xmapr, const float* ymapr, float* diverg,
                    int* fdefined, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  const StencilCall sc = {mifc::ST_DIVERGENCE, nx, ny, 1, u, v, xmapr, ymapr, nullptr, diverg, nullptr};
  return run_stencil(c, sc, fdefined, undef, memkind);
}

int mifc_gradient(mifc_ctx* c, int nx, int ny, const float* field, const float* xmapr, const float* ymapr, int compute, float* fgrad, int* fdefined,
                  float undef, int memkind)
{
  CTX_OR_FAIL(c);
  if (compute < 1 || compute > 4) // :2064 (size check comes first in the reference, both return false)
    return 0;
  const int op = mifc::ST_GRAD_X + (compute - 1);
  const StencilCall sc = {op, nx, ny, 1, field, nullptr, xmapr, ymapr, nullptr, fgrad, nullptr};
  return run_stencil(c, sc, fdefined, undef, memkind);
}

int mifc_plevelgwind_xcomp(mifc_ctx* c, int nx, int ny, const float* z, const float* xmapr, const float* ymapr, const float* fcoriolis, float* ug,
                           int* fdefined, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  (void)xmapr; // unused by the reference as well (:638)
  const StencilCall sc = {mifc::ST_GWIND_X, nx, ny, 1, z, nullptr, nullptr, ymapr, fcoriolis, ug, nullptr};
  return run_stencil(c, sc, fdefined, undef, memkind);
}

int mifc_plevelgwind_ycomp(mifc_ctx* c, int nx, int ny, const float* z, const float* xmapr, const float* ymapr, const float* fcoriolis, float* vg,
                           int* fdefined, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  (void)ymapr;
  // the reference lacks the nx<3||ny<3 guard here and would read out of bounds;
  // this implementation returns false instead
  const StencilCall sc = {mifc::ST_GWIND_Y, nx, ny, 1, z, nullptr, xmapr, nullptr, fcoriolis, vg, nullptr};
  return run_stencil(c, sc, fdefined, undef, memkind);
}

int mifc_plevelgvort(mifc_ctx* c, int nx, int ny, const float* z, const float* xmapr, const float* ymapr, const float* fcoriolis, float* gvort,
                     int* fdefined, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  const StencilCall sc = {mifc::ST_GVORT, nx, ny, 1, z, nullptr, xmapr, ymapr, fcoriolis, gvort, nullptr};
  return run_stencil(c, sc, fdefined, undef, memkind);
}

int mifc_ilevelgwind(mifc_ctx* c, int nx, int ny, const float* mpot, const float* xmapr, const float* ymapr, const float* fcoriolis, float* ug,
                     float* vg, int* fdefined, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  const StencilCall sc = {mifc::ST_IGWIND, nx, ny, 1, mpot, nullptr, xmapr, ymapr, fcoriolis, ug, vg};
  return run_stencil(c, sc, fdefined, undef, memkind);
}

// ------------------------------------------------ SURVEY.md 8f-1 operators

int mifc_advection(mifc_ctx* c, int nx, int ny, const float* f, const float* u, const float* v, const float* xmapr, const float* ymapr, float hours,
                   float* advec, int* fdefined, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  StencilCall sc = {mifc::ST_ADVECTION, nx, ny, 1, f, u, xmapr, ymapr, nullptr, advec, nullptr};
  sc.f2 = v;
  sc.scale = (float)(-3600. * (double)hours); // FieldCalculations.cc:1963
  return run_stencil(c, sc, fdefined, undef, memkind);
}

int mifc_jacobian(mifc_ctx* c, int nx, int ny, const float* field1, const float* field2, const float* xmapr, const float* ymapr, float* fjacobian,
                  int* fdefined, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  const StencilCall sc = {mifc::ST_JACOBIAN, nx, ny, 1, field1, field2, xmapr, ymapr, nullptr, fjacobian, nullptr};
  return run_stencil(c, sc, fdefined, undef, memkind);
}

// ----------------------------------------------------------------- batched

int mifc_vortdiv_levels(mifc_ctx* c, int nx, int ny, int nlev, const float* u, const float* v, const float* xmapr, const float* ymapr, float* rvort,
                        float* diverg, int* fdefined, float undef, int memkind)
{
  if (!c || (!rvort && !diverg))
    return 0;
  enter(c);
  const StencilCall sc = {mifc::ST_VORTDIV, nx, ny, nlev, u, v, xmapr, ymapr, nullptr, rvort, diverg};
  return run_stencil(c, sc, fdefined, undef, memkind);
}

int mifc_stencil_levels(mifc_ctx* c, int op, int nx, int ny, int nlev, const float* f0, const float* f1, const float* xmapr, const float* ymapr,
                        const float* fcoriolis, float* out0, float* out1, int* fdefined, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  if (!is_level_batch_op(op) || !f0 || !out0)
    return 0;
  const unsigned k = op_class(op);
  if ((k & OPC_TAKES_F1) && !f1)
    return 0;
  const StencilCall sc = {op, nx, ny, nlev, f0, (k & OPC_TAKES_F1) ? f1 : nullptr, xmapr, ymapr, fcoriolis, out0, (k & OPC_TWO_OUTPUTS) ? out1 : nullptr};
  return run_stencil(c, sc, fdefined, undef, memkind);
}

// mifc_stencil_levels plus the rest of the stencil family over a batch of levels (shared map factors): advection runs on the
// batched stencil driver here; thermalFrontParameter, plevelqvector and shapiro2_filter have their drivers in
// mifc_capi_twostage.hip
int mifc_stencil_levels_ex(mifc_ctx* c, int op, int nx, int ny, int nlev, const float* f0, const float* f1, const float* f2, const float* xmapr,
                           const float* ymapr, const float* fcoriolis, const float* level_scalars, float scalar, int compute, float* out0,
                           float* out1, int* fdefined, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  mifc::hostpipe_note_chunks(0, 0); // (the two-stage operators and the filter stage their batch whole and may not reach run_stencil())
  if (op != MIFC_OP_ADVECTION && op != MIFC_OP_TFP && op != MIFC_OP_QVECTOR && op != MIFC_OP_SHAPIRO2)
    return mifc_stencil_levels(c, op, nx, ny, nlev, f0, f1, xmapr, ymapr, fcoriolis, out0, out1, fdefined, undef, memkind);
  if (nx < 3 || ny < 3 || nlev < 1 || !f0 || !out0 || !fdefined)
    return 0;
  if (op == MIFC_OP_ADVECTION) { // FieldCalculations.cc:1942-1983: f0 = f, f1 = u, f2 = v, scalar = hours
    if (!f1 || !f2)
      return 0;
    StencilCall sc = {mifc::ST_ADVECTION, nx, ny, nlev, f0, f1, xmapr, ymapr, nullptr, out0, nullptr};
    sc.f2 = f2;
    sc.scale = (float)(-3600. * (double)scalar); // :1963
    return run_stencil(c, sc, fdefined, undef, memkind);
  }
  return two_stage_levels_ex(c, op, nx, ny, nlev, f0, f1, xmapr, ymapr, fcoriolis, level_scalars, compute, out0, fdefined, undef, memkind);
}

int mifc_vortdiv_levels_enqueue(mifc_ctx* c, int nx, int ny, int nlev, const float* u, const float* v, const float* xmapr, const float* ymapr,
                                float* rvort, float* diverg, const int* fdefined_in, float undef, unsigned long long* n_undefined_dev)
{
  const size_t n = (size_t)(nx > 0 ? nx : 0) * (size_t)(ny > 0 ? ny : 0);
  return mifc_vortdiv_levels_strided_enqueue(c, nx, ny, nlev, u, v, xmapr, ymapr, rvort, diverg, n, n, fdefined_in, undef, n_undefined_dev);
}

int mifc_vortdiv_ff_levels_enqueue(mifc_ctx* c, int nx, int ny, int nlev, const float* u, const float* v, const float* xmapr, const float* ymapr,
                                   float* rvort, float* diverg, float* ff, const int* fdefined_in, float undef, unsigned long long* n_undefined_dev,
                                   unsigned long long* n_undefined_ff_dev)
{
  if (!c || !rvort || !diverg || !ff || !u || !v || !xmapr || !ymapr)
    return 0;
  enter(c);
  if (nx < 3 || ny < 3 || nlev < 1)
    return 0;
  if (!ensure_levels(c, (size_t)nlev))
    return 0;
  StencilCall sc = {mifc::ST_VORTDIV, nx, ny, nlev, u, v, xmapr, ymapr, nullptr, rvort, diverg};
  sc.in_level_stride = sc.out_level_stride = (long)nx * ny;
  sc.out_ff = ff;
  mifc::StencilParams P = stencil_params(sc, undef);
  // this entry's own ways, kept: both counter arrays are zeroed whatever mifc_counts_accumulate says, and the kernels are
  // handed c->d_flags even when no level is ALL_DEFINED
  bool scratch_read;
  if (!prepare_levels(c, P, fdefined_in, n_undefined_dev, n_undefined_ff_dev,
                      "mifc_vortdiv_ff_levels_enqueue: both counter arrays are required unless every level is ALL_DEFINED", COUNTS_ZERO_IF_TESTED,
                      /*null_when_none*/ false, &scratch_read))
    return 0;
  const bool every_all = P.every_level_all_defined != 0;
  const bool timed = c->timing && c->n_timed < mifc_ctx::NTIMED;
  if (timed)
    (void)hipEventRecord(c->tev[2 * c->n_timed], c->stream);
  hipError_t e = mifc::launch_stencil(P, c->stream);
  if (e == hipErrorNotSupported) {
    // not a launch the three-output kernel takes (shallow or small batch, ragged width, NaN undef, a forced tuning): the
    // pair as usual and the wind speed as a launch of its own (the batched vectorabs of mifc_derived.hip)
    (void)hipGetLastError();
    P.out_ff = nullptr;
    P.n_undefined_ff = nullptr;
    e = mifc::launch_stencil(P, c->stream);
    if (e == hipSuccess && (nx * ny) % 4 != 0) {
      // a cell count the batched vectorabs does not take: level by level on the single-field kernel
      for (int l = 0; l < nlev && e == hipSuccess; ++l) {
        const bool all = level_all_defined(fdefined_in, l);
        const int fl = all ? MIFC_ALL_DEFINED : MIFC_SOME_DEFINED;
        mifc::EwiseParams E = ewise_base(mifc::EW_VECTORABS, nx, ny, &fl, undef);
        E.in0 = u + (size_t)l * nx * ny;
        E.in1 = v + (size_t)l * nx * ny;
        E.out = ff + (size_t)l * nx * ny;
        E.count = all ? 0 : 1;
        E.n_undefined = all ? nullptr : n_undefined_ff_dev + l;
        e = mifc::launch_ewise(E, c->stream);
      }
    } else if (e == hipSuccess) {
      mifc::DerivedParams D;
      std::memset(&D, 0, sizeof D);
      D.n = nx * ny;
      D.nlev = nlev;
      D.u = u;
      D.v = v;
      D.ff = ff;
      D.wind_all_defined = c->d_flags;
      D.thermo_all_defined = c->d_flags;
      D.every_level_all_defined = every_all ? 1 : 0;
      D.undef = undef;
      D.cnt_ff = n_undefined_ff_dev;
      e = mifc::launch_derived_levels(D, c->stream);
    }
  }
  if (timed) {
    (void)hipEventRecord(c->tev[2 * c->n_timed + 1], c->stream);
    c->n_timed += 1;
  }
  if (e != hipSuccess) {
    fail(c, "mifc_vortdiv_ff_levels_enqueue: launch", e);
    return 0;
  }
  if (scratch_read && !scratch_release(c)) // the kernels read c->d_flags
    return 0;
  return 1;
}

const char* mifc_last_stencil_form(void)
{
  return mifc::last_form();
}

int mifc_last_host_chunks(int* levels_per_chunk)
{
  return mifc::hostpipe_last_chunks(levels_per_chunk);
}

int mifc_host_chunk_levels(size_t n, int nlev)
{
  return mifc::hostpipe_chunk_levels(n, nlev);
}

unsigned long long mifc_stencil_count_domain(int op, int nx, int ny)
{
  return stencil_denominator(op, nx, ny);
}

// what the asynchronous level-batch entries share: flags up, counters zeroed, one launch, nothing read back
static int stencil_enqueue(mifc_ctx* c, const char* missing, const StencilCall& sc, float undef, const int* fdefined_in, u64* n_undefined_dev)
{
  if (!ensure_levels(c, (size_t)sc.nlev))
    return 0;
  mifc::StencilParams P = stencil_params(sc, undef);
  bool scratch_read;
  if (!prepare_levels(c, P, fdefined_in, n_undefined_dev, nullptr, missing, c->counts_accumulate ? COUNTS_KEEP : COUNTS_ZERO, /*null_when_none*/ true,
                      &scratch_read))
    return 0;
  stencil_partials(c, P);
  MIFC_LAUNCH(c, mifc::launch_stencil(P, c->stream));
  if ((scratch_read || P.partials) && !scratch_release(c)) // the kernels read c->d_flags / write and read c->d_partials
    return 0;
  return 1;
}

int mifc_vortdiv_levels_strided_enqueue(mifc_ctx* c, int nx, int ny, int nlev, const float* u, const float* v, const float* xmapr, const float* ymapr,
                                        float* rvort, float* diverg, size_t in_level_stride, size_t out_level_stride, const int* fdefined_in,
                                        float undef, unsigned long long* n_undefined_dev)
{
  if (!c || (!rvort && !diverg))
    return 0;
  enter(c);
  if (nx < 3 || ny < 3 || nlev < 1)
    return 0;
  if (in_level_stride < (size_t)nx * ny || out_level_stride < (size_t)nx * ny) {
    c->err = "mifc_vortdiv_levels_strided_enqueue: a level stride is smaller than one field";
    return 0;
  }
  StencilCall sc = {mifc::ST_VORTDIV, nx, ny, nlev, u, v, xmapr, ymapr, nullptr, rvort, diverg};
  sc.in_level_stride = (long)in_level_stride;
  sc.out_level_stride = (long)out_level_stride;
  return stencil_enqueue(c, "mifc_vortdiv_levels_enqueue: n_undefined_dev is required unless every level is ALL_DEFINED", sc, undef, fdefined_in,
                         n_undefined_dev);
}

int mifc_stencil_levels_enqueue(mifc_ctx* c, int op, int nx, int ny, int nlev, const float* f0, const float* f1, const float* xmapr, const float* ymapr,
                                const float* fcoriolis, float* out0, float* out1, const int* fdefined_in, float undef,
                                unsigned long long* n_undefined_dev)
{
  CTX_OR_FAIL(c);
  if (!is_level_batch_op(op) || !f0 || nx < 3 || ny < 3 || nlev < 1 || !xmapr || !ymapr)
    return 0;
  const unsigned k = op_class(op);
  if (((k & OPC_TAKES_F1) && !f1) || ((k & OPC_NEEDS_FC) && !fcoriolis) || (op == mifc::ST_IGWIND && !out1))
    return 0;
  if (op == mifc::ST_VORTDIV ? (!out0 && !out1) : !out0)
    return 0;
  StencilCall sc = {op, nx, ny, nlev, f0, (k & OPC_TAKES_F1) ? f1 : nullptr, xmapr, ymapr, (k & OPC_NEEDS_FC) ? fcoriolis : nullptr, out0,
                    (k & OPC_TWO_OUTPUTS) ? out1 : nullptr};
  sc.in_level_stride = sc.out_level_stride = (long)nx * ny;
  return stencil_enqueue(c, "mifc_stencil_levels_enqueue: n_undefined_dev is required unless every level is ALL_DEFINED", sc, undef, fdefined_in,
                         n_undefined_dev);
}

int mifc_vortdiv_slab_enqueue(mifc_ctx* c, int nx, int ny_global, int j0, int ny_local, const float* u_halo, const float* v_halo, const float* xmapr,
                              const float* ymapr, float* rvort, float* diverg, int fdefined_in, float undef, unsigned long long* n_undefined_dev)
{
  return mifc_vortdiv_slab_rows_enqueue(c, nx, ny_global, j0, ny_local, 0, ny_local, u_halo, v_halo, xmapr, ymapr, rvort, diverg, fdefined_in, undef,
                                        n_undefined_dev, 0);
}

int mifc_vortdiv_slab_rows_enqueue(mifc_ctx* c, int nx, int ny_global, int j0, int ny_local, int row_begin, int row_end, const float* u_halo,
                                   const float* v_halo, const float* xmapr, const float* ymapr, float* rvort, float* diverg, int fdefined_in,
                                   float undef, unsigned long long* n_undefined_dev, int accumulate_count)
{
  if (!c || (!rvort && !diverg))
    return 0;
  enter(c);
  if (nx < 3 || ny_global < 3 || ny_local < 1 || j0 < 0 || j0 + ny_local > ny_global)
    return 0;
  // a slab that owns a global edge row must also own the row it is filled from
  if ((j0 == 0 || j0 + ny_local == ny_global) && ny_local < 2)
    return 0;
  if (row_begin < 0 || row_end > ny_local || row_begin >= row_end)
    return 0;
  // ... and a row range must keep the two together (fillEdges copies row 1 to row 0, row ny-2 to row ny-1)
  if ((j0 == 0 && (row_begin == 1 || row_end == 1)) || (j0 + ny_local == ny_global && (row_begin == ny_local - 1 || row_end == ny_local - 1))) {
    c->err = "mifc_vortdiv_slab_rows_enqueue: a row range must not separate a global edge row from the row it is filled from";
    return 0;
  }
  // owned row 0; halo rows sit directly before and after
  StencilCall sc = {mifc::ST_VORTDIV, nx, ny_global, 1, u_halo + nx, v_halo + nx, xmapr, ymapr, nullptr, rvort, diverg};
  sc.j0 = j0;
  sc.ny_local = ny_local;
  if (row_begin != 0 || row_end != ny_local) {
    sc.row_begin = row_begin;
    sc.row_end = row_end;
  }
  mifc::StencilParams P = stencil_params(sc, undef);
  P.every_level_all_defined = (fdefined_in == MIFC_ALL_DEFINED) ? 1 : 0;
  P.all_defined = nullptr;
  P.n_undefined = n_undefined_dev;
  if (!P.every_level_all_defined && !n_undefined_dev) {
    c->err = "mifc_vortdiv_slab_enqueue: n_undefined_dev is required unless the input is ALL_DEFINED";
    return 0;
  }
  if (n_undefined_dev && !accumulate_count)
    MIFC_HIP(c, hipMemsetAsync(n_undefined_dev, 0, sizeof(u64), c->stream));
  MIFC_LAUNCH(c, mifc::launch_stencil(P, c->stream));
  return 1;
}

} // extern "C"
