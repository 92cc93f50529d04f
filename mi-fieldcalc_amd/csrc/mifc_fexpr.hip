// mifc_fexpr.hip -- field expressions over level batches (mifc_fexpr_levels, include/mifc.h rules 1-5; EXTENSION: the
// reference's callers compose field algebra one single-field call per operation).
//
// An interpreter: the program is data, so one kernel serves every expression.  What keeps it near the speed of a
// hand-written kernel:
//   * the register file of a cell is ONE 16-wide vector value, indexed with wave-uniform indices: it stays in VGPRs
//     (index mode / movrel), where an array of arrays went to scratch;
//   * the instruction words and the constants are kernel arguments and the level scalars a constant table: scalar loads,
//     the decoded fields passed through readfirstlane so that no access gets a waterfall loop;
//   * the opcode switch is wave-uniform: a wave executes one case per instruction, for its V cells;
//   * every operation computes unconditionally and selects undef behind it (mifc_device.h, pick()): two tests per operand
//     and one select per cell and operation, no exec-mask regions.
// A lane owns V consecutive cells of one level (blockIdx.y): four through 16-byte accesses (at dword alignment where a
// level size is no multiple of four: that costs loads nothing), or one.  All loads of the cell are issued before the
// tables are staged and the first instruction runs; the stores are nontemporal.  Undefined cells are counted per output
// and level, one atomic per workgroup and counter and only where the count is not zero.
#include "mifc_column_walk.h"
#include "mifc_device.h"
#include "mifc_kernels.h"

#include "../../include/mifc.h"

namespace mifc {

namespace {

typedef float fexpr_regs __attribute__((ext_vector_type(16)));
typedef float fexpr_quad __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ unsigned int uniform(unsigned int x)
{
  return (unsigned int)__builtin_amdgcn_readfirstlane((int)x);
}

template <int V, bool TABLES>
__global__ __launch_bounds__(256) void fexpr_kernel(const FexprParams P)
{
  __shared__ double s_pow[TABLES ? (2 * MIFC_POW_LOG_N + MIFC_POW_EXP_N) : 1];
  PowTables PT = {s_pow, s_pow, s_pow, s_pow};

  const float undef = P.undef;
  const int k = P.lev0 + (int)blockIdx.y; // wave-uniform
  const long at = ((long)blockIdx.x * 256 + threadIdx.x) * V;
  const bool mine = at < (long)P.n;                  // (the vector launch covers whole quads only)
  const long cell = P.cell0 + (mine ? at : 0);       // a lane outside reads the first cells and throws them away
  const long level = (long)k * P.stride;

  // the inputs as plain values first (an unset register is 0: the program check lets nobody read it), the register files
  // built from them in one piece: inserting under the tests makes the compiler carry a copy of the file per input
  float x0[FEXPR_MAX_IN][V];
  const int nin = P.nfields + P.nplanes;
#pragma unroll
  for (int i = 0; i < FEXPR_MAX_IN; ++i) {
#pragma unroll
    for (int c = 0; c < V; ++c)
      x0[i][c] = 0.f;
    if (i < nin) { // wave-uniform
      const float* p = P.in[i] + (i < P.nfields ? level : 0L) + cell;
      if constexpr (V == 4) {
        const fexpr_quad q = *reinterpret_cast<const fexpr_quad*>(p);
        x0[i][0] = q.x;
        x0[i][1] = q.y;
        x0[i][2] = q.z;
        x0[i][3] = q.w;
      } else {
        x0[i][0] = p[0];
      }
    }
  }
  fexpr_regs r[V];
#pragma unroll
  for (int c = 0; c < V; ++c)
    r[c] = (fexpr_regs){x0[0][c], x0[1][c], x0[2][c], x0[3][c], x0[4][c], x0[5][c], x0[6][c], x0[7][c], x0[8][c], x0[9][c], x0[10][c], x0[11][c],
                        0.f,      0.f,      0.f,      0.f};
  if constexpr (TABLES)
    PT = pow_tables_init(s_pow);

  const ConstFloats scalars = (ConstFloats)(unsigned long long)P.level_scalars;
  // a source byte: a register of the cell, or a wave-uniform number
  auto fetch = [&](unsigned int s, float(&x)[V]) {
    if (s < 16u) {
#pragma unroll
      for (int c = 0; c < V; ++c)
        x[c] = r[c][s];
    } else {
      const float u = s < 32u ? scalars[(long)(s - 16u) * P.nlev_all + k] : P.consts[s - 32u];
#pragma unroll
      for (int c = 0; c < V; ++c)
        x[c] = u;
    }
  };

  for (int i = 0; i < P.ncode; ++i) {
    const unsigned int w0 = uniform(P.code[2 * i]), w1 = uniform(P.code[2 * i + 1]);
    const unsigned int op = w0 & 255u, dst = (w0 >> 8) & 255u;
    float a[V], b[V], res[V];
    bool ok[V];
    fetch((w0 >> 16) & 255u, a);
    fetch(w0 >> 24, b); // (the program check made b = a where the operation has one operand)
#pragma unroll
    for (int c = 0; c < V; ++c)
      ok[c] = all_def(undef, a[c], b[c]);
    switch (op) {
    case MIFC_FEXPR_ADD:
#pragma unroll
      for (int c = 0; c < V; ++c)
        res[c] = a[c] + b[c];
      break;
    case MIFC_FEXPR_SUB:
#pragma unroll
      for (int c = 0; c < V; ++c)
        res[c] = a[c] - b[c];
      break;
    case MIFC_FEXPR_MUL:
#pragma unroll
      for (int c = 0; c < V; ++c)
        res[c] = a[c] * b[c];
      break;
    case MIFC_FEXPR_DIV: // divideUndef, FieldCalculations.cc:84
#pragma unroll
      for (int c = 0; c < V; ++c) {
        res[c] = a[c] / b[c];
        ok[c] = ok[c] & (b[c] != 0.f);
      }
      break;
    case MIFC_FEXPR_MIN: // :2504
#pragma unroll
      for (int c = 0; c < V; ++c)
        res[c] = (b[c] < a[c]) ? b[c] : a[c];
      break;
    case MIFC_FEXPR_MAX: // :2519
#pragma unroll
      for (int c = 0; c < V; ++c)
        res[c] = (a[c] < b[c]) ? b[c] : a[c];
      break;
    case MIFC_FEXPR_ABS:
#pragma unroll
      for (int c = 0; c < V; ++c)
        res[c] = fabsf(a[c]);
      break;
    case MIFC_FEXPR_NEG:
#pragma unroll
      for (int c = 0; c < V; ++c)
        res[c] = -a[c];
      break;
    case MIFC_FEXPR_SQRT:
#pragma unroll
      for (int c = 0; c < V; ++c)
        res[c] = sqrtf(a[c]);
      break;
    case MIFC_FEXPR_LOG:
    case MIFC_FEXPR_LOG10:
      if constexpr (TABLES) {
        const bool base10 = op == MIFC_FEXPR_LOG10;
#pragma unroll
        for (int c = 0; c < V; ++c)
          res[c] = log_float(PT, a[c], base10);
      }
      break;
    case MIFC_FEXPR_EXP:
    case MIFC_FEXPR_POW10:
      if constexpr (TABLES) {
        const bool base10 = op == MIFC_FEXPR_POW10;
#pragma unroll
        for (int c = 0; c < V; ++c)
          res[c] = exp_float(PT, (double)a[c], base10);
      }
      break;
    case MIFC_FEXPR_POW:
      if constexpr (TABLES) {
#pragma unroll
        for (int c = 0; c < V; ++c)
          res[c] = pow_float(PT, a[c], (double)b[c]);
      }
      break;
    case MIFC_FEXPR_LT:
#pragma unroll
      for (int c = 0; c < V; ++c)
        res[c] = a[c] < b[c] ? 1.f : 0.f;
      break;
    case MIFC_FEXPR_LE:
#pragma unroll
      for (int c = 0; c < V; ++c)
        res[c] = a[c] <= b[c] ? 1.f : 0.f;
      break;
    case MIFC_FEXPR_EQ:
#pragma unroll
      for (int c = 0; c < V; ++c)
        res[c] = a[c] == b[c] ? 1.f : 0.f;
      break;
    case MIFC_FEXPR_NE:
#pragma unroll
      for (int c = 0; c < V; ++c)
        res[c] = a[c] != b[c] ? 1.f : 0.f;
      break;
    case MIFC_FEXPR_SELECT: {
      float s[V];
      fetch(w1 & 255u, s);
#pragma unroll
      for (int c = 0; c < V; ++c) {
        res[c] = s[c] != 0.f ? a[c] : b[c];
        ok[c] = all_def(undef, s[c], res[c]); // the condition and the chosen operand only
      }
      break;
    }
    case MIFC_FEXPR_IFDEF:
#pragma unroll
      for (int c = 0; c < V; ++c) {
        res[c] = is_def(a[c], undef) ? a[c] : b[c];
        ok[c] = true;
      }
      break;
    case MIFC_FEXPR_MASK: {
      float s[V];
      fetch(w1 & 255u, s);
#pragma unroll
      for (int c = 0; c < V; ++c) {
        res[c] = a[c];
        ok[c] = is_def(s[c], undef) & (s[c] != 0.f);
      }
      break;
    }
    default: // MIFC_FEXPR_MOV
#pragma unroll
      for (int c = 0; c < V; ++c)
        res[c] = a[c];
      break;
    }
#pragma unroll
    for (int c = 0; c < V; ++c)
      r[c][dst] = pick(ok[c], res[c], undef);
  }

  unsigned int bad[FEXPR_MAX_OUT] = {0, 0, 0, 0};
  u64* counter[FEXPR_MAX_OUT];
#pragma unroll
  for (int o = 0; o < FEXPR_MAX_OUT; ++o) {
    counter[o] = o < P.nout ? P.n_undefined + (long)o * P.nlev_all + k : nullptr;
    if (o < P.nout) { // wave-uniform
      const unsigned int reg = uniform((P.out_regs >> (8 * o)) & 255u);
      float x[V];
#pragma unroll
      for (int c = 0; c < V; ++c) {
        x[c] = r[c][reg];
        bad[o] += (mine && x[c] == undef) ? 1u : 0u;
      }
      if (mine) {
        float* p = P.out[o] + level + cell;
        if constexpr (V == 4) {
          fexpr_quad q;
          q.x = x[0];
          q.y = x[1];
          q.z = x[2];
          q.w = x[3];
          __builtin_nontemporal_store(q, reinterpret_cast<fexpr_quad*>(p));
        } else {
          __builtin_nontemporal_store(x[0], p);
        }
      }
    }
  }
  block_count_add<FEXPR_MAX_OUT>(counter, bad);
}

bool on_grid16(const void* p)
{
  return (reinterpret_cast<size_t>(p) & 15u) == 0;
}

template <int V>
void launch_tables(const FexprParams& P, int tables, dim3 grid, int block, hipStream_t stream)
{
  if (tables)
    hipLaunchKernelGGL((fexpr_kernel<V, true>), grid, dim3(block), 0, stream, P);
  else
    hipLaunchKernelGGL((fexpr_kernel<V, false>), grid, dim3(block), 0, stream, P);
}

} // namespace

FexprShape fexpr_shape(const FexprParams& P)
{
  bool vec = P.n >= 4;
  for (int i = 0; i < P.nfields + P.nplanes; ++i)
    vec = vec && on_grid16(P.in[i]);
  for (int o = 0; o < P.nout; ++o)
    vec = vec && on_grid16(P.out[o]);
  if (vec)
    return {1, (int)((((long)P.n >> 2) + 255) / 256), P.n & 3};
  return {0, (int)(((long)P.n + 255) / 256), 0};
}

hipError_t launch_fexpr(const FexprParams& prm, int nlev, int tables, hipStream_t stream)
{
  if (prm.n < 1 || nlev < 1 || prm.ncode < 1 || prm.ncode > FEXPR_MAX_CODE || prm.nout < 1 || prm.nout > FEXPR_MAX_OUT || prm.nfields < 0 ||
      prm.nplanes < 0 || prm.nfields + prm.nplanes < 1 || prm.nfields + prm.nplanes > FEXPR_MAX_IN)
    return hipErrorInvalidValue;
  const FexprShape shape = fexpr_shape(prm);
  const int max_grid_y = 65535;
  for (int lev0 = 0; lev0 < nlev; lev0 += max_grid_y) {
    const unsigned int levels = (unsigned int)(nlev - lev0 < max_grid_y ? nlev - lev0 : max_grid_y);
    FexprParams P = prm;
    P.lev0 = lev0;
    P.cell0 = 0;
    if (shape.vector) {
      P.n = prm.n & ~3;
      launch_tables<4>(P, tables, dim3((unsigned int)shape.grid, levels), 256, stream);
      if (shape.tail > 0) {
        P.cell0 = prm.n & ~3;
        P.n = shape.tail;
        launch_tables<1>(P, tables, dim3(1, levels), 64, stream);
      }
    } else {
      launch_tables<1>(P, tables, dim3((unsigned int)shape.grid, levels), 256, stream);
    }
  }
  return hipGetLastError();
}

} // namespace mifc
