// mifc_vcumul.hip -- running vertical integrals of level batches (mifc_vcumul_hlevels / mifc_vcumul_fields /
// mifc_vcumul_levels, include/mifc.h; EXTENSION: the reference has no function that crosses levels).
//
// The walk is the one of mifc_vderiv.hip: consecutive lanes own consecutive cells, four each through 16-byte loads
// (V = 4) or one each (V = 1), a lane keeps its cells for all levels, three level slots rotate (the loop unrolled three
// times so that the slots are static), the per-level scalars come from a small table through the constant address space.
// What differs: this kernel carries state from level to level, and in a direction the call chooses.  Position j of the
// walk is level first + j * step with step = +1 or -1: the planes are addressed with that level number, so the walk from
// the last level is the same code with a negative distance between planes.  Per field and cell the lane carries the sum S
// in double, beside them the previous level's values (float) and g(c) of the previous level (double) per cell; g is the
// coordinate itself or its logarithm -- one double log per cell and level however many fields the launch has.  Which
// (field, cell) has met a hole is one word per cell (bit f = nothing in the way so far): bits only ever go out, a cell
// whose bit is out is written as undef and counted at every later level.  Position 0 is peeled out of the loop: the sum
// starts there (+0, or x * (g(c) - g(start)) where a start coordinate is given) instead of growing.  Undefined cells are
// counted per level and field by ballot into LDS and leave the workgroup as one atomic per counter that is not zero
// (DESIGN.md 4.8, 4.17a).
#include "mifc_column_walk.h"
#include "mifc_device.h"
#include "mifc_kernels.h"

#include <type_traits>

namespace mifc {

namespace {

template <int KIND, bool LOG, int NF, int V>
__global__ __launch_bounds__(256, 2) void vcumul_kernel(const VcumulParams P)
{
  constexpr int R = 3;                       // level slots
  constexpr unsigned int EVERY = (1u << NF) - 1u;
  extern __shared__ unsigned int s_cnt[]; // [NF][nlev]
  const int nlev = P.nlev, f0 = P.f0;
  const bool lds = P.lds_counts != 0;
  if (lds) {
    for (int j = threadIdx.x; j < NF * nlev; j += 256)
      s_cnt[j] = 0;
    __syncthreads();
  }

  const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * V;
  const long left = (long)P.n - i0;
  const int n_cells = left < 0 ? 0 : (left < V ? (int)left : V); // this lane's cells inside the launch: cells 0 .. n_cells - 1
  // a wave-uniform base plus the lane's 32-bit byte offset inside the workgroup; lanes past the end walk the workgroup's
  // first column group and neither store nor count (mifc_vlayer.hip)
  const long block0 = (long)blockIdx.x * (256 * V);
  const unsigned int lane_bytes = n_cells > 0 ? threadIdx.x * (unsigned int)(V * sizeof(float)) : 0u;
  auto lane_of = [&](const float* uniform_base) { return reinterpret_cast<const float*>(reinterpret_cast<const char*>(uniform_base) + lane_bytes); };
  const float undef = P.undef;
  const ConstFloats ab = (ConstFloats)(unsigned long long)P.ab;
  const ConstWords lev_bits = (ConstWords)(unsigned long long)P.lev_bits;
  const ConstDoubles lev_g = (ConstDoubles)(unsigned long long)P.lev_g;
  typedef WalkLevel<NF, V> Level;

  // rule 2: position j of the walk is this level
  const int first = P.from != 0 ? nlev - 1 : 0, step = P.from != 0 ? -1 : 1;
  auto level_of = [&](int j) { return first + j * step; };

  auto load = [&](Level& L, int j) {
    const long off = (long)walk_here(level_of(j)) * P.in_stride + block0; // (opaque: no induction variable per pointer)
    if constexpr (KIND == VDERIV_FIELD)
      walk_load<V>(L.c, lane_of(P.coord + off));
#pragma unroll
    for (int f = 0; f < NF; ++f)
      walk_load<V>(L.x[f], lane_of(P.fields[f] + off));
  };

  auto g_of = [&](float c) -> double {
    if constexpr (LOG)
      return log((double)c);
    else
      return (double)c;
  };
  // rule 1: not NaN (an undefined coordinate is carried as NaN), positive where its logarithm is taken
  auto usable = [&](float c) -> bool {
    if constexpr (LOG)
      return c > 0.f;
    else
      return c == c;
  };

  const float nan = __int_as_float(0x7fc00000);
  float ps[V];
  if constexpr (KIND == VDERIV_HYBRID) {
    walk_load<V>(ps, lane_of(P.coord + block0));
#pragma unroll
    for (int c = 0; c < V; ++c)
      ps[c] = (P.ps_all != 0 || ps[c] != undef) ? ps[c] : nan;
  }

  // what is carried: bit f of alive[c] = nothing has been in the way of field f in cell c so far (rules 4 and 6)
  unsigned int alive[V];
  double gs[V]; // g(start)
  const bool has_start = P.start != nullptr;
#pragma unroll
  for (int c = 0; c < V; ++c) {
    alive[c] = EVERY;
    gs[c] = 0.0;
  }
  if (has_start) {
    float s[V];
    walk_load<V>(s, lane_of(P.start + block0));
#pragma unroll
    for (int c = 0; c < V; ++c) {
      const bool ok = (P.start_all != 0 || s[c] != undef) && usable(s[c]);
      gs[c] = g_of(s[c]);
      alive[c] = ok ? EVERY : 0u;
    }
  }
  float bs[NF][V];
#pragma unroll
  for (int f = 0; f < NF; ++f) {
#pragma unroll
    for (int c = 0; c < V; ++c)
      bs[f][c] = 0.f;
    if (P.base[f] != nullptr) {
      walk_load<V>(bs[f], lane_of(P.base[f] + block0));
#pragma unroll
      for (int c = 0; c < V; ++c) {
        const bool ok = (((P.base_all >> f) & 1) != 0 || bs[f][c] != undef) && bs[f][c] == bs[f][c];
        alive[c] &= ok ? EVERY : ~(1u << f);
      }
    }
  }

  double S[NF][V], gp[V];
  float xp[NF][V];

  auto count = [&](int f, int k, unsigned int n) {
    // (the lane test and the row of the counter computed here, not kept in SGPRs through the walk)
    if (n != 0 && (walk_here_v(threadIdx.x) & 63) == 0) {
      const int row = walk_here(nlev), field0 = walk_here(f0);
      if (lds)
        atomicAdd(&s_cnt[f * row + k], n);
      else
        atomicAdd(P.n_undefined + (long)(field0 + f) * row + k, (u64)n);
    }
  };

  // one position of the walk: FIRST = position 0, where the sums start
  auto advance = [&](auto first_tag, const Level& L, int j) {
    constexpr bool FIRST = decltype(first_tag)::value;
    const int k = level_of(j);
    const unsigned int bits = lev_bits[k];
    double g[V];
#pragma unroll
    for (int c = 0; c < V; ++c) {
      bool ok = true;
      if constexpr (KIND == VDERIV_LEVELS) {
        g[c] = lev_g[k]; // the call refuses a level that is not usable
      } else {
        float cc;
        if constexpr (KIND == VDERIV_HYBRID) {
          const float prod = ab[nlev + k] * ps[c]; // p_hlevel, FieldCalculations.cc:303: the product rounded, then the sum
          cc = ab[k] + prod;
        } else {
          cc = (((bits >> VINTERP_COORD_BIT) & 1u) != 0 || L.c[c] != undef) ? L.c[c] : nan;
        }
        ok = usable(cc);
        g[c] = g_of(cc);
      }
      // rule 3: bit f = x_f passes is_defined
      const unsigned int all = bits >> f0;
      unsigned int w = 0;
#pragma unroll
      for (int f = 0; f < NF; ++f)
        w |= (((all >> f) & 1u) != 0 || is_def(L.x[f][c], undef)) ? 1u << f : 0u;
      alive[c] &= ok ? w : 0u;
    }

    float res[NF][V];
#pragma unroll
    for (int c = 0; c < V; ++c) {
      const double dg = g[c] - (FIRST ? gs[c] : gp[c]);
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const double x = (double)L.x[f][c];
        if constexpr (FIRST) {
          const double held = x * dg; // rule 4: the integrand held constant between the start and the first level
          S[f][c] = has_start ? held : 0.0;
        } else {
          const double sum = (double)xp[f][c] + x; // rule 5
          const double half = sum * 0.5;
          const double term = half * dg;
          S[f][c] = S[f][c] + term;
        }
        const double scaled = P.scale[f] * S[f][c]; // rule 7
        const double based = (double)bs[f][c] + scaled;
        res[f][c] = (float)(P.base[f] != nullptr ? based : scaled);
        xp[f][c] = L.x[f][c];
      }
      gp[c] = g[c];
    }

    const long at = (long)walk_here(k) * P.out_stride + i0;
    const int n_mine = (int)walk_here_v((unsigned int)n_cells); // (compared here: no lane masks that live through the walk)
    bool whole = true;
#pragma unroll
    for (int c = 0; c < V; ++c)
      whole = whole && (alive[c] == EVERY || c >= n_mine);
    if (__builtin_amdgcn_ballot_w64(!whole) != 0) {
      // somewhere in the wave a column has met a hole: select and count
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        unsigned int n = 0;
#pragma unroll
        for (int c = 0; c < V; ++c) {
          const bool dead = ((alive[c] >> f) & 1u) == 0;
          res[f][c] = dead ? undef : res[f][c];
          n += (unsigned int)__popcll(__builtin_amdgcn_ballot_w64(dead && c < n_mine));
        }
        count(f, k, n);
      }
    }
#pragma unroll
    for (int f = 0; f < NF; ++f)
      walk_store<V>(P.out[walk_here(f)] + at, res[f], n_mine);
  };

  Level L[R];
#pragma unroll
  for (int c = 0; c < V; ++c) {
    L[2].c[c] = 0.f;
#pragma unroll
    for (int f = 0; f < NF; ++f)
      L[2].x[f][c] = 0.f;
  }
  load(L[0], 0);
  load(L[1], 1);
  if (2 < nlev)
    load(L[2], 2);

  advance(std::true_type(), L[0], 0);
  if (R < nlev)
    load(L[0], R);
  for (int j0 = 1; j0 < nlev; j0 += R) {
#pragma unroll
    for (int d = 0; d < R; ++d) {
      const int j = j0 + d; // j0 is 1 more than a multiple of R: position j sits in slot (1 + d) % R
      if (j < nlev) {
        Level& cur = L[(1 + d) % R];
        advance(std::false_type(), cur, j);
        if (j + R < nlev)
          load(cur, j + R);
      }
    }
  }

  if (lds) {
    __syncthreads();
    for (int j = threadIdx.x; j < NF * nlev; j += 256) {
      const unsigned int n = s_cnt[j];
      if (n != 0) {
        const int f = j / nlev, k = j - f * nlev;
        atomicAdd(P.n_undefined + (long)(f0 + f) * nlev + k, (u64)n);
      }
    }
  }
}

template <int KIND, bool LOG, int NF>
hipError_t launch_v(const VcumulParams& P, hipStream_t stream)
{
  const int per_block = 256 * (P.vec4 ? 4 : 1);
  const dim3 grid((unsigned int)(((long)P.n + per_block - 1) / per_block)), block(256);
  const size_t lds = P.lds_counts ? (size_t)NF * (size_t)P.nlev * sizeof(unsigned int) : 0;
  if (P.vec4)
    hipLaunchKernelGGL((vcumul_kernel<KIND, LOG, NF, 4>), grid, block, lds, stream, P);
  else
    hipLaunchKernelGGL((vcumul_kernel<KIND, LOG, NF, 1>), grid, block, lds, stream, P);
  return hipGetLastError();
}

template <int KIND, bool LOG>
hipError_t launch_nf(const VcumulParams& P, hipStream_t stream)
{
  static_assert(VCUMUL_PASS == 4, "one case per field count of a launch");
  switch (P.nfields) {
  case 1:
    return launch_v<KIND, LOG, 1>(P, stream);
  case 2:
    return launch_v<KIND, LOG, 2>(P, stream);
  case 3:
    return launch_v<KIND, LOG, 3>(P, stream);
  case 4:
    return launch_v<KIND, LOG, 4>(P, stream);
  default:
    return hipErrorInvalidValue;
  }
}

template <int KIND>
hipError_t launch_method(const VcumulParams& P, hipStream_t stream)
{
  return P.method != 0 ? launch_nf<KIND, true>(P, stream) : launch_nf<KIND, false>(P, stream);
}

} // namespace

hipError_t launch_vcumul(const VcumulParams& prm, hipStream_t stream)
{
  if (prm.n <= 0)
    return hipSuccess;
  if (prm.nlev < 2 || prm.f0 < 0 || prm.f0 + prm.nfields > VCUMUL_MAX_FIELDS || (prm.method != 0 && prm.method != 1) || (prm.from != 0 && prm.from != 1))
    return hipErrorInvalidValue;
  VcumulParams P = prm;
  // the workgroup's counters in LDS where they fit into half of what two resident workgroups may share
  P.lds_counts = (size_t)VCUMUL_PASS * (size_t)P.nlev * sizeof(unsigned int) <= 32768 ? 1 : 0;
  switch (P.kind) {
  case VDERIV_HYBRID:
    return launch_method<VDERIV_HYBRID>(P, stream);
  case VDERIV_FIELD:
    return launch_method<VDERIV_FIELD>(P, stream);
  case VDERIV_LEVELS:
    return launch_method<VDERIV_LEVELS>(P, stream);
  default:
    return hipErrorInvalidValue;
  }
}

} // namespace mifc
