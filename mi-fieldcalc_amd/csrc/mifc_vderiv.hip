// mifc_vderiv.hip -- vertical derivatives of level batches, with vector magnitude (mifc_vderiv_hlevels / mifc_vderiv_fields /
// mifc_vderiv_levels, include/mifc.h; EXTENSION: the reference has no function that crosses levels).
//
// The walk is the one of mifc_vinterp.hip and mifc_vlayer.hip: consecutive lanes own consecutive cells, four each through
// 16-byte loads (V = 4) or one each (V = 1), a lane keeps its cells for all levels, three level slots rotate (the k loop
// unrolled three times so that the slots are static), the per-level scalars come from a small table through the constant
// address space.  What differs: this kernel writes a full batch.  Output level k needs the levels k - 1, k and k + 1, so
// it is stored as soon as level k + 1 has arrived; the slots hold k, k + 1 and k + 2 and level k - 1 is carried beside
// them, so the loads stay two levels ahead of the level being stored, every input level is read once and every output
// level written once.  A level has two bodies.  Where every cell of the wave has both sides taking part for every field of
// the launch and no zero denominator -- one ballot -- the fast body runs: the one or two double divisions of the weights
// per cell, then per field two or three subtractions, multiplications and one addition, no select.  The general body does
// the rest (the first and the last level, holes, equal or undefined coordinates): it sorts every (field, cell) into
// both / lower only / upper only / undef, computes only the weights that some cell of the wave needs and selects.  With
// the coordinate given per level (VDERIV_LEVELS) the weights are the same for every cell: the host has divided, they come
// in through scalar loads.  Undefined cells are counted per level and field by ballot into LDS and leave the workgroup as
// one atomic per counter that is not zero.  The rules themselves -- the sides, the weights, the
// derivative of one (field, cell) -- are stated in mifc_vderiv_cell.h, for this kernel and pvort_kernel (mifc_pvort.hip).
#include "mifc_kernels.h"
#include "mifc_vderiv_cell.h"

#include <type_traits>

namespace mifc {

namespace {

template <int KIND, int W, int NF, int V>
__global__ __launch_bounds__(256, 2) void vderiv_kernel(const VderivParams P)
{
  constexpr int R = 3;       // level slots
  constexpr int NM = NF / 2; // vectors
  extern __shared__ unsigned int s_cnt[]; // [NF + NM][nlev]
  const int nlev = P.nlev, f0 = P.f0;
  const bool lds = P.lds_counts != 0;
  const int method = P.method;
  if (lds) {
    for (int j = threadIdx.x; j < (NF + NM) * nlev; j += 256)
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
  const ConstDoubles lev_w = (ConstDoubles)(unsigned long long)P.lev_w;
  typedef WalkLevel<NF, V> Level;

  auto load = [&](Level& L, int k) {
    const long off = (long)walk_here(k) * P.in_stride + block0; // (k opaque: no induction variable per pointer)
    if constexpr (KIND == VDERIV_FIELD)
      walk_load<V>(L.c, lane_of(P.coord + off));
#pragma unroll
    for (int f = 0; f < NF; ++f)
      walk_load<V>(L.x[f], lane_of(P.fields[f] + off));
  };

  // a coordinate that is not usable is carried as NaN (rule 1)
  float ps[V];
  if constexpr (KIND == VDERIV_HYBRID) {
    walk_load<V>(ps, lane_of(P.coord + block0));
    walk_usable_ps<V>(ps, P.ps_all != 0, undef);
  }

  auto count = [&](int slot, int k, unsigned int n) {
    // (the lane test and the row of the counter computed here, not kept in SGPRs through the walk)
    if (n != 0 && (walk_here_v(threadIdx.x) & 63) == 0) {
      const int row = walk_here(nlev), first = walk_here(f0);
      if (lds)
        atomicAdd(&s_cnt[slot * row + k], n);
      else if (slot < NF)
        atomicAdd(P.n_undefined + (long)(first + slot) * row + k, (u64)n);
      else
        atomicAdd(P.n_undefined_mag + (long)(first / 2 + slot - NF) * row + k, (u64)n);
    }
  };

  // stores level k: the derivatives and / or the magnitudes; FAST: nothing is undef, nothing to count
  auto emit = [&](auto fast, const float (&res)[NF][V], const unsigned int (&cls)[V], int k) {
    constexpr bool FAST = decltype(fast)::value;
    const long at = (long)walk_here(k) * P.out_stride + i0;
    const int n_mine = (int)walk_here_v((unsigned int)n_cells); // (compared here: no lane masks that live through the walk)
    if constexpr ((W & VDERIV_DERIV) != 0) {
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        if constexpr (!FAST) {
          unsigned int n = 0;
#pragma unroll
          for (int c = 0; c < V; ++c)
            n += (unsigned int)__popcll(__builtin_amdgcn_ballot_w64(((cls[c] >> (2 * f)) & 3u) == 0 && c < n_mine));
          count(f, k, n);
        }
        walk_store<V>(P.out[walk_here(f)] + at, res[f], n_mine);
      }
    }
    if constexpr ((W & VDERIV_MAG) != 0) {
#pragma unroll
      for (int j = 0; j < NM; ++j) {
        float m[V];
#pragma unroll
        for (int c = 0; c < V; ++c)
          m[c] = absval(res[2 * j][c], res[2 * j + 1][c]); // rule 8
        if constexpr (!FAST) {
          unsigned int n = 0;
#pragma unroll
          for (int c = 0; c < V; ++c) {
            const bool bad = ((cls[c] >> (4 * j)) & 3u) == 0 || ((cls[c] >> (4 * j + 2)) & 3u) == 0;
            m[c] = bad ? undef : m[c];
            n += (unsigned int)__popcll(__builtin_amdgcn_ballot_w64(bad && c < n_mine));
          }
          count(NF + j, k, n);
        }
        walk_store<V>(P.mag[walk_here(j)] + at, m, n_mine);
      }
    }
  };

  // Output level k from the levels k - 1 (lo), k (cur) and k + 1 (hi) and their coordinates cp, cc, cn.
  // dfp, dfk, dfn: the words of vderiv_defined for the three levels.  The rules are those of mifc_vderiv_cell.h.
  auto level = [&](const Level& lo, const Level& cur, const Level& hi, const float (&cp)[V], const float (&cc)[V], const float (&cn)[V],
                   const unsigned int (&dfp)[V], const unsigned int (&dfk)[V], const unsigned int (&dfn)[V], unsigned int bits_k, int k) {
    const bool weighted = walk_here(method) != 0; // (tested here: as lane masks for the selects it would sit in four SGPRs through the walk)
    unsigned int cm[V];
    double h1[V], h2[V], den[V];
    vderiv_cell_mask<KIND, V>(cm, h1, h2, den, cp, cc, cn, bits_k, weighted);
    auto both_weights = [&](double (&wa)[V], double (&wb)[V]) {
#pragma unroll
      for (int c = 0; c < V; ++c)
        vderiv_both_weights<KIND>(wa[c], wb[c], h1[c], h2[c], den[c], weighted, lev_w, k);
    };

    unsigned int cls[V];
    unsigned int every = SIDE_BOTH, any = 0;
#pragma unroll
    for (int c = 0; c < V; ++c)
      cls[c] = vderiv_classify<NF>(every, any, cm[c], dfp[c], dfk[c], dfn[c]);
    const bool good = every == SIDE_BOTH;

    float res[NF][V];
    if (__builtin_amdgcn_ballot_w64(!good) == 0) {
      // the fast body: both sides everywhere in the wave
      double wa[V], wb[V];
      both_weights(wa, wb);
      if (weighted) {
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
          for (int c = 0; c < V; ++c)
            res[f][c] = (float)vderiv_both(lo.x[f][c], cur.x[f][c], hi.x[f][c], wa[c], wb[c], true);
      } else {
#pragma unroll
        for (int f = 0; f < NF; ++f)
#pragma unroll
          for (int c = 0; c < V; ++c)
            res[f][c] = (float)vderiv_both(lo.x[f][c], cur.x[f][c], hi.x[f][c], wa[c], wb[c], false);
      }
      emit(std::true_type(), res, cls, k);
      return;
    }

    // the general body: only the weights that some cell of the wave needs
    double wl[V], wh[V], wa[V], wb[V];
#pragma unroll
    for (int c = 0; c < V; ++c)
      wl[c] = wh[c] = wa[c] = wb[c] = 0.0;
    if (__builtin_amdgcn_ballot_w64((any & (1u << (SIDE_LOWER - 1))) != 0) != 0) {
#pragma unroll
      for (int c = 0; c < V; ++c)
        wl[c] = vderiv_one_weight<KIND, false>(h1[c], lev_w, k);
    }
    if (__builtin_amdgcn_ballot_w64((any & (1u << (SIDE_UPPER - 1))) != 0) != 0) {
#pragma unroll
      for (int c = 0; c < V; ++c)
        wh[c] = vderiv_one_weight<KIND, true>(h2[c], lev_w, k);
    }
    if (__builtin_amdgcn_ballot_w64((any & (1u << (SIDE_BOTH - 1))) != 0) != 0)
      both_weights(wa, wb);
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int c = 0; c < V; ++c) {
        const unsigned int s = (cls[c] >> (2 * f)) & 3u;
        const double r = vderiv_sided(s, lo.x[f][c], cur.x[f][c], hi.x[f][c], wl[c], wh[c], wa[c], wb[c], weighted);
        res[f][c] = s == 0 ? undef : (float)r;
      }
    emit(std::false_type(), res, cls, k);
  };

  const float nan = __int_as_float(0x7fc00000);
  Level L[R], prev;
#pragma unroll
  for (int c = 0; c < V; ++c) {
    prev.c[c] = L[2].c[c] = 0.f;
#pragma unroll
    for (int f = 0; f < NF; ++f)
      prev.x[f][c] = L[2].x[f][c] = 0.f;
  }
  load(L[0], 0);
  load(L[1], 1);
  if (2 < nlev)
    load(L[2], 2);

  unsigned int bits_k = lev_bits[0];
  float cp[V], cc[V];
  unsigned int dfp[V], dfk[V];
#pragma unroll
  for (int c = 0; c < V; ++c) {
    cp[c] = nan;
    dfp[c] = 0;
  }
  walk_coordinate<KIND, V>(cc, L[0].c, ps, ab, nlev, 0, bits_k, undef);
  vderiv_defined<NF, V>(dfk, L[0], bits_k >> f0, undef);

  for (int k0 = 0; k0 < nlev; k0 += R) {
#pragma unroll
    for (int d = 0; d < R; ++d) {
      const int k = k0 + d; // the output level
      if (k < nlev) {
        Level& cur = L[d];
        Level& nx = L[(d + 1) % R];
        const bool has_next = k + 1 < nlev;
        const unsigned int bits_n = lev_bits[has_next ? k + 1 : k];
        float cn[V];
        walk_coordinate<KIND, V>(cn, nx.c, ps, ab, nlev, has_next ? k + 1 : k, bits_n, undef);
#pragma unroll
        for (int c = 0; c < V; ++c)
          cn[c] = has_next ? cn[c] : nan;
        unsigned int dfn[V];
        vderiv_defined<NF, V>(dfn, nx, bits_n >> f0, undef); // (no level k + 1: cn is NaN)
        level(prev, cur, nx, cp, cc, cn, dfp, dfk, dfn, bits_k, k);
        // level k becomes level k - 1, level k + 1 level k; level k's slot takes level k + 3
        prev = cur;
        bits_k = bits_n;
#pragma unroll
        for (int c = 0; c < V; ++c) {
          cp[c] = cc[c];
          cc[c] = cn[c];
          dfp[c] = dfk[c];
          dfk[c] = dfn[c];
        }
        if (k + R < nlev)
          load(cur, k + R);
      }
    }
  }

  if (lds) {
    __syncthreads();
    for (int j = threadIdx.x; j < (NF + NM) * nlev; j += 256) {
      const unsigned int n = s_cnt[j];
      if (n != 0) {
        const int slot = j / nlev, k = j - slot * nlev;
        if (slot < NF)
          atomicAdd(P.n_undefined + (long)(f0 + slot) * nlev + k, (u64)n);
        else
          atomicAdd(P.n_undefined_mag + (long)(f0 / 2 + slot - NF) * nlev + k, (u64)n);
      }
    }
  }
}

template <int KIND, int W, int NF>
hipError_t launch_v(const VderivParams& P, hipStream_t stream)
{
  const int per_block = 256 * (P.vec4 ? 4 : 1);
  const dim3 grid((unsigned int)(((long)P.n + per_block - 1) / per_block)), block(256);
  const size_t lds = P.lds_counts ? (size_t)(NF + NF / 2) * (size_t)P.nlev * sizeof(unsigned int) : 0;
  if (P.vec4)
    hipLaunchKernelGGL((vderiv_kernel<KIND, W, NF, 4>), grid, block, lds, stream, P);
  else
    hipLaunchKernelGGL((vderiv_kernel<KIND, W, NF, 1>), grid, block, lds, stream, P);
  return hipGetLastError();
}

template <int KIND, int W>
hipError_t launch_nf(const VderivParams& P, hipStream_t stream)
{
  static_assert(VDERIV_PASS == 4, "one case per field count of a launch");
  switch (P.nfields) {
  case 1:
    if constexpr ((W & VDERIV_MAG) == 0)
      return launch_v<KIND, W, 1>(P, stream);
    return hipErrorInvalidValue; // (a magnitude takes a pair)
  case 2:
    return launch_v<KIND, W, 2>(P, stream);
  case 3:
    if constexpr ((W & VDERIV_MAG) == 0)
      return launch_v<KIND, W, 3>(P, stream);
    return hipErrorInvalidValue;
  case 4:
    if constexpr (vderiv_pass_fields(W) >= 4)
      return launch_v<KIND, W, 4>(P, stream);
    return hipErrorInvalidValue; // (the instances beyond a launch's capacity do not exist)
  default:
    return hipErrorInvalidValue;
  }
}

template <int KIND>
hipError_t launch_what(const VderivParams& P, hipStream_t stream)
{
  switch (P.what) {
  case VDERIV_DERIV:
    return launch_nf<KIND, VDERIV_DERIV>(P, stream);
  case VDERIV_MAG:
    return launch_nf<KIND, VDERIV_MAG>(P, stream);
  case VDERIV_DERIV | VDERIV_MAG:
    return launch_nf<KIND, VDERIV_DERIV | VDERIV_MAG>(P, stream);
  default:
    return hipErrorInvalidValue;
  }
}

} // namespace

hipError_t launch_vderiv(const VderivParams& prm, hipStream_t stream)
{
  if (prm.n <= 0)
    return hipSuccess;
  if (prm.nlev < 2 || prm.f0 < 0 || (prm.f0 & 1) != 0 || prm.f0 + prm.nfields > VDERIV_MAX_FIELDS)
    return hipErrorInvalidValue;
  VderivParams P = prm;
  // the workgroup's counters in LDS where they fit into half of what two resident workgroups may share
  P.lds_counts = (size_t)(VDERIV_PASS + VDERIV_PASS / 2) * (size_t)P.nlev * sizeof(unsigned int) <= 32768 ? 1 : 0;
  switch (P.kind) {
  case VDERIV_HYBRID:
    return launch_what<VDERIV_HYBRID>(P, stream);
  case VDERIV_FIELD:
    return launch_what<VDERIV_FIELD>(P, stream);
  case VDERIV_LEVELS:
    return launch_what<VDERIV_LEVELS>(P, stream);
  default:
    return hipErrorInvalidValue;
  }
}

} // namespace mifc
