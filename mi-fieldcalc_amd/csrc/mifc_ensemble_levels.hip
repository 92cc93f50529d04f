// mifc_ensemble_levels.hip -- several per-cell reductions over ensemble members in ONE pass over the members, for
// [nlev][ny][nx] batches (mifc_ensemble_levels, include/mifc.h; FieldCalculations.cc:2671-2860).
//
// A lane owns four consecutive cells of a level (grid.y walks the levels) and walks the members once, in index order,
// in groups of eight whose 16-byte loads are all issued before the first is consumed.  Every live product keeps its own
// accumulators and is fed the value in the reference's own sequence of operations -- the per-product code below restates
// ens_member / ens_finish of mifc_ensemble.hip statement by statement -- so that each output is bit for bit what the
// single-field kernel writes.  Nothing is shared between two products except the load and the is_defined test of the value.
//
// Which products are live is uniform over the launch.  The kernel is specialised over a few shapes (Welford on / off, the
// sumFields / extremeValue family on / off, room for 0 / 3 / 8 probability products); inside a shape the slots are
// switched by wave-uniform tests of `live`.  Every accumulator is a named register array indexed by unrolled loops
// only: a run-time product number as an index would put the arrays in scratch.
// The undefined counts are kept per slot and level and handed over per workgroup.
#include "mifc_device.h"
#include "mifc_kernels.h"

namespace mifc {

namespace {

constexpr int MB = 8; // members per group of loads

__device__ __forceinline__ u64 lv_none(const EnsLevelsParams& P, int lev, int w)
{
  return P.inline_args ? P.none_inline[lev] : P.tab.none_bits[(long)lev * P.words + w];
}
__device__ __forceinline__ int lv_ndef(const EnsLevelsParams& P, int lev)
{
  return P.inline_args ? (int)P.ndef_inline[lev] : P.tab.ndef[lev];
}
__device__ __forceinline__ unsigned int lv_in_all(const EnsLevelsParams& P, int lev)
{
  return P.inline_args ? P.in_all_inline[lev] : P.tab.in_all[lev];
}

template <int C>
__device__ __forceinline__ void lv_load(const float* p, long at, float (&f)[C])
{
  if constexpr (C == 4) {
    const float4 v = *reinterpret_cast<const float4*>(p + at);
    f[0] = v.x;
    f[1] = v.y;
    f[2] = v.z;
    f[3] = v.w;
  } else {
    f[0] = p[at];
  }
}
template <int C>
__device__ __forceinline__ void lv_store(float* p, long at, const float (&o)[C])
{
  if constexpr (C == 4) {
    typedef float v4f __attribute__((ext_vector_type(4)));
    v4f t;
    t.x = o[0];
    t.y = o[1];
    t.z = o[2];
    t.w = o[3];
    __builtin_nontemporal_store(t, reinterpret_cast<v4f*>(p + at));
  } else {
    p[at] = o[0];
  }
}

// the workgroup's counts of level l: one atomic per live slot, or the slot's entry of the partial-count table
__device__ __forceinline__ void lv_hand_over(const EnsLevelsParams& P, int l, const unsigned int (&bad)[ENSLV_SLOTS])
{
  __shared__ unsigned int s_total[ENSLV_SLOTS];
  if (threadIdx.x < ENSLV_SLOTS)
    s_total[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < ENSLV_SLOTS; ++k) {
    if (((P.live >> k) & 1u) && __builtin_amdgcn_ballot_w64(bad[k] != 0) != 0) {
      const unsigned int s = wave_sum(bad[k]);
      if ((threadIdx.x & 63) == 0)
        atomicAdd(&s_total[k], s);
    }
  }
  __syncthreads();
  if (threadIdx.x < ENSLV_SLOTS && ((P.live >> threadIdx.x) & 1u)) {
    const unsigned int t = s_total[threadIdx.x];
    if (P.partials)
      P.partials[((long)threadIdx.x * P.nlev + l) * gridDim.x + blockIdx.x] = t; // always written: the table is not zeroed
    else if (t != 0)
      atomicAdd(P.n_undefined + (long)threadIdx.x * P.call_nlev + P.lev0 + l, (u64)t);
  }
}

// per-cell state of every product, C cells of one lane (ens_init of mifc_ensemble.hip)
template <int C, int NP>
struct LvCells
{
  float sum_r[C];
  bool sum_live[C];
  float mean_r[C];
  int mean_n[C];
  float w_m[C], w_m2[C];
  int w_n[C];
  float e1_r[C], e2_r[C], e3_r[C], e3_tmp[C], e4_r[C], e4_tmp[C];
  float pr[NP > 0 ? NP : 1][C];
};
// what is uniform over a level: the live slots and the input flags of the products that have one
struct LvSwitch
{
  bool do_sum, do_mean, do_w, do_e1, do_e2, do_e3, do_e4;
  bool sum_all, e1_all, e2_all, e3_all, e4_all;
};

// member j's values f of the lane's cells into every live product: ens_member of mifc_ensemble.hip, product by product
template <int C, bool WELFORD, bool FLAGGED, int NP>
__device__ __forceinline__ void lv_member(const EnsLevelsParams& P, const LvSwitch& w, LvCells<C, NP>& a, int j, const float (&v)[C], bool m_all,
                                          bool m_none)
{
  const float undef = P.undef;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float f = v[c];
    const bool def = is_def(f, undef);
    if (w.do_mean) { // :2709-2714
      if (m_all || def) {
        a.mean_n[c]++;
        a.mean_r[c] += f;
      }
    }
    if (WELFORD && w.do_w) { // :2739-2747, Welford in float
      if (m_all || def) {
        const float delta = f - a.w_m[c];
        a.w_n[c] += 1;
        a.w_m[c] += delta / a.w_n[c];
        a.w_m2[c] += delta * (f - a.w_m[c]);
      }
    }
    if (FLAGGED) {
      if (w.do_sum && a.sum_live[c]) { // :2682-2690: the first undefined member ends the cell
        if (w.sum_all || def) {
          a.sum_r[c] += f;
        } else {
          a.sum_r[c] = undef;
          a.sum_live[c] = false;
        }
      }
      if (w.do_e1) { // :2778-2783
        if (a.e1_r[c] == undef || ((w.e1_all || def) && a.e1_r[c] < f))
          a.e1_r[c] = f;
      }
      if (w.do_e2) {
        if (a.e2_r[c] == undef || ((w.e2_all || def) && a.e2_r[c] > f))
          a.e2_r[c] = f;
      }
      if (w.do_e3) { // :2792-2798
        if (a.e3_tmp[c] == undef || ((w.e3_all || def) && a.e3_tmp[c] < f)) {
          a.e3_tmp[c] = f;
          a.e3_r[c] = (float)j;
        }
      }
      if (w.do_e4) {
        if (a.e4_tmp[c] == undef || ((w.e4_all || def) && a.e4_tmp[c] > f)) {
          a.e4_tmp[c] = f;
          a.e4_r[c] = (float)j;
        }
      }
    }
    if (NP > 0) { // :2840-2848: members flagged NONE_DEFINED do not take part
      if (!m_none) {
#pragma unroll
        for (int i = 0; i < NP; ++i)
          if ((f != undef) && (!((P.check_above >> i) & 1u) || f > P.value_above[i]) && (!((P.check_below >> i) & 1u) || f < P.value_below[i]))
            a.pr[i][c] += 1;
      }
    }
  }
}

// C cells per lane (4: 16-byte loads and non-temporal stores, 1: the scalar form); WELFORD: slot 2; FLAGGED: the
// products with one in/out flag, slot 0 and slots 3..6; NP: probability slots 7 .. 7 + NP - 1
template <int C, bool WELFORD, bool FLAGGED, int NP>
__global__ __launch_bounds__(256) void ensemble_levels_kernel(const EnsLevelsParams P)
{
  const float undef = P.undef;
  LvSwitch w;
  w.do_sum = FLAGGED && (P.live & 1u);
  w.do_mean = (P.live >> 1) & 1u;
  w.do_w = WELFORD && ((P.live >> 2) & 1u);
  w.do_e1 = FLAGGED && ((P.live >> 3) & 1u);
  w.do_e2 = FLAGGED && ((P.live >> 4) & 1u);
  w.do_e3 = FLAGGED && ((P.live >> 5) & 1u);
  w.do_e4 = FLAGGED && ((P.live >> 6) & 1u);
  const bool do_sum = w.do_sum, do_mean = w.do_mean, do_w = w.do_w, do_e1 = w.do_e1, do_e2 = w.do_e2, do_e3 = w.do_e3, do_e4 = w.do_e4;
  const long lanes = P.n / C;
  for (int l = blockIdx.y; l < P.nlev; l += gridDim.y) { // uniform per workgroup
    const int lev = P.lev0 + l;
    const unsigned int in_all = FLAGGED ? lv_in_all(P, lev) : 0u;
    w.sum_all = in_all & 1u;
    w.e1_all = (in_all >> 1) & 1u;
    w.e2_all = (in_all >> 2) & 1u;
    w.e3_all = (in_all >> 3) & 1u;
    w.e4_all = (in_all >> 4) & 1u;
    const int ndef = NP > 0 ? lv_ndef(P, lev) : 0;
    unsigned int bad[ENSLV_SLOTS];
#pragma unroll
    for (int k = 0; k < ENSLV_SLOTS; ++k)
      bad[k] = 0;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < lanes; q += (long)gridDim.x * 256) {
      const long at = (long)l * P.stride + q * C;
      LvCells<C, NP> a;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        a.sum_r[c] = 0.f;
        a.sum_live[c] = true;
        a.mean_r[c] = 0.f;
        a.mean_n[c] = 0;
        a.w_m[c] = 0.f;
        a.w_m2[c] = 0.f;
        a.w_n[c] = 0;
        a.e1_r[c] = a.e2_r[c] = a.e3_r[c] = a.e3_tmp[c] = a.e4_r[c] = a.e4_tmp[c] = undef;
#pragma unroll
        for (int i = 0; i < NP; ++i)
          a.pr[i][c] = 0.f;
      }
      // members in groups of MB: all loads of a group are issued before the first is consumed (the accumulation
      // itself stays in member order); the empty slots of the last group load the last member again (a cache hit)
      // and are skipped, so that no load sits behind a branch
      for (int j0 = 0; j0 < P.nmem; j0 += MB) {
        float v[MB][C];
#pragma unroll
        for (int k = 0; k < MB; ++k)
          lv_load<C>(arg_mem(P, j0 + k < P.nmem ? j0 + k : P.nmem - 1), at, v[k]);
        const u64 all_w = arg_all(P, lev, j0 >> 6) >> (j0 & 63), none_w = NP > 0 ? lv_none(P, lev, j0 >> 6) >> (j0 & 63) : 0ull;
#pragma unroll
        for (int k = 0; k < MB; ++k)
          if (j0 + k < P.nmem)
            lv_member<C, WELFORD, FLAGGED, NP>(P, w, a, j0 + k, v[k], (all_w >> k) & 1ull, (none_w >> k) & 1ull);
      }
      // ens_finish of mifc_ensemble.hip, slot by slot
      float o[C];
      if (do_sum) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
          o[c] = a.sum_r[c];
          bad[0] += a.sum_live[c] ? 0u : 1u;
        }
        lv_store<C>(P.out[0], at, o);
      }
      if (do_mean) { // :2715-2720
#pragma unroll
        for (int c = 0; c < C; ++c) {
          if (a.mean_n[c] > 0) {
            o[c] = a.mean_r[c] / a.mean_n[c];
          } else {
            o[c] = undef;
            bad[1] += 1u;
          }
        }
        lv_store<C>(P.out[1], at, o);
      }
      if (do_w) { // :2748-2753, sqrt is the double function there
#pragma unroll
        for (int c = 0; c < C; ++c) {
          if (a.w_n[c] > 0) {
            o[c] = (float)sqrt((double)(a.w_m2[c] / a.w_n[c]));
          } else {
            o[c] = undef;
            bad[2] += 1u;
          }
        }
        lv_store<C>(P.out[2], at, o);
      }
      if (do_e1) { // :2784
#pragma unroll
        for (int c = 0; c < C; ++c)
          bad[3] += a.e1_r[c] == undef ? 1u : 0u;
        lv_store<C>(P.out[3], at, a.e1_r);
      }
      if (do_e2) {
#pragma unroll
        for (int c = 0; c < C; ++c)
          bad[4] += a.e2_r[c] == undef ? 1u : 0u;
        lv_store<C>(P.out[4], at, a.e2_r);
      }
      if (do_e3) { // :2799
#pragma unroll
        for (int c = 0; c < C; ++c)
          bad[5] += a.e3_r[c] == undef ? 1u : 0u;
        lv_store<C>(P.out[5], at, a.e3_r);
      }
      if (do_e4) {
#pragma unroll
        for (int c = 0; c < C; ++c)
          bad[6] += a.e4_r[c] == undef ? 1u : 0u;
        lv_store<C>(P.out[6], at, a.e4_r);
      }
#pragma unroll
      for (int i = 0; i < NP; ++i) { // :2850-2856
        if ((P.live >> (ENSLV_PROB0 + i)) & 1u) {
#pragma unroll
          for (int c = 0; c < C; ++c) {
            if (ndef == 0) {
              o[c] = undef;
              bad[ENSLV_PROB0 + i] += 1u;
            } else {
              o[c] = ((P.percent >> i) & 1u) ? (float)((double)a.pr[i][c] / (ndef / 100.0)) : a.pr[i][c];
            }
          }
          lv_store<C>(P.out[ENSLV_PROB0 + i], at, o);
        }
      }
    }
    lv_hand_over(P, l, bad);
  }
}

template <int C, bool WELFORD, bool FLAGGED, int NP>
void launch_shape(const EnsLevelsParams& P, dim3 grid, hipStream_t stream)
{
  hipLaunchKernelGGL((ensemble_levels_kernel<C, WELFORD, FLAGGED, NP>), grid, dim3(256), 0, stream, P);
}

template <bool WELFORD, bool FLAGGED>
void launch_tier(const EnsLevelsParams& P, int np, dim3 grid, hipStream_t stream)
{
  if (np == 0)
    launch_shape<4, WELFORD, FLAGGED, 0>(P, grid, stream);
  else if (np == 8)
    launch_shape<4, WELFORD, FLAGGED, 8>(P, grid, stream);
  else if constexpr (!WELFORD || FLAGGED)
    // <true, false, 3> is left out: the compiler reserves a 36-byte private segment for it that no instruction touches,
    // and a dispatch would set scratch up for it; such a list runs on the shape with the flagged family switched off by
    // `live` (ensemble_levels_shape says so)
    launch_shape<4, WELFORD, FLAGGED, 3>(P, grid, stream);
}

} // namespace

hipError_t launch_ensemble_levels(const EnsLevelsParams& prm, hipStream_t stream)
{
  if (prm.n <= 0 || prm.nlev <= 0 || (prm.live & ((1u << ENSLV_SLOTS) - 1u)) == 0)
    return hipSuccess;
  EnsLevelsParams P = prm;
  const EnsLevelsShape s = ensemble_levels_shape(P);
  const int gx = ensemble_levels_blocks(P.n, s.c == 4);
  const int gy = P.nlev < 65535 ? P.nlev : 65535;
  // big levels: per-workgroup counts in partials[slot][level][workgroup], added up behind the launch
  const bool parts = s.partials;
  if (!parts)
    P.partials = nullptr;
  const dim3 grid(gx, gy);
  if (s.c == 1) // the scalar form: one shape with everything in it, the slots switched by `live`
    launch_shape<1, true, true, ENSLV_NPROB>(P, grid, stream);
  else if (s.welford && s.flagged)
    launch_tier<true, true>(P, s.np, grid, stream);
  else if (s.welford)
    launch_tier<true, false>(P, s.np, grid, stream);
  else if (s.flagged)
    launch_tier<false, true>(P, s.np, grid, stream);
  else
    launch_tier<false, false>(P, s.np, grid, stream);
  hipError_t e = hipGetLastError();
  for (int k = 0; k < ENSLV_SLOTS && e == hipSuccess && parts; ++k)
    if ((P.live >> k) & 1u)
      e = launch_count_partials_levels(P.partials + (size_t)k * P.nlev * gx, gx, P.nlev, P.n_undefined + (size_t)k * P.call_nlev + P.lev0, stream);
  return e;
}

} // namespace mifc
