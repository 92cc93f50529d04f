// mifc_vinterp.hip -- level batches interpolated to constant surfaces (mifc_vinterp_hlevels / mifc_vinterp_fields,
// include/mifc.h; EXTENSION: the reference has no function that crosses levels).
//
// Columns are independent and x is the fastest index: consecutive lanes own consecutive cells, four each through
// 16-byte loads (V = 4) or one each (V = 1) where the batch is off the 16-byte grid, so every load of a level is one
// contiguous row segment per wave.  A lane walks the levels of its cells ONCE: level k's coordinate and NF field values
// stay in registers, level k + 1 is loaded two pairs ahead of use (three level slots that rotate, the k loop unrolled
// three times so that the slots are static).  What makes the walk cheap is that the targets a wave has to look at per level are few: the
// wave reduces [min, max] of the coordinate pairs of its 64 * V cells to one interval, lane t compares target t's
// order-preserving integer key against it, and one ballot leaves the candidates in a bit mask -- none for most levels.  Per candidate the lanes test their own cells against a found-mask (one register per
// cell, one bit per target, hence VINTERP_PASS = 32 targets per launch), the weight is computed once per cell and the NF
// results are stored straight away; LOG takes its two log() only there, log(ct) comes from the host.  Targets never
// found are stored as undef behind the walk.  Undefined results are counted per wave by ballot into a table in LDS and
// leave the workgroup as one atomic per (field, target) that has something to count.
#include "mifc_column_walk.h"
#include "mifc_device.h"
#include "mifc_kernels.h"

namespace mifc {

namespace {

// the cells of a lane that `m` marks (all of them inside the launch): one 16-byte store where that is all four
template <int V>
__device__ __forceinline__ void vi_store(float* p, const float (&r)[V], const bool (&m)[V])
{
  if constexpr (V == 4) {
    if (m[0] && m[1] && m[2] && m[3]) {
      *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1], r[2], r[3]);
      return;
    }
  }
#pragma unroll
  for (int c = 0; c < V; ++c)
    if (m[c])
      p[c] = r[c];
}

// wave-wide minimum / maximum, the same value in every lane's SGPR afterwards
__device__ __forceinline__ float vi_wave_min(float x)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    x = fminf(x, __shfl_xor(x, off, 64));
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}
__device__ __forceinline__ float vi_wave_max(float x)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    x = fmaxf(x, __shfl_xor(x, off, 64));
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}

template <bool HYBRID, bool LOG, int NF, int V>
__global__ __launch_bounds__(256) void vinterp_kernel(const VinterpParams P)
{
  constexpr int R = 3; // level slots
  __shared__ unsigned int s_bad[NF * VINTERP_PASS];
  for (int j = threadIdx.x; j < NF * VINTERP_PASS; j += 256)
    s_bad[j] = 0;
  __syncthreads();

  const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * V;
  const long left = (long)P.n - i0;
  const int n_mine = left < 0 ? 0 : (left < V ? (int)left : V); // this lane's cells inside the launch: cells 0 .. n_mine - 1
  const long at = n_mine > 0 ? i0 : 0; // lanes past the end walk column group 0 and neither store nor count
  const float undef = P.undef;
  const int nlev = P.nlev, nt = P.nt;
  // the per-level scalars through the scalar cache (mifc_column_walk.h)
  const ConstFloats ab = (ConstFloats)(unsigned long long)P.ab;
  const ConstWords lev_bits = (ConstWords)(unsigned long long)P.lev_bits;

  auto load = [&](WalkLevel<NF, V>& L, int k) {
    const long off = (long)k * P.in_stride + at;
    if constexpr (!HYBRID)
      walk_load<V>(L.c, P.coord + off);
#pragma unroll
    for (int f = 0; f < NF; ++f)
      walk_load<V>(L.x[f], P.fields[f] + off);
  };

  // An undefined coordinate is carried as NaN: a NaN coordinate never brackets anyway (it fails both comparisons), so
  // "both ends defined" is one ordered compare of the pair, and no flag per cell has to live through the walk.
  float ps[V];
  if constexpr (HYBRID) {
    walk_load<V>(ps, P.coord + at);
    walk_usable_ps<V>(ps, P.ps_all != 0, undef);
  }
  auto coordinate = [&](const WalkLevel<NF, V>& L, int k, unsigned int bits, float (&cc)[V]) {
    walk_coordinate<HYBRID ? VDERIV_HYBRID : VDERIV_FIELD, V>(cc, L.c, ps, ab, nlev, k, bits, undef);
  };

  // level k lives in slot k % 3: at the pair (k, k + 1) the third slot holds level k + 2, already on its way, and the
  // slot of level k is loaded with level k + 3 as soon as the pair is done (two pairs ahead of its first use)
  WalkLevel<NF, V> L[R];
  load(L[0], 0);
  load(L[1], 1);
  if (2 < nlev)
    load(L[2], 2);
  // lane t < nt of the wave holds target t's key, the other lanes one below every interval (the key of -inf is larger)
  const int my_key = (int)(threadIdx.x & 63) < nt ? P.target_key[threadIdx.x & (VINTERP_PASS - 1)] : (int)0x80000000;

  unsigned int bits_k = lev_bits[0];
  float ck[V];
  coordinate(L[0], 0, bits_k, ck);
  unsigned int found[V]; // bit t: target t of the pass is done with (cells outside the launch: all of them, from the start)
#pragma unroll
  for (int c = 0; c < V; ++c)
    found[c] = c < n_mine ? 0u : 0xffffffffu;
  const float inf = __int_as_float(0x7f800000);

  for (int k0 = 0; k0 < nlev - 1; k0 += R) {
#pragma unroll
    for (int d = 0; d < R; ++d) {
      const int k = k0 + d; // the pair (k, k + 1)
      if (k < nlev - 1) {
        WalkLevel<NF, V>& cur = L[d];
        WalkLevel<NF, V>& nx = L[(d + 1) % R];
        const unsigned int bits_k1 = lev_bits[k + 1];
        float ck1[V], lo[V], hi[V];
        coordinate(nx, k + 1, bits_k1, ck1);
        float lane_lo = inf, lane_hi = -inf;
#pragma unroll
        for (int c = 0; c < V; ++c) {
          const bool pair = !__builtin_isunordered(ck[c], ck1[c]);
          lo[c] = pair ? fminf(ck[c], ck1[c]) : inf;
          hi[c] = pair ? fmaxf(ck[c], ck1[c]) : -inf;
          lane_lo = fminf(lane_lo, lo[c]);
          lane_hi = fmaxf(lane_hi, hi[c]);
        }
        // the targets inside the wave's interval, on integer keys (+ 0.f: -0 becomes +0, whose key orders like the float)
        const int wlo = vinterp_key(__float_as_int(vi_wave_min(lane_lo) + 0.f)), whi = vinterp_key(__float_as_int(vi_wave_max(lane_hi) + 0.f));
        unsigned int cand = (unsigned int)__builtin_amdgcn_ballot_w64(my_key >= wlo && my_key <= whi); // nt <= 32: the low half
        while (cand != 0) { // wave-uniform
          const int t = __builtin_ctz(cand);
          cand &= cand - 1;
          const float ct = P.target[t];
          // per cell, as bits of one register (1: this target is found here, 2: c_k == c_k+1, 4: LOG of a coordinate <= 0) --
          // as separate predicates they would each hold a pair of SGPRs through the body, which does not have them to spare
          unsigned int state[V];
          bool any = false;
#pragma unroll
          for (int c = 0; c < V; ++c) {
            const bool hit = ((found[c] >> t) & 1u) == 0 && lo[c] <= ct && ct <= hi[c];
            state[c] = hit ? 1u : 0u;
            any |= hit;
          }
          if (__builtin_amdgcn_ballot_w64(any) == 0)
            continue;
          // every lane goes through the arithmetic, the stores are masked: the counting below sees the whole wave
          double w[V];
#pragma unroll
          for (int c = 0; c < V; ++c) {
            found[c] |= state[c] << t;
            const float c0 = walk_here(ck[c]), c1 = walk_here(ck1[c]);
            state[c] |= c0 == c1 ? 2u : 0u;
            if constexpr (LOG) {
              state[c] |= !(fminf(c0, c1) > 0.f) ? 4u : 0u;
              const double lk = log((double)c0), lk1 = log((double)c1);
              w[c] = (P.target_log[t] - lk) / (lk1 - lk);
            } else {
              w[c] = ((double)ct - (double)c0) / ((double)c1 - (double)c0);
            }
            state[c] = walk_here_v(state[c]);
          }
          const unsigned int here_k = (unsigned int)walk_here((int)bits_k), here_k1 = (unsigned int)walk_here((int)bits_k1);
#pragma unroll
          for (int f = 0; f < NF; ++f) {
            const bool all_k = ((here_k >> f) & 1u) != 0, all_k1 = ((here_k1 >> f) & 1u) != 0;
            float r[V];
            bool hit[V];
            unsigned int n = 0;
#pragma unroll
            for (int c = 0; c < V; ++c) {
              const float xk = walk_here(cur.x[f][c]), xk1 = walk_here(nx.x[f][c]);
              const bool ok = (all_k || is_def(xk, undef)) && (all_k1 || is_def(xk1, undef)) && (state[c] & 4u) == 0;
              const double dk = (double)xk;
              const double diff = (double)xk1 - dk;
              const double prod = w[c] * diff;
              const float v = (float)(dk + prod);
              r[c] = ok ? ((state[c] & 2u) != 0 ? xk : v) : undef;
              hit[c] = (state[c] & 1u) != 0;
              n += (unsigned int)__popcll(__builtin_amdgcn_ballot_w64(hit[c] && !ok)); // the whole wave is here
            }
            vi_store<V>(P.out[walk_here(f)] + (long)(P.t0 + t) * P.out_stride + i0, r, hit);
            if (n != 0 && (threadIdx.x & 63) == 0)
              atomicAdd(&s_bad[f * VINTERP_PASS + t], n);
          }
        }
        // level k + 1 becomes level k; level k's slot takes level k + 3
        bits_k = bits_k1;
#pragma unroll
        for (int c = 0; c < V; ++c)
          ck[c] = ck1[c];
        if (k + R < nlev)
          load(cur, k + R);
      }
    }
  }

  // the targets without a bracket: undef in every field
  unsigned int missing_any = 0;
#pragma unroll
  for (int c = 0; c < V; ++c)
    missing_any |= ~found[c];
  missing_any &= nt >= 32 ? 0xffffffffu : (1u << nt) - 1u;
  // (wave-uniform set of targets that somebody misses: the union over the lanes)
  unsigned int todo = missing_any;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    todo |= (unsigned int)__shfl_xor((int)todo, off, 64);
  todo = (unsigned int)__builtin_amdgcn_readfirstlane((int)todo);
  while (todo != 0) {
    const int t = __builtin_ctz(todo);
    todo &= todo - 1;
    bool miss[V];
    float r[V];
    unsigned int n = 0;
#pragma unroll
    for (int c = 0; c < V; ++c) {
      miss[c] = ((found[c] >> t) & 1u) == 0;
      r[c] = undef;
      n += (unsigned int)__popcll(__builtin_amdgcn_ballot_w64(miss[c]));
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      vi_store<V>(P.out[walk_here(f)] + (long)(P.t0 + t) * P.out_stride + i0, r, miss);
      if ((threadIdx.x & 63) == 0)
        atomicAdd(&s_bad[f * VINTERP_PASS + t], n);
    }
  }

  __syncthreads();
  for (int j = threadIdx.x; j < NF * VINTERP_PASS; j += 256) {
    const int f = j / VINTERP_PASS, t = j % VINTERP_PASS;
    if (t < nt && s_bad[j] != 0)
      atomicAdd(P.n_undefined + (long)f * P.nt_call + P.t0 + t, (u64)s_bad[j]);
  }
}

template <bool HYBRID, bool LOG, int NF>
hipError_t launch_v(const VinterpParams& P, hipStream_t stream)
{
  const int per_block = 256 * (P.vec4 ? 4 : 1);
  const dim3 grid((unsigned int)(((long)P.n + per_block - 1) / per_block)), block(256);
  if (P.vec4)
    hipLaunchKernelGGL((vinterp_kernel<HYBRID, LOG, NF, 4>), grid, block, 0, stream, P);
  else
    hipLaunchKernelGGL((vinterp_kernel<HYBRID, LOG, NF, 1>), grid, block, 0, stream, P);
  return hipGetLastError();
}

template <bool HYBRID, bool LOG>
hipError_t launch_nf(const VinterpParams& P, hipStream_t stream)
{
  switch (P.nfields) {
  case 1:
    return launch_v<HYBRID, LOG, 1>(P, stream);
  case 2:
    return launch_v<HYBRID, LOG, 2>(P, stream);
  case 3:
    return launch_v<HYBRID, LOG, 3>(P, stream);
  case 4:
    return launch_v<HYBRID, LOG, 4>(P, stream);
  case 5:
    return launch_v<HYBRID, LOG, 5>(P, stream);
  case 6:
    return launch_v<HYBRID, LOG, 6>(P, stream);
  case 7:
    return launch_v<HYBRID, LOG, 7>(P, stream);
  case 8:
    return launch_v<HYBRID, LOG, 8>(P, stream);
  default:
    return hipErrorInvalidValue;
  }
}

} // namespace

hipError_t launch_vinterp(const VinterpParams& P, hipStream_t stream)
{
  if (P.n <= 0)
    return hipSuccess;
  if (P.nlev < 2 || P.nt < 1 || P.nt > VINTERP_PASS)
    return hipErrorInvalidValue;
  if (P.hybrid)
    return P.method ? launch_nf<true, true>(P, stream) : launch_nf<true, false>(P, stream);
  return P.method ? launch_nf<false, true>(P, stream) : launch_nf<false, false>(P, stream);
}

} // namespace mifc
