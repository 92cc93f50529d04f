// mifc_vregrid.hip -- level batches interpolated to per-cell target surfaces (mifc_vregrid_hlevels / _fields / _levels,
// include/mifc.h; EXTENSION: the reference has no function that crosses levels).
//
// The walk is that of mifc_vinterp.hip: consecutive lanes own consecutive cells, four each through 16-byte loads (V = 4)
// or one each (V = 1), level k's coordinate and NF field values stay in registers, the next levels are loaded two pairs
// ahead of use in three slots that rotate.  What differs is where the targets live: they are per cell, so a lane keeps
// the targets of a pass (`tb` at most) for its own cells -- in LDS, each lane reading only what it wrote itself, which leaves the
// registers to the level slots and lets the loop over the targets be a loop (a register array could only be indexed by
// unrolling the body tb times, in each of the three slots).  A found-mask per cell (one bit per target, hence tb <= 32)
// marks the targets that are done with.  vinterp's scalar-key ballot does not carry over; its replacement is one
// wave-uniform interval: the wave reduces [min, max] of its usable targets once per pass, and a level pair whose own
// wave interval does not meet it is skipped whole -- for a model-to-model pass that is most pairs.  Direction and
// `outside` are wave-uniform runtime values: FROM_LAST walks k descending and orients the pair (k, k + 1) by a select.
// For OUTSIDE_CLAMP a cell carries the two extreme coordinates and their levels (mifc_vregrid_rules.h), not the values;
// those are fetched behind the walk for the cells that need them, where the targets never found are stored.  Undefined
// results are counted per wave by ballot into a table in LDS and leave the workgroup as one atomic per (field, target)
// that has something to count.
#include <hip/hip_runtime.h>
#define MIFC_VREGRID_FN __host__ __device__ __forceinline__
#include "mifc_column_walk.h"
#include "mifc_device.h"
#include "mifc_kernels.h"
#include "mifc_vregrid_rules.h"

namespace mifc {

namespace {

// the cells of a lane that `m` marks (all of them inside the launch): one 16-byte store where that is all four
template <int V>
__device__ __forceinline__ void vr_store(float* p, const float (&r)[V], const bool (&m)[V])
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
__device__ __forceinline__ float vr_wave_min(float x)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    x = fminf(x, __shfl_xor(x, off, 64));
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}
__device__ __forceinline__ float vr_wave_max(float x)
{
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
    x = fmaxf(x, __shfl_xor(x, off, 64));
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x)));
}

// the lane's own targets in LDS: slot t of lane `lane` at (t * 256 + lane) * V
template <int V>
__device__ __forceinline__ void vr_targets_put(float* s, int t, const float (&ct)[V])
{
  float* p = s + ((long)t * 256 + threadIdx.x) * V;
  if constexpr (V == 4)
    *reinterpret_cast<float4*>(p) = make_float4(ct[0], ct[1], ct[2], ct[3]);
  else
    p[0] = ct[0];
}
template <int V>
__device__ __forceinline__ void vr_targets_get(const float* s, int t, float (&ct)[V])
{
  walk_load<V>(ct, s + ((long)t * 256 + threadIdx.x) * V);
}

template <bool HYBRID, bool LOG, int NF, int V>
__global__ __launch_bounds__(256) void vregrid_kernel(const VregridParams P)
{
  constexpr int R = 3; // level slots
  extern __shared__ __align__(16) float s_tc[];
  __shared__ unsigned int s_bad[NF * VREGRID_MAX_TB];
  for (int j = threadIdx.x; j < NF * VREGRID_MAX_TB; j += 256)
    s_bad[j] = 0;
  __syncthreads();

  const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * V;
  const long left = (long)P.n - i0;
  const int n_mine = left < 0 ? 0 : (left < V ? (int)left : V); // this lane's cells inside the launch: cells 0 .. n_mine - 1
  const long at = n_mine > 0 ? i0 : 0; // lanes past the end walk column group 0 and neither store nor count
  const float undef = P.undef;
  const int nlev = P.nlev, nt = P.nt;
  const bool last = P.from != VREGRID_FROM_FIRST, clamp = P.outside != VREGRID_OUTSIDE_UNDEF; // wave-uniform
  const float inf = __int_as_float(0x7f800000), nan = __int_as_float(0x7fc00000);
  // the per-level scalars through the scalar cache (mifc_column_walk.h)
  const ConstFloats ab = (ConstFloats)(unsigned long long)P.ab;
  const ConstWords lev_bits = (ConstWords)(unsigned long long)P.lev_bits;

  // step s of the walk is level s, or level nlev - 1 - s against the index order
  auto level_of = [&](int s) { return last ? nlev - 1 - s : s; };
  auto load = [&](WalkLevel<NF, V>& L, int s) {
    const long off = (long)level_of(s) * P.in_stride + at;
    if constexpr (!HYBRID)
      walk_load<V>(L.c, P.coord + off);
#pragma unroll
    for (int f = 0; f < NF; ++f)
      walk_load<V>(L.x[f], P.fields[f] + off);
  };
  WalkLevel<NF, V> L[R];
  load(L[0], 0);
  load(L[1], 1);
  if (2 < nlev)
    load(L[2], 2);

  // rule 2: the targets of the pass, not usable = NaN, into the lane's slots; the wave's interval of the usable ones
  float lane_tmin = inf, lane_tmax = -inf;
#pragma unroll 1
  for (int t = 0; t < nt; ++t) {
    float ct[V];
    walk_load<V>(ct, P.tcoord + (long)(P.t0 + t) * P.in_stride + at);
    const bool all = ((P.tc_all >> t) & 1u) != 0;
#pragma unroll
    for (int c = 0; c < V; ++c) {
      ct[c] = c < n_mine ? vregrid_target(ct[c], all, undef, LOG) : nan;
      lane_tmin = fminf(lane_tmin, ct[c]); // (fminf / fmaxf pass a NaN by)
      lane_tmax = fmaxf(lane_tmax, ct[c]);
    }
    vr_targets_put<V>(s_tc, t, ct);
  }
  const float wave_tmin = vr_wave_min(lane_tmin), wave_tmax = vr_wave_max(lane_tmax);

  // An undefined coordinate is carried as NaN (mifc_column_walk.h): it never brackets and is never an extreme.
  float ps[V];
  if constexpr (HYBRID) {
    if (P.no_ps) {
#pragma unroll
      for (int c = 0; c < V; ++c)
        ps[c] = -0.f; // the `levels` form: a = levels[k], b = +0; 0 * -0 = -0 and a + -0 is a bit for bit, a level of -0 too (a + +0 made it +0)
    } else {
      walk_load<V>(ps, P.coord + at);
      walk_usable_ps<V>(ps, P.ps_all != 0, undef);
    }
  }
  auto coordinate = [&](const WalkLevel<NF, V>& Lv, int k, unsigned int bits, float (&cc)[V]) {
    walk_coordinate<HYBRID ? VDERIV_HYBRID : VDERIV_FIELD, V>(cc, Lv.c, ps, ab, nlev, k, bits, undef);
  };
  VregridExtremes ext[V];
#pragma unroll
  for (int c = 0; c < V; ++c)
    vregrid_extremes_start(ext[c]);
  auto extremes = [&](const float (&cc)[V], int k) {
    if (clamp) {
#pragma unroll
      for (int c = 0; c < V; ++c)
        vregrid_extremes_level(ext[c], cc[c], k, last);
    }
  };

  unsigned int bits_s = lev_bits[level_of(0)];
  float cs[V]; // the coordinate of step s, cs1 below that of step s + 1
  coordinate(L[0], level_of(0), bits_s, cs);
  extremes(cs, level_of(0));
  unsigned int found[V]; // bit t: target t of the pass is done with (cells outside the launch and targets past nt: from the start)
#pragma unroll
  for (int c = 0; c < V; ++c)
    found[c] = c < n_mine ? (nt >= 32 ? 0u : ~((1u << nt) - 1u)) : 0xffffffffu;

  for (int s0 = 0; s0 < nlev - 1; s0 += R) {
#pragma unroll
    for (int d = 0; d < R; ++d) {
      const int s = s0 + d; // the steps s and s + 1: the pair (k, k + 1) with k the smaller of their levels
      if (s < nlev - 1) {
        WalkLevel<NF, V>& cur = L[d];
        WalkLevel<NF, V>& nx = L[(d + 1) % R];
        const int k1 = level_of(s + 1);
        const unsigned int bits_s1 = lev_bits[k1];
        float cs1[V], lo[V], hi[V];
        coordinate(nx, k1, bits_s1, cs1);
        extremes(cs1, k1);
        float lane_lo = inf, lane_hi = -inf;
#pragma unroll
        for (int c = 0; c < V; ++c) {
          const bool pair = !__builtin_isunordered(cs[c], cs1[c]);
          lo[c] = pair ? fminf(cs[c], cs1[c]) : inf;
          hi[c] = pair ? fmaxf(cs[c], cs1[c]) : -inf;
          lane_lo = fminf(lane_lo, lo[c]);
          lane_hi = fmaxf(lane_hi, hi[c]);
        }
        // the wave's pairs against the wave's targets: most pairs of a pass meet none of them
        const float wave_lo = vr_wave_min(lane_lo), wave_hi = vr_wave_max(lane_hi);
        if (wave_lo <= wave_tmax && wave_hi >= wave_tmin) {
#pragma unroll 1
          for (int t = 0; t < nt; ++t) { // wave-uniform
            float ct[V];
            vr_targets_get<V>(s_tc, t, ct);
            // per cell, as bits of one register (1: this target is found here, 2: c_k == c_k+1, 4: LOG of a coordinate <= 0),
            // as in mifc_vinterp.hip
            unsigned int state[V];
            bool any = false;
#pragma unroll
            for (int c = 0; c < V; ++c) {
              const bool hit = ((found[c] >> t) & 1u) == 0 && lo[c] <= ct[c] && ct[c] <= hi[c];
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
              const float ca = walk_here(cs[c]), cb = walk_here(cs1[c]);
              const float c0 = last ? cb : ca, c1 = last ? ca : cb; // the pair is (k, k + 1) whichever way the walk goes
              state[c] |= c0 == c1 ? 2u : 0u;
              if constexpr (LOG)
                state[c] |= !(fminf(c0, c1) > 0.f) ? 4u : 0u;
              w[c] = vregrid_weight<LOG>(c0, c1, ct[c]);
              state[c] = walk_here_v(state[c]);
            }
            const unsigned int here_s = (unsigned int)walk_here((int)bits_s), here_s1 = (unsigned int)walk_here((int)bits_s1);
            const unsigned int here_k = last ? here_s1 : here_s, here_k1 = last ? here_s : here_s1;
#pragma unroll
            for (int f = 0; f < NF; ++f) {
              const bool all_k = ((here_k >> f) & 1u) != 0, all_k1 = ((here_k1 >> f) & 1u) != 0;
              float r[V];
              bool hit[V];
              unsigned int n = 0;
#pragma unroll
              for (int c = 0; c < V; ++c) {
                const float xa = walk_here(cur.x[f][c]), xb = walk_here(nx.x[f][c]);
                const float xk = last ? xb : xa, xk1 = last ? xa : xb;
                const bool ok = (all_k || is_def(xk, undef)) && (all_k1 || is_def(xk1, undef)) && (state[c] & 4u) == 0;
                const float v = vregrid_value(w[c], xk, xk1);
                r[c] = ok ? ((state[c] & 2u) != 0 ? xk : v) : undef;
                hit[c] = (state[c] & 1u) != 0;
                n += (unsigned int)__popcll(__builtin_amdgcn_ballot_w64(hit[c] && !ok)); // the whole wave is here
              }
              vr_store<V>(P.out[walk_here(f)] + (long)(P.t0 + t) * P.out_stride + i0, r, hit);
              if (n != 0 && (threadIdx.x & 63) == 0)
                atomicAdd(&s_bad[f * VREGRID_MAX_TB + t], n);
            }
          }
        }
        // step s + 1 becomes step s; the slot of step s takes step s + 3
        bits_s = bits_s1;
#pragma unroll
        for (int c = 0; c < V; ++c)
          cs[c] = cs1[c];
        if (s + R < nlev)
          load(cur, s + R);
      }
    }
  }

  // the targets without a bracket: undef in every field, or (OUTSIDE_CLAMP, beyond the extremes) the value at kmin / kmax
#pragma unroll 1
  for (int t = 0; t < nt; ++t) { // wave-uniform
    bool miss[V], any = false;
#pragma unroll
    for (int c = 0; c < V; ++c) {
      miss[c] = ((found[c] >> t) & 1u) == 0;
      any |= miss[c];
    }
    if (__builtin_amdgcn_ballot_w64(any) == 0)
      continue;
    float ct[V];
    vr_targets_get<V>(s_tc, t, ct);
    int ksel[V];
#pragma unroll
    for (int c = 0; c < V; ++c)
      ksel[c] = (clamp && miss[c]) ? vregrid_clamp_level(ext[c], ct[c]) : -1; // a missing cell is inside the launch
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      float r[V];
      unsigned int n = 0;
#pragma unroll
      for (int c = 0; c < V; ++c) {
        float x = undef;
        unsigned int b = 0;
        if (ksel[c] >= 0) { // 0 <= ksel < nlev, the lane's own cell: the values were not carried, they are fetched here
          x = P.fields[f][(long)ksel[c] * P.in_stride + i0 + c];
          b = P.lev_bits[ksel[c]];
        }
        const bool ok = ksel[c] >= 0 && (((b >> f) & 1u) != 0 || is_def(x, undef));
        r[c] = ok ? x : undef; // copied bit for bit, no arithmetic
        n += (unsigned int)__popcll(__builtin_amdgcn_ballot_w64(miss[c] && !ok));
      }
      vr_store<V>(P.out[walk_here(f)] + (long)(P.t0 + t) * P.out_stride + i0, r, miss);
      if (n != 0 && (threadIdx.x & 63) == 0)
        atomicAdd(&s_bad[f * VREGRID_MAX_TB + t], n);
    }
  }

  __syncthreads();
  for (int j = threadIdx.x; j < NF * VREGRID_MAX_TB; j += 256) {
    const int f = j / VREGRID_MAX_TB, t = j % VREGRID_MAX_TB;
    if (t < nt && s_bad[j] != 0)
      atomicAdd(P.n_undefined + (long)f * P.nt_call + P.t0 + t, (u64)s_bad[j]);
  }
}

template <bool HYBRID, bool LOG, int NF>
hipError_t launch_v(const VregridParams& P, hipStream_t stream)
{
  const int v = P.vec4 ? 4 : 1, per_block = 256 * v;
  const dim3 grid((unsigned int)(((long)P.n + per_block - 1) / per_block)), block(256);
  const size_t lds = (size_t)P.nt * 256 * (size_t)v * sizeof(float); // the slots of this pass' targets: a short pass leaves the LDS to more workgroups
  if (P.vec4)
    hipLaunchKernelGGL((vregrid_kernel<HYBRID, LOG, NF, 4>), grid, block, lds, stream, P);
  else
    hipLaunchKernelGGL((vregrid_kernel<HYBRID, LOG, NF, 1>), grid, block, lds, stream, P);
  return hipGetLastError();
}

template <bool HYBRID, bool LOG>
hipError_t launch_nf(const VregridParams& P, hipStream_t stream)
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

hipError_t launch_vregrid(const VregridParams& P, hipStream_t stream)
{
  if (P.n <= 0)
    return hipSuccess;
  if (P.nlev < 2 || P.nt < 1 || P.nt > P.tb || P.tb > VREGRID_MAX_TB || (size_t)P.tb * 256 * (P.vec4 ? 4 : 1) * sizeof(float) > (size_t)VREGRID_MAX_LDS)
    return hipErrorInvalidValue;
  if (P.hybrid)
    return P.method ? launch_nf<true, true>(P, stream) : launch_nf<true, false>(P, stream);
  return P.method ? launch_nf<false, true>(P, stream) : launch_nf<false, false>(P, stream);
}

} // namespace mifc
