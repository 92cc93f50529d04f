// mifc_vrotate.hip -- vector pairs of level batches rotated on the grid (mifc_vrotate_levels, include/mifc.h rule R;
// EXTENSION: the reference's callers rotate u, v with field algebra, six single-field calls per level).
//
// The kernel streams: 16 B per cell, level and pair (8 in, 8 out) plus the two coefficient planes once per level chunk.
// A lane owns V consecutive cells -- four through 16-byte accesses, one where a pointer or the level size is off the
// 16-byte grid -- for the levels of its workgroup's chunk: it loads cosa and sina once, tests and widens them to double
// once, then walks the levels.  Per level the address is a wave-uniform 64-bit base (field pointer + level * stride, scalar
// registers) plus the lane's cell offset.  The walk is unrolled twice with registers of their own: all loads of both levels
// and of every pair of the launch are issued before the first value is used.  The tested instances read the level's
// ALL_DEFINED bits through the scalar cache and skip the tests of a component that is flagged (wave-uniform); the untested
// ones test nothing and count nothing.  Holes are counted per pair and level by ballot + popcount, one atomic per wave and
// only where the count is not zero.  No LDS.
#include "mifc_column_walk.h"
#include "mifc_device.h"
#include "mifc_env.h"
#include "mifc_kernels.h"

#include <algorithm>
#include <type_traits>

namespace mifc {

namespace {

template <int NP, int V, bool TESTED>
__global__ __launch_bounds__(256) void vrotate_kernel(const VrotateParams P)
{
  const float undef = P.undef;
  const long first = ((long)blockIdx.x * 256 + threadIdx.x) * V;
  const int n_mine = (int)max(0L, min((long)V, (long)P.n - first)); // the lane's cells inside the launch
  const long cell = n_mine > 0 ? first : 0;                         // (a lane outside reads the first cells and throws them away)
  const bool lane0 = (threadIdx.x & 63) == 0;

  // rule R1, once per cell
  float cf[V], sf[V];
  walk_load<V>(cf, P.cosa + cell);
  walk_load<V>(sf, P.sina + cell);
  double c[V], s[V];
  bool rot_bad[V];
#pragma unroll
  for (int i = 0; i < V; ++i) {
    c[i] = (double)cf[i];
    s[i] = (double)sf[i];
    rot_bad[i] = TESTED && P.rot_all == 0 && !all_def(undef, cf[i], sf[i]);
  }

  const ConstWords lev_bits = (ConstWords)(unsigned long long)P.lev_bits;

  // U levels from level k on: every load first, then the values
  auto levels = [&](auto count, int k) {
    constexpr int U = decltype(count)::value;
    float x[U][2 * NP][V];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int f = 0; f < 2 * NP; ++f)
        walk_load<V>(x[u][f], P.fields[f] + (long)(k + u) * P.in_stride + cell); // (the level's base: wave-uniform, 64-bit)
#pragma unroll
    for (int u = 0; u < U; ++u) {
      unsigned int bits = 0;
      if constexpr (TESTED)
        bits = lev_bits[k + u];
#pragma unroll
      for (int q = 0; q < NP; ++q) {
        const bool u_all = !TESTED || ((bits >> (2 * q)) & 1u) != 0, v_all = !TESTED || ((bits >> (2 * q + 1)) & 1u) != 0; // wave-uniform
        float ru[V], rv[V];
        u64 holes = 0;
#pragma unroll
        for (int i = 0; i < V; ++i) {
          const float uf = x[u][2 * q][i], vf = x[u][2 * q + 1][i];
          // R2: each component by its own flag
          const bool u_ok = u_all || is_def(uf, undef), v_ok = v_all || is_def(vf, undef);
          const bool bad = rot_bad[i] | !u_ok | !v_ok;
          // R3: the four products are exact in double; one double rounding and one float rounding per result
          const double ud = (double)uf, vd = (double)vf;
          const double cu = c[i] * ud, sv = s[i] * vd, su = s[i] * ud, cv = c[i] * vd;
          const double a = cu - sv, b = su + cv;
          ru[i] = bad ? undef : (float)a;
          rv[i] = bad ? undef : (float)b;
          if constexpr (TESTED)
            holes += (u64)__popcll(__builtin_amdgcn_ballot_w64(bad && i < n_mine));
        }
        if constexpr (TESTED) {
          if (holes != 0 && lane0) // R4
            atomicAdd(P.n_undefined + (long)q * P.nlev + (k + u), holes);
        }
        walk_store<V>(P.out[2 * q] + (long)(k + u) * P.out_stride + cell, ru, n_mine);
        walk_store<V>(P.out[2 * q + 1] + (long)(k + u) * P.out_stride + cell, rv, n_mine);
      }
    }
  };

  const int k_begin = (int)blockIdx.y * P.chunk, k_end = min(P.nlev, k_begin + P.chunk);
  int k = k_begin;
  for (; k + VROTATE_UNROLL <= k_end; k += VROTATE_UNROLL)
    levels(std::integral_constant<int, VROTATE_UNROLL>(), k);
  for (; k < k_end; ++k)
    levels(std::integral_constant<int, 1>(), k);
}

template <int NP, int V>
hipError_t launch_tested(const VrotateParams& P, const dim3 grid, hipStream_t stream)
{
  if (P.tested)
    hipLaunchKernelGGL((vrotate_kernel<NP, V, true>), grid, dim3(256), 0, stream, P);
  else
    hipLaunchKernelGGL((vrotate_kernel<NP, V, false>), grid, dim3(256), 0, stream, P);
  return hipGetLastError();
}

template <int V>
hipError_t launch_np(const VrotateParams& P, const dim3 grid, hipStream_t stream)
{
  static_assert(VROTATE_MAX_PAIRS == 4, "one case per pair count of a launch");
  switch (P.npairs) {
  case 1:
    return launch_tested<1, V>(P, grid, stream);
  case 2:
    return launch_tested<2, V>(P, grid, stream);
  case 3:
    return launch_tested<3, V>(P, grid, stream);
  case 4:
    return launch_tested<4, V>(P, grid, stream);
  default:
    return hipErrorInvalidValue;
  }
}

} // namespace

VrotatePlan vrotate_plan(int cells, int nlev, int vec4)
{
  // Measured (profiles/README.md, "vrotate: the levels per workgroup"): chunks of four levels -- two trips of the unrolled
  // body -- were the fastest or within the spread of the fastest on every grid tried, from 90 x 45 to 1440 x 720 cells: a
  // small field needs the many workgroups, and on a large one the short workgroups still beat one long walk by 6 %, the
  // coefficients they read again (8 B per cell and chunk against 16 * npairs B per cell and level) notwithstanding.
  const int max_grid_y = 65535;
  const long per_block = 256L * (vec4 ? 4 : 1);
  const int blocks = (int)(((long)cells + per_block - 1) / per_block);
  int chunk = std::min(nlev, VROTATE_CHUNK);
  if (env().hinterp_level_chunk > 0)
    chunk = std::min(nlev, env().hinterp_level_chunk);
  chunk = std::max(chunk, (nlev + max_grid_y - 1) / max_grid_y);
  return {blocks, chunk, (nlev + chunk - 1) / chunk};
}

hipError_t launch_vrotate(const VrotateParams& prm, hipStream_t stream)
{
  if (prm.n < 1 || prm.nlev < 1 || prm.npairs < 1 || prm.npairs > VROTATE_MAX_PAIRS || (!prm.tested && !prm.rot_all))
    return hipErrorInvalidValue;
  VrotateParams P = prm;
  const VrotatePlan plan = vrotate_plan(P.n, P.nlev, P.vec4);
  P.chunk = plan.chunk;
  const dim3 grid((unsigned int)plan.blocks, (unsigned int)plan.level_chunks);
  return P.vec4 ? launch_np<4>(P, grid, stream) : launch_np<1>(P, grid, stream);
}

} // namespace mifc
