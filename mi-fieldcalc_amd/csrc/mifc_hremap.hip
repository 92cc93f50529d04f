// mifc_hremap.hip -- level batches regridded by a sparse weight table (mifc_hremap_levels, include/mifc.h; EXTENSION:
// the reference's callers apply conservative-remap weights on the host).
//
// A sparse gather with a variable number of terms per output, batched over levels.  The table is the plan's sliced-ELL
// copy (mifc_hremap_plan.h): a lane owns one destination, a wave one slice of 64, a workgroup four slices.  The wave's
// trip count is the slice's width, a scalar; per trip a lane reads ONE 8-byte (col, w) pair -- 512 contiguous bytes per
// wave -- and uses it for a register block of levels (eight, or four where the launch has more fields) and every field of
// the launch, with the sums in registers, so the table is read once per register block of levels, not once per level.
// The pair of the next trip is fetched before the values of this one.  Per level the address is a wave-uniform 64-bit
// base (field pointer + level * stride, scalar registers) plus the lane's 32-bit column.  The loads are written as
// straight-line code: padding entries carry a valid column, the predicate r < len acts on the accumulation, not on the
// load (every column is safe wherever the compiler puts a load), and a padding entry is never added as a zero.  The sums are
// sequential double sums in the table's order, every operation rounded on its own.  Stores are one dword per lane,
// consecutive lanes consecutive destinations.  No LDS.  Destinations left undef are counted per level and field by
// ballot + popcount, one atomic per wave and only where the count is not zero; the instances for
// calls whose every flag is ALL_DEFINED test nothing, count nothing and keep no Wdef or nbad.
#include "mifc_column_walk.h"
#include "mifc_device.h"
#include "mifc_env.h"
#include "mifc_kernels.h"

#include <algorithm>
#include <type_traits>

namespace mifc {

namespace {

template <int NF, bool TESTED, int MODE>
__global__ __launch_bounds__(256) void hremap_kernel(const HremapParams P)
{
  const unsigned int lane = threadIdx.x & 63u;
  const int slice = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6)));
  if (slice >= P.nslices) // (the whole wave; the kernel has no barrier)
    return;
  const unsigned int d = (unsigned int)slice * 64u + lane; // (len and wall are padded to whole slices)
  const bool mine = d < (unsigned int)P.ndst;
  const bool lane0 = lane == 0;
  const int len = P.len[d];
  const double wall = P.wall[d];
  // (the slice's scalars through the constant address space, like the level words: scalar loads)
  const int width = (int)((ConstWords)(unsigned long long)P.slice_width)[slice];
  const u64 first = ((const __attribute__((address_space(4))) u64*)(unsigned long long)P.slice_off)[slice];
  const int2* ent = static_cast<const int2*>(P.entries) + first + lane;
  const float undef = P.undef;
  const ConstWords lev_bits = (ConstWords)(unsigned long long)P.lev_bits;

  // U levels from level k of the launch on
  auto levels = [&](auto count, int k) {
    constexpr int U = decltype(count)::value;
    double S[U][NF], Wdef[U][NF];
    int nbad[U][NF];
    unsigned int bits[U]; // bit f: field f of the launch is flagged ALL_DEFINED at the level (wave-uniform)
    long level[U];        // the level's offset from the field pointers (wave-uniform, 64-bit)
#pragma unroll
    for (int u = 0; u < U; ++u) {
      bits[u] = 0;
      if constexpr (TESTED)
        bits[u] = lev_bits[P.lev0 + k + u] >> P.f0;
      level[u] = (long)(k + u) * P.in_stride;
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        S[u][f] = 0.0;
        Wdef[u][f] = 0.0;
        nbad[u][f] = 0;
      }
    }
    if (width > 0) {
      int2 next = ent[0];
      for (int r = 0; r < width; ++r) {
        const int2 e = next;
        next = ent[(long)min(r + 1, width - 1) * 64];
        const int col = e.x;
        const double wd = (double)__int_as_float(e.y);
        const bool active = r < len;
        // The tested instances keep U * NF level pointers and as many lane masks of the flags in scalar registers if the
        // compiler may hoist them out of the trip loop, and spill them; a zero it cannot see through keeps the pointer
        // sums and the flag tests inside the loop, where they are scalar instructions beside the double adds.
        long zero = 0;
        if constexpr (TESTED)
          asm volatile("" : "+s"(zero));
        float x[U][NF];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int f = 0; f < NF; ++f)
            x[u][f] = (P.fields[f] + (level[u] + zero))[col];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if constexpr (TESTED) // (one level's lane masks at a time: scheduled across the levels they do not fit the scalar registers)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int f = 0; f < NF; ++f) {
            bool use = active;
            if constexpr (TESTED) {
              const bool all = (((bits[u] | (unsigned int)zero) >> f) & 1u) != 0;
              const bool def = all || is_def(x[u][f], undef);
              use = active & def;
              nbad[u][f] += (active & !def) ? 1 : 0;
              const double wsum = Wdef[u][f] + wd;
              Wdef[u][f] = use ? wsum : Wdef[u][f];
            }
            const double prod = wd * (double)x[u][f]; // exact: 24 x 24 bits
            const double sum = S[u][f] + prod;
            S[u][f] = use ? sum : S[u][f];
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kc = P.lev0 + k + u; // the call's level
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        bool hole = len == 0;
        float res = (float)S[u][f];
        if constexpr (TESTED) {
          const bool some_bad = nbad[u][f] > 0;
          if constexpr (MODE == HREMAP_STRICT) {
            hole |= some_bad;
          } else {
            if (__builtin_amdgcn_ballot_w64(some_bad) != 0) {
              const double wdef = Wdef[u][f];
              const double need = P.min_frac * __builtin_fabs(wall);
              const bool lost = nbad[u][f] == len || wdef == 0.0 || !(__builtin_fabs(wdef) >= need);
              const double q = S[u][f] / wdef;
              const float renorm = (float)(q * wall);
              hole |= some_bad & lost;
              res = some_bad ? renorm : res;
            }
          }
          const u64 m = __builtin_amdgcn_ballot_w64(mine && len > 0 && hole);
          if (m != 0 && lane0)
            atomicAdd(P.n_undefined + (long)(P.f0 + f) * P.call_nlev + kc, (u64)__popcll(m));
        }
        if (mine)
          (P.out[f] + (long)(k + u) * P.out_stride)[d] = hole ? undef : res;
      }
    }
  };

  const int k_begin = (int)blockIdx.y * P.chunk, k_end = min(P.nlev, k_begin + P.chunk);
  constexpr int BLOCK = hremap_levels(NF, TESTED);
  static_assert((BLOCK == HREMAP_LEVELS || BLOCK == 2 * HREMAP_LEVELS) && HREMAP_LEVELS == 4, "a block, half a block, one body per remainder");
  int k = k_begin;
  for (; k + BLOCK <= k_end; k += BLOCK)
    levels(std::integral_constant<int, BLOCK>(), k);
  if constexpr (BLOCK > HREMAP_LEVELS)
    if (k + HREMAP_LEVELS <= k_end) {
      levels(std::integral_constant<int, HREMAP_LEVELS>(), k);
      k += HREMAP_LEVELS;
    }
  switch (k_end - k) {
  case 3:
    levels(std::integral_constant<int, 3>(), k);
    break;
  case 2:
    levels(std::integral_constant<int, 2>(), k);
    break;
  case 1:
    levels(std::integral_constant<int, 1>(), k);
    break;
  default:
    break;
  }
}

template <int NF>
hipError_t launch_mode(const HremapParams& P, hipStream_t stream)
{
  const dim3 grid((unsigned int)((P.nslices + 3) / 4), (unsigned int)((P.nlev + P.chunk - 1) / P.chunk)), block(256);
  if (!P.tested) { // (both modes are one rule where nothing is tested)
    hipLaunchKernelGGL((hremap_kernel<NF, false, HREMAP_STRICT>), grid, block, 0, stream, P);
  } else if constexpr (NF <= HREMAP_PASS_TESTED) { // (the instances beyond a launch's capacity do not exist)
    if (P.mode == HREMAP_STRICT)
      hipLaunchKernelGGL((hremap_kernel<NF, true, HREMAP_STRICT>), grid, block, 0, stream, P);
    else
      hipLaunchKernelGGL((hremap_kernel<NF, true, HREMAP_RENORM>), grid, block, 0, stream, P);
  } else {
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

} // namespace

HremapShape hremap_shape(int nslices, int nlev, int nfields, bool tested)
{
  // Measured (profiles/hremap.txt): one register block per workgroup wherever that fills the device -- the tables are
  // then read once per chunk, and longer chunks gain nothing --; with few destinations the call is bound by the gathers
  // each CU can keep in flight, and its time falls in proportion to the chunk down to one level per workgroup.  So:
  // the target of hinterp_plan, eight workgroups per CU, with the register block as the longest chunk.
  const int wanted_workgroups = 8 * 256, max_grid_y = 65535;
  const int block = hremap_levels(nfields, tested);
  const int blocks = (nslices + 3) / 4;
  const int wanted = std::min(nlev, std::max(1, (wanted_workgroups + blocks - 1) / blocks)); // level chunks
  int chunk = std::min(nlev / wanted, block);
  if (chunk > HREMAP_LEVELS && chunk < block) // (between the two block sizes: a whole small block)
    chunk = HREMAP_LEVELS;
  if (env().hremap_level_chunk > 0)
    chunk = std::min(nlev, env().hremap_level_chunk);
  chunk = std::max(chunk, (nlev + max_grid_y - 1) / max_grid_y);
  return {blocks, chunk, (nlev + chunk - 1) / chunk};
}

hipError_t launch_hremap(const HremapParams& prm, hipStream_t stream)
{
  if (prm.ndst < 1 || prm.nslices != (prm.ndst + 63) / 64 || prm.nlev < 1 || prm.f0 < 0 || prm.f0 + prm.nfields > HREMAP_MAX_FIELDS ||
      prm.lev0 < 0 || prm.lev0 + prm.nlev > prm.call_nlev || (prm.mode != HREMAP_STRICT && prm.mode != HREMAP_RENORM) || prm.chunk < 1 ||
      (prm.nlev + prm.chunk - 1) / prm.chunk > 65535)
    return hipErrorInvalidValue;
  const HremapParams& P = prm;
  static_assert(HREMAP_PASS == 4 && HREMAP_PASS_TESTED <= HREMAP_PASS, "one case per field count of a launch");
  switch (P.nfields) {
  case 1:
    return launch_mode<1>(P, stream);
  case 2:
    return launch_mode<2>(P, stream);
  case 3:
    return launch_mode<3>(P, stream);
  case 4:
    return launch_mode<4>(P, stream);
  default:
    return hipErrorInvalidValue;
  }
}

} // namespace mifc
