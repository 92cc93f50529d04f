// mifc_column_walk.h -- what the kernels that walk the levels of a column have in common (mifc_vinterp.hip,
// mifc_vlayer.hip, mifc_vderiv.hip, mifc_vcumul.hip, mifc_vparcel.hip, mifc_pvort.hip): a lane owns V consecutive cells (four through 16-byte accesses, or one where the
// batch is off the 16-byte grid) and keeps them for all levels, in level slots that rotate.  Device code only.
#ifndef MIFC_COLUMN_WALK_H
#define MIFC_COLUMN_WALK_H

#include "mifc_kernels.h"

#include <hip/hip_runtime.h>

namespace mifc {

namespace {

// The per-level scalars are written before the launch and only read by the kernel.  Read through the constant address
// space they come through the scalar cache; as plain global loads the compiler has to assume that the kernel's own stores
// may have changed them and fetches them per lane, in the queue of the field loads.
typedef const __attribute__((address_space(4))) float* ConstFloats;
typedef const __attribute__((address_space(4))) unsigned int* ConstWords;
typedef const __attribute__((address_space(4))) double* ConstDoubles;

template <int V>
__device__ __forceinline__ void walk_load(float (&r)[V], const float* p)
{
  if constexpr (V == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    r[0] = q.x;
    r[1] = q.y;
    r[2] = q.z;
    r[3] = q.w;
  } else {
    r[0] = p[0];
  }
}

// the first n_mine cells of a lane (the ones inside the launch): one 16-byte store where that is all four
template <int V>
__device__ __forceinline__ void walk_store(float* p, const float (&r)[V], int n_mine)
{
  if constexpr (V == 4) {
    if (n_mine == 4) {
      *reinterpret_cast<float4*>(p) = make_float4(r[0], r[1], r[2], r[3]);
      return;
    }
  }
#pragma unroll
  for (int c = 0; c < V; ++c)
    if (c < n_mine)
      p[c] = r[c];
}

// A body that runs for a few of the levels only still has everything in it that depends on the level alone (conversions
// to double, defined tests, logarithms) hoisted by the compiler, which computes it for EVERY level and keeps it in
// registers (measured in mifc_vinterp.hip: 32 VGPRs per field instead of 12, hundreds of SGPR spills).  Passing a value
// through one of these makes it opaque where it is used.
__device__ __forceinline__ float walk_here(float x)
{
  asm volatile("" : "+v"(x));
  return x;
}
// a per-lane word: it is kept in a VGPR instead of being recomputed from lane masks
__device__ __forceinline__ unsigned int walk_here_v(unsigned int x)
{
  asm volatile("" : "+v"(x));
  return x;
}
// a wave-uniform index: output pointers, product slots and the like are fetched from the kernel arguments where they are
// used instead of sitting in SGPRs through the walk
__device__ __forceinline__ int walk_here(int uniform)
{
  asm volatile("" : "+s"(uniform));
  return uniform;
}

// one level of the lane's cells
template <int NF, int V>
struct WalkLevel
{
  float c[V]; // field coordinate: as loaded
  float x[NF][V];
};

// The coordinate of a level in the lane's cells, with "not usable" carried as NaN (a NaN never brackets, differs from
// everything and fails every ordered compare, so no flag per cell has to live through the walk).  KIND: VDERIV_HYBRID =
// alevel + blevel * ps, VDERIV_FIELD = a batch like the fields, VDERIV_LEVELS = one number per level, nothing per cell.
// walk_usable_ps: ps as loaded -> ps for walk_coordinate (an undefined ps: every level of the cell is not usable).
template <int V>
__device__ __forceinline__ void walk_usable_ps(float (&ps)[V], bool ps_all, float undef)
{
  const float nan = __int_as_float(0x7fc00000);
#pragma unroll
  for (int c = 0; c < V; ++c) {
    const float p = ps[c]; // (read first: the test below then selects, it does not branch around a load)
    ps[c] = (ps_all || p != undef) ? p : nan;
  }
}
// level k: `lc` = the coordinate field's cells as loaded (VDERIV_FIELD), `bits` = the level's word of the table
template <int KIND, int V>
__device__ __forceinline__ void walk_coordinate(float (&cc)[V], const float (&lc)[V], const float (&ps)[V], ConstFloats ab, int nlev, int k, unsigned int bits,
                                                float undef)
{
  if constexpr (KIND == VDERIV_HYBRID) {
    const float a = ab[k], b = ab[nlev + k];
#pragma unroll
    for (int c = 0; c < V; ++c) {
      const float prod = b * ps[c]; // p_hlevel, FieldCalculations.cc:303: the product rounded, then the sum
      cc[c] = a + prod;
    }
  } else if constexpr (KIND == VDERIV_FIELD) {
    const float nan = __int_as_float(0x7fc00000);
    const bool all = ((bits >> VINTERP_COORD_BIT) & 1u) != 0;
#pragma unroll
    for (int c = 0; c < V; ++c) {
      const float x = lc[c]; // (read first, as in walk_usable_ps)
      cc[c] = (all || x != undef) ? x : nan;
    }
  } else {
#pragma unroll
    for (int c = 0; c < V; ++c)
      cc[c] = 0.f; // not used: the table says which sides exist
  }
}

} // namespace

} // namespace mifc

#endif // MIFC_COLUMN_WALK_H
