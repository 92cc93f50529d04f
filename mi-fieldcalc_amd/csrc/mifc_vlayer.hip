// mifc_vlayer.hip -- layer integrals, means and extremes of level batches (mifc_vlayer_hlevels / mifc_vlayer_fields,
// include/mifc.h; EXTENSION: the reference has no function that crosses levels).
//
// The walk is the one of mifc_vinterp.hip: consecutive lanes own consecutive cells, four each through 16-byte loads
// (V = 4) or one each (V = 1), a lane keeps its cells for all levels, level k + 1 is loaded two pairs ahead of use (three
// level slots that rotate, the k loop unrolled three times so that the slots are static), the per-level scalars come
// from a small table through the constant address space.  What differs is what a pair (k, k + 1) does: it is clipped to
// the cell's layer [L, H], and where a piece is left the trapezoid goes to the double accumulators (G & VLAYER_SUMS) and
// the two end values to the running extremes (G & VLAYER_EXTREMES).  Two things keep that cheap: a pair in which no cell
// of the wave takes part is skipped by one ballot (everything above and below the layer), and the interpolation to a
// bound -- two double divisions per cell -- is only compiled into a second body that a wave enters when one of its cells
// has a bound strictly inside the pair; everywhere else the ends ARE the two levels.  Nothing is stored before the end
// of the walk: per cell and field one double and four floats, per cell the extent, the bounds and a word of bits (bit f:
// field f has a hole in the layer; CELL_BAD: coordinate or bounds unusable; CELL_ANY: a pair took part).  Undefined
// cells are counted per wave by ballot into LDS and leave the workgroup as one atomic per field.
#include "mifc_column_walk.h"
#include "mifc_device.h"
#include "mifc_kernels.h"

namespace mifc {

namespace {

const unsigned int CELL_BAD = 1u << 31, CELL_ANY = 1u << 30;

// what a cell carries through the walk
template <int G, int NF, int V>
struct LayerState
{
  double ext[V];
  double acc[(G & VLAYER_SUMS) ? NF : 1][V];
  float mx[(G & VLAYER_EXTREMES) ? NF : 1][V], mn[(G & VLAYER_EXTREMES) ? NF : 1][V];
  float cmx[(G & VLAYER_EXTREMES) ? NF : 1][V], cmn[(G & VLAYER_EXTREMES) ? NF : 1][V];
  unsigned int bits[V];
};

// One candidate (value, coordinate) of the extremes: the first one of the cell initialises both, a later one replaces
// the maximum on > and the minimum on < (so the first occurrence wins and a NaN that came first stays).
__device__ __forceinline__ void vl_candidate(bool part, bool first, float v, float e, float& mx, float& cmx, float& mn, float& cmn)
{
  const bool up = part & (first | (v > mx)), down = part & (first | (v < mn));
  mx = up ? v : mx;
  cmx = up ? e : cmx;
  mn = down ? v : mn;
  cmn = down ? e : cmn;
}

// The pair (k, k + 1) for the lane's V cells.  CLIPPED = false: every cell that takes part does so with both ends on
// the levels themselves (a = min, b = max of the two coordinates), so v_a + v_b is x_k + x_k+1 and the candidates are
// the level values; CLIPPED = true: the general form of rule 5.
template <bool CLIPPED, int G, int NF, int V>
__device__ __forceinline__ void vl_pair(LayerState<G, NF, V>& S, const WalkLevel<NF, V>& cur, const WalkLevel<NF, V>& nx, const float (&ck)[V],
                                        const float (&ck1)[V], const float (&a)[V], const float (&b)[V], const bool (&part)[V], unsigned int all_k,
                                        unsigned int all_k1, float undef)
{
  double d[V], wa[V], wb[V];
  bool first[V];
#pragma unroll
  for (int c = 0; c < V; ++c) {
    d[c] = (double)b[c] - (double)a[c];
    S.ext[c] = part[c] ? S.ext[c] + d[c] : S.ext[c];
    first[c] = (S.bits[c] & CELL_ANY) == 0;
    if constexpr (CLIPPED) {
      const double c0 = (double)ck[c], span = (double)ck1[c] - c0;
      wa[c] = ((double)a[c] - c0) / span;
      wb[c] = ((double)b[c] - c0) / span;
    }
  }
#pragma unroll
  for (int f = 0; f < NF; ++f) {
#pragma unroll
    for (int c = 0; c < V; ++c) {
      const float xk = cur.x[f][c], xk1 = nx.x[f][c];
      const bool ok_k = ((all_k >> f) & 1u) != 0 || is_def(xk, undef), ok_k1 = ((all_k1 >> f) & 1u) != 0 || is_def(xk1, undef);
      const bool ok = ok_k && ok_k1;
      S.bits[c] |= (part[c] & !ok) ? (1u << f) : 0u;
      const double dk = (double)xk, dk1 = (double)xk1;
      double va, vb; // the values at the ends a and b
      float near_v, far_v, near_e, far_e; // the end nearer level k first
      if constexpr (CLIPPED) {
        const double diff = dk1 - dk;
        const double pa = wa[c] * diff, pb = wb[c] * diff;
        const double ia = dk + pa, ib = dk + pb;
        // (compared again for every field: hoisted out of the field loop these five tests per cell are forty SGPRs of
        // lane masks that live through it, more than the wave has to spare)
        const float ea = walk_here(a[c]), eb = walk_here(b[c]), c0 = walk_here(ck[c]), c1 = walk_here(ck1[c]);
        va = ea == c0 ? dk : (ea == c1 ? dk1 : ia);
        vb = eb == c0 ? dk : (eb == c1 ? dk1 : ib);
        const bool rising = c0 <= c1; // a is the end at level k's side
        near_v = (float)(rising ? va : vb);
        far_v = (float)(rising ? vb : va);
        near_e = rising ? ea : eb;
        far_e = rising ? eb : ea;
      } else {
        va = dk; // (in either order: the sum below is commutative)
        vb = dk1;
        near_v = xk;
        far_v = xk1;
        near_e = ck[c];
        far_e = ck1[c];
      }
      if constexpr ((G & VLAYER_SUMS) != 0) {
        const double sum = va + vb;
        const double half = sum * 0.5;
        const double term = half * d[c];
        S.acc[f][c] = part[c] ? S.acc[f][c] + term : S.acc[f][c];
      }
      if constexpr ((G & VLAYER_EXTREMES) != 0) {
        vl_candidate(part[c], first[c], near_v, near_e, S.mx[f][c], S.cmx[f][c], S.mn[f][c], S.cmn[f][c]);
        vl_candidate(part[c], false, far_v, far_e, S.mx[f][c], S.cmx[f][c], S.mn[f][c], S.cmn[f][c]);
      }
    }
  }
#pragma unroll
  for (int c = 0; c < V; ++c)
    S.bits[c] |= part[c] ? CELL_ANY : 0u;
}

template <bool HYBRID, int G, int NF, int V>
__global__ __launch_bounds__(256, 2) void vlayer_kernel(const VlayerParams P)
{
  constexpr int R = 3; // level slots
  __shared__ unsigned int s_bad[NF];
  if (threadIdx.x < NF)
    s_bad[threadIdx.x] = 0;
  __syncthreads();

  const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * V;
  const long left = (long)P.n - i0;
  const int n_mine = left < 0 ? 0 : (left < V ? (int)left : V); // this lane's cells inside the launch: cells 0 .. n_mine - 1
  // Addresses are a wave-uniform base (array + level + the workgroup's first cell, computed in SGPRs where it is used) plus
  // the lane's 32-bit byte offset inside the workgroup: one VGPR for all loads, instead of an induction pointer in a VGPR
  // or SGPR pair per field and level slot.  Lanes past the end walk the workgroup's first column group and neither store
  // nor count (a workgroup has at least one cell).
  const long block0 = (long)blockIdx.x * (256 * V);
  const unsigned int lane_bytes = n_mine > 0 ? threadIdx.x * (unsigned int)(V * sizeof(float)) : 0u;
  auto lane_of = [&](const float* uniform_base) { return reinterpret_cast<const float*>(reinterpret_cast<const char*>(uniform_base) + lane_bytes); };
  const float undef = P.undef;
  const int nlev = P.nlev, f0 = P.f0;
  // the per-level scalars through the scalar cache (mifc_column_walk.h)
  const ConstFloats ab = (ConstFloats)(unsigned long long)P.ab;
  const ConstWords lev_bits = (ConstWords)(unsigned long long)P.lev_bits;

  auto load = [&](WalkLevel<NF, V>& L, int k) {
    const long off = (long)walk_here(k) * P.in_stride + block0; // (k opaque: no induction variable per pointer)
    if constexpr (!HYBRID)
      walk_load<V>(L.c, lane_of(P.coord + off));
#pragma unroll
    for (int f = 0; f < NF; ++f)
      walk_load<V>(L.x[f], lane_of(P.fields[f] + off));
  };

  // an undefined coordinate is carried as NaN: it makes the cell undefined like a NaN that came in as a value (rule 1)
  float ps[V];
  if constexpr (HYBRID) {
    walk_load<V>(ps, lane_of(P.coord + block0));
    // (walk_usable_ps, written out: through the helper the hybrid instances with four cells per lane come out of the
    // register allocator 3 to 5 % slower on two or four fields, profiles/README.md)
#pragma unroll
    for (int c = 0; c < V; ++c)
      ps[c] = (P.ps_all != 0 || ps[c] != undef) ? ps[c] : __int_as_float(0x7fc00000);
  }
  auto coordinate = [&](const WalkLevel<NF, V>& L, int k, unsigned int bits, float (&cc)[V]) {
    walk_coordinate<HYBRID ? VDERIV_HYBRID : VDERIV_FIELD, V>(cc, L.c, ps, ab, nlev, k, bits, undef);
  };

  WalkLevel<NF, V> L[R];
  load(L[0], 0);
  load(L[1], 1);
  if (2 < nlev)
    load(L[2], 2);

  LayerState<G, NF, V> S;
  float lo[V], hi[V];
#pragma unroll
  for (int c = 0; c < V; ++c) {
    lo[c] = P.lo;
    hi[c] = P.hi;
    S.bits[c] = 0;
    S.ext[c] = 0.0;
  }
  // rule 2: a bound from a field is tested, the scalars were by the host
  if (P.lo_field != nullptr) {
    walk_load<V>(lo, lane_of(P.lo_field + block0));
#pragma unroll
    for (int c = 0; c < V; ++c)
      S.bits[c] |= (lo[c] != lo[c] || lo[c] == undef) ? CELL_BAD : 0u;
  }
  if (P.hi_field != nullptr) {
    walk_load<V>(hi, lane_of(P.hi_field + block0));
#pragma unroll
    for (int c = 0; c < V; ++c)
      S.bits[c] |= (hi[c] != hi[c] || hi[c] == undef) ? CELL_BAD : 0u;
  }
#pragma unroll
  for (int c = 0; c < V; ++c)
    S.bits[c] |= !(lo[c] < hi[c]) ? CELL_BAD : 0u;
#pragma unroll
  for (int f = 0; f < ((G & VLAYER_SUMS) ? NF : 1); ++f)
#pragma unroll
    for (int c = 0; c < V; ++c)
      S.acc[f][c] = 0.0;
#pragma unroll
  for (int f = 0; f < ((G & VLAYER_EXTREMES) ? NF : 1); ++f)
#pragma unroll
    for (int c = 0; c < V; ++c)
      S.mx[f][c] = S.mn[f][c] = S.cmx[f][c] = S.cmn[f][c] = 0.f;

  unsigned int bits_k = lev_bits[0];
  float ck[V];
  coordinate(L[0], 0, bits_k, ck);
#pragma unroll
  for (int c = 0; c < V; ++c)
    S.bits[c] |= ck[c] != ck[c] ? CELL_BAD : 0u;

  for (int k0 = 0; k0 < nlev - 1; k0 += R) {
#pragma unroll
    for (int d = 0; d < R; ++d) {
      const int k = k0 + d; // the pair (k, k + 1)
      if (k < nlev - 1) {
        WalkLevel<NF, V>& cur = L[d];
        WalkLevel<NF, V>& nx = L[(d + 1) % R];
        const unsigned int bits_k1 = lev_bits[k + 1];
        float ck1[V], a[V], b[V];
        bool part[V];
        coordinate(nx, k + 1, bits_k1, ck1);
        bool any = false, clipped = false;
#pragma unroll
        for (int c = 0; c < V; ++c) {
          S.bits[c] |= ck1[c] != ck1[c] ? CELL_BAD : 0u;
          // rule 3 (a NaN coordinate fails a < b; its cell is undefined anyway)
          const bool rising = ck[c] <= ck1[c];
          const float p = rising ? ck[c] : ck1[c], q = rising ? ck1[c] : ck[c];
          a[c] = p >= lo[c] ? p : lo[c];
          b[c] = q <= hi[c] ? q : hi[c];
          part[c] = a[c] < b[c];
          any |= part[c];
          clipped |= part[c] & (((a[c] != ck[c]) & (a[c] != ck1[c])) | ((b[c] != ck[c]) & (b[c] != ck1[c])));
        }
        if (__builtin_amdgcn_ballot_w64(any) != 0) { // wave-uniform: most pairs outside the layer cost nothing more
          const unsigned int all_k = bits_k >> f0, all_k1 = bits_k1 >> f0;
          if (__builtin_amdgcn_ballot_w64(clipped) != 0)
            vl_pair<true, G, NF, V>(S, cur, nx, ck, ck1, a, b, part, all_k, all_k1, undef);
          else
            vl_pair<false, G, NF, V>(S, cur, nx, ck, ck1, a, b, part, all_k, all_k1, undef);
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

  // rules 1 to 4 decide what is undefined; the products of the others; one store per cell, field and product
  bool cell_bad[V];
#pragma unroll
  for (int c = 0; c < V; ++c)
    cell_bad[c] = (S.bits[c] & CELL_BAD) != 0 || (S.bits[c] & CELL_ANY) == 0;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    bool bad[V];
    unsigned int n = 0;
#pragma unroll
    for (int c = 0; c < V; ++c) {
      bad[c] = cell_bad[c] || ((S.bits[c] >> f) & 1u) != 0;
      n += (unsigned int)__popcll(__builtin_amdgcn_ballot_w64(bad[c] && c < n_mine));
    }
    if (n != 0 && (threadIdx.x & 63) == 0)
      atomicAdd(&s_bad[f], n);
    float* const out = P.out[walk_here(f)] + i0;
    const long out_stride = P.out_stride;
    float r[V];
    if constexpr ((G & VLAYER_SUMS) != 0) {
      if (const int slot = P.slot[walk_here(0)]; slot >= 0) { // MIFC_VLAYER_INTEGRAL
#pragma unroll
        for (int c = 0; c < V; ++c)
          r[c] = bad[c] ? undef : (float)S.acc[f][c];
        walk_store<V>(out + (long)slot * out_stride, r, n_mine);
      }
      if (const int slot = P.slot[walk_here(1)]; slot >= 0) { // MIFC_VLAYER_MEAN
#pragma unroll
        for (int c = 0; c < V; ++c) {
          const double mean = S.acc[f][c] / S.ext[c];
          r[c] = bad[c] ? undef : (float)mean;
        }
        walk_store<V>(out + (long)slot * out_stride, r, n_mine);
      }
    }
    if constexpr ((G & VLAYER_EXTREMES) != 0) {
      if (const int slot = P.slot[walk_here(2)]; slot >= 0) { // MIFC_VLAYER_MAX
#pragma unroll
        for (int c = 0; c < V; ++c)
          r[c] = bad[c] ? undef : S.mx[f][c];
        walk_store<V>(out + (long)slot * out_stride, r, n_mine);
      }
      if (const int slot = P.slot[walk_here(3)]; slot >= 0) { // MIFC_VLAYER_MIN
#pragma unroll
        for (int c = 0; c < V; ++c)
          r[c] = bad[c] ? undef : S.mn[f][c];
        walk_store<V>(out + (long)slot * out_stride, r, n_mine);
      }
      if (const int slot = P.slot[walk_here(4)]; slot >= 0) { // MIFC_VLAYER_COORD_OF_MAX
#pragma unroll
        for (int c = 0; c < V; ++c)
          r[c] = bad[c] ? undef : S.cmx[f][c];
        walk_store<V>(out + (long)slot * out_stride, r, n_mine);
      }
      if (const int slot = P.slot[walk_here(5)]; slot >= 0) { // MIFC_VLAYER_COORD_OF_MIN
#pragma unroll
        for (int c = 0; c < V; ++c)
          r[c] = bad[c] ? undef : S.cmn[f][c];
        walk_store<V>(out + (long)slot * out_stride, r, n_mine);
      }
    }
  }

  __syncthreads();
  if (threadIdx.x < NF && s_bad[threadIdx.x] != 0)
    atomicAdd(P.n_undefined + f0 + threadIdx.x, (u64)s_bad[threadIdx.x]);
}

template <bool HYBRID, int G, int NF>
hipError_t launch_v(const VlayerParams& P, hipStream_t stream)
{
  const int per_block = 256 * (P.vec4 ? 4 : 1);
  const dim3 grid((unsigned int)(((long)P.n + per_block - 1) / per_block)), block(256);
  if (P.vec4)
    hipLaunchKernelGGL((vlayer_kernel<HYBRID, G, NF, 4>), grid, block, 0, stream, P);
  else
    hipLaunchKernelGGL((vlayer_kernel<HYBRID, G, NF, 1>), grid, block, 0, stream, P);
  return hipGetLastError();
}

template <bool HYBRID, int G>
hipError_t launch_nf(const VlayerParams& P, hipStream_t stream)
{
  static_assert(VLAYER_PASS == 4, "one case per field count of a launch");
  if (P.nfields > vlayer_pass_fields(G)) // (the instances beyond a group's capacity do not exist)
    return hipErrorInvalidValue;
  switch (P.nfields) {
  case 1:
    return launch_v<HYBRID, G, 1>(P, stream);
  case 2:
    return launch_v<HYBRID, G, 2>(P, stream);
  case 3:
    if constexpr (vlayer_pass_fields(G) >= 3)
      return launch_v<HYBRID, G, 3>(P, stream);
    return hipErrorInvalidValue;
  case 4:
    if constexpr (vlayer_pass_fields(G) >= 4)
      return launch_v<HYBRID, G, 4>(P, stream);
    return hipErrorInvalidValue;
  default:
    return hipErrorInvalidValue;
  }
}

template <bool HYBRID>
hipError_t launch_group(const VlayerParams& P, hipStream_t stream)
{
  switch (P.group) {
  case VLAYER_SUMS:
    return launch_nf<HYBRID, VLAYER_SUMS>(P, stream);
  case VLAYER_EXTREMES:
    return launch_nf<HYBRID, VLAYER_EXTREMES>(P, stream);
  case VLAYER_SUMS | VLAYER_EXTREMES:
    return launch_nf<HYBRID, VLAYER_SUMS | VLAYER_EXTREMES>(P, stream);
  default:
    return hipErrorInvalidValue;
  }
}

} // namespace

hipError_t launch_vlayer(const VlayerParams& P, hipStream_t stream)
{
  if (P.n <= 0)
    return hipSuccess;
  if (P.nlev < 2 || P.f0 < 0 || P.f0 + P.nfields > VLAYER_MAX_FIELDS)
    return hipErrorInvalidValue;
  return P.hybrid ? launch_group<true>(P, stream) : launch_group<false>(P, stream);
}

} // namespace mifc
