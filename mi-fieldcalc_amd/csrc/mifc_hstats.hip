// mifc_hstats.hip -- horizontal statistics of level batches: area and row reductions (mifc_hstats_levels,
// include/mifc.h; EXTENSION: the reference's callers copy the batch to the host for a minimum or a mean).
//
// The one kernel family of the library that reduces across lanes into a value.  The sums have to come out bit for bit the
// same for every launch shape, memory kind and staging, so the order of every addition is part of the definition (rules 3
// and 4) and the kernels follow it: the cell-to-lane mapping depends on the column index only -- lane l of the wave that
// owns a (row, segment) takes the cells with (i / 4) mod 64 == l, four consecutive cells per trip of 256, at most 16
// trips -- each lane adds its cells in ascending order, and the 64 partials are merged down the fixed tree
// P[t] += P[t + s], s = 32 .. 1, through __shfl_down: no LDS, no atomics on the values.  The (value, index) extremes go
// down the same tree, ties broken by the smaller index.  A wave writes its eight numbers per field as one partial; the
// combine kernel adds the partials of a result sequentially in row-major order.  Cells outside the box, outside the row
// and undefined cells contribute +0.0, which an accumulator that started at +0.0 cannot tell from skipping them, so the
// arithmetic is straight-line code, and the loads are too: addresses outside the box are clamped into it.  All loads of U
// trips (4, or 2 with more than four planes per trip) are issued before the first value is used.
#include "mifc_column_walk.h"
#include "mifc_device.h"
#include "mifc_kernels.h"

#include <algorithm>
#include <cstdint>
#include <type_traits>

namespace mifc {

namespace {

const int HSTATS_COMBINE_AHEAD = 32; // partials in flight per lane of the combine kernel

// what a lane (after the merge: lane 0, the wave) holds of one field
struct HstatsAcc
{
  double w, s1, s2, mn, mx;
  int n, imn, imx;
};

template <int V, int NF, bool WEIGHTED, bool MINUS, bool TESTED, int PRODUCTS>
__global__ __launch_bounds__(256) void hstats_segment_kernel(const HstatsParams P)
{
  constexpr bool MOM = (PRODUCTS & HSTATS_MOMENTS) != 0, EXT = (PRODUCTS & HSTATS_EXTREMES) != 0;
  constexpr int U = NF * (MINUS ? 2 : 1) > 4 ? 2 : 4, NY = MINUS ? NF : 1;
  const int lane = (int)(threadIdx.x & 63u);
  const int unit = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (unit >= P.rows * P.segs) // (wave-uniform)
    return;
  const int r = unit / P.segs, sg = unit - r * P.segs;
  const int seg_begin = (P.seg0 + sg) * HSTATS_SEGMENT;
  // the cells of the segment that are in the box, relative to its first column: [lo, hi), not empty
  const int lo = max(P.i0 - seg_begin, 0), hi = min(P.i1 - seg_begin, HSTATS_SEGMENT);
  const int t_lo = lo / HSTATS_TRIP, t_hi = (hi + HSTATS_TRIP - 1) / HSTATS_TRIP;
  const long row_off = (long)(P.plane_row0 + r) * P.nx + seg_begin; // from a plane's first cell
  const int index0 = (P.grid_row0 + r) * P.nx + seg_begin;          // rule 6: j * nx + i, below 2^31
  const float undef = P.undef;
  const ConstWords lev_bits = (ConstWords)(unsigned long long)P.lev_bits;
  const float* wrow = WEIGHTED ? P.weight + row_off : nullptr;
  double* const part = P.part + (((long)P.f0 * P.nlev * P.box_rows + P.part_row0 + r) * P.segs + sg) * 8; // field f0, level 0
  const long part_level = (long)P.box_rows * P.segs * 8, part_field = part_level * P.nlev;
  const bool weight_all = P.weight_all != 0;

  // The lane's four cells of trip t: one 16-byte load where the rows are on the 16-byte grid (nx % 4 == 0: the groups of
  // four that [lo, hi) touches are inside the row), else four dwords.  The addresses are made safe instead of the loads
  // conditional: a cell outside [lo, hi) reads the nearest one inside (the nearest group of four), and rule 1 throws the
  // value away -- straight-line loads, nothing outside the row is read.
  const int lo4 = lo & ~3, hi4 = ((hi + 3) & ~3) - 4;
  auto load = [&](float (&v)[4], const float* row, int t) {
    const int c0 = t * HSTATS_TRIP + 4 * lane;
    if constexpr (V == 4) {
      const float4 q = *reinterpret_cast<const float4*>(row + min(max(c0, lo4), hi4));
      v[0] = q.x;
      v[1] = q.y;
      v[2] = q.z;
      v[3] = q.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        v[c] = row[min(max(c0 + c, lo), hi - 1)];
    }
  };

  // the wave's row of every plane, at the level the walk is at (advanced, so that the planes' bases need no registers)
  const float* xrow[NF];
  const float* yrow[NY];
  const long level_step = (long)P.level_blocks * P.stride;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    xrow[f] = P.fields[f] + (long)blockIdx.y * P.stride + row_off;
    if constexpr (MINUS)
      yrow[f] = P.minus[f] + (long)blockIdx.y * P.stride + row_off;
  }
  for (int k = (int)blockIdx.y; k < P.nlev; k += P.level_blocks) {
    unsigned int bits = 0; // (wave-uniform, through the scalar cache)
    if constexpr (TESTED)
      bits = lev_bits[k] >> P.f0;
    double pv[NF];
    HstatsAcc a[NF];
    bool allx[NF], ally[NF]; // (wave-uniform: a level flagged ALL_DEFINED tests nothing -- one scalar OR, no branch per cell)
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      allx[f] = ((bits >> f) & 1u) != 0;
      ally[f] = ((bits >> (HSTATS_MINUS_BIT + f)) & 1u) != 0;
      pv[f] = P.pivot[(long)(P.f0 + f) * P.nlev + k]; // (a plain load: the pivots live in vector registers, the scalar ones are short)
      a[f] = {0.0, 0.0, 0.0, __builtin_inf(), -__builtin_inf(), 0, -1, -1};
    }

    // UU trips from trip t on: every load first, then the cells in ascending order
    auto trips = [&](auto count, int t) {
      constexpr int UU = decltype(count)::value;
      float x[UU][NF][4], y[UU][NY][4], wt[UU][4];
#pragma unroll
      for (int u = 0; u < UU; ++u) {
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          load(x[u][f], xrow[f], t + u);
          if constexpr (MINUS)
            load(y[u][f], yrow[f], t + u);
        }
        if constexpr (WEIGHTED)
          load(wt[u], wrow, t + u);
      }
#pragma unroll
      for (int u = 0; u < UU; ++u) {
        const int c0 = (t + u) * HSTATS_TRIP + 4 * lane;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          bool in = (c0 + c >= lo) & (c0 + c < hi); // rule 1: the box
          double wd = 1.0;
          if constexpr (WEIGHTED) {
            wd = (double)wt[u][c];
            if constexpr (TESTED)
              in &= weight_all | is_def(wt[u][c], undef);
          }
#pragma unroll
          for (int f = 0; f < NF; ++f) {
            bool ok = in;
            if constexpr (TESTED)
              ok &= allx[f] | is_def(x[u][f][c], undef);
            double d = (double)x[u][f][c]; // rule 2, every operation rounded on its own
            if constexpr (MINUS) {
              if constexpr (TESTED)
                ok &= ally[f] | is_def(y[u][f][c], undef);
              d = d - (double)y[u][f][c];
            }
            d = d - pv[f];
            if constexpr (MOM) {
              double q1 = d;
              if constexpr (WEIGHTED) {
                q1 = wd * d;
                a[f].w = a[f].w + (ok ? wd : 0.0);
              }
              const double q2 = q1 * d;
              a[f].s1 = a[f].s1 + (ok ? q1 : 0.0);
              a[f].s2 = a[f].s2 + (ok ? q2 : 0.0);
              a[f].n += ok ? 1 : 0;
            }
            if constexpr (EXT) { // rule 6: ordered comparisons, the first of equal values stays (ascending index)
              const bool lt = ok & (d < a[f].mn), gt = ok & (d > a[f].mx);
              a[f].mn = lt ? d : a[f].mn;
              a[f].imn = lt ? index0 + c0 + c : a[f].imn;
              a[f].mx = gt ? d : a[f].mx;
              a[f].imx = gt ? index0 + c0 + c : a[f].imx;
            }
            // (the scheduler otherwise forms the lane masks of every cell of the trips up front and runs out of scalar registers)
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
    };
    int t = t_lo;
    for (; t + U <= t_hi; t += U)
      trips(std::integral_constant<int, U>(), t);
    for (; t < t_hi; ++t)
      trips(std::integral_constant<int, 1>(), t);

    // rule 3: P[t] = P[t] + P[t + s] for t < s, s = 32 .. 1 (the lanes t >= s compute values that nothing reads)
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        if constexpr (MOM) {
          if constexpr (WEIGHTED)
            a[f].w = a[f].w + __shfl_down(a[f].w, s);
          a[f].s1 = a[f].s1 + __shfl_down(a[f].s1, s);
          a[f].s2 = a[f].s2 + __shfl_down(a[f].s2, s);
          a[f].n += __shfl_down(a[f].n, s);
        }
        if constexpr (EXT) { // equal values: the smaller index (nothing selected: +-inf and -1 on both sides, nothing moves)
          const double omn = __shfl_down(a[f].mn, s), omx = __shfl_down(a[f].mx, s);
          const int oimn = __shfl_down(a[f].imn, s), oimx = __shfl_down(a[f].imx, s);
          const bool lt = (omn < a[f].mn) | ((omn == a[f].mn) & (oimn < a[f].imn));
          const bool gt = (omx > a[f].mx) | ((omx == a[f].mx) & (oimx < a[f].imx));
          a[f].mn = lt ? omn : a[f].mn;
          a[f].imn = lt ? oimn : a[f].imn;
          a[f].mx = gt ? omx : a[f].mx;
          a[f].imx = gt ? oimx : a[f].imx;
        }
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        double* o = part + f * part_field + k * part_level;
        if constexpr (MOM) {
          o[0] = (double)a[f].n;
          o[1] = WEIGHTED ? a[f].w : (double)a[f].n; // (w = 1.0 per cell: the sum of rule 3 is the count, exactly)
          o[2] = a[f].s1;
          o[3] = a[f].s2;
        }
        if constexpr (EXT) {
          o[4] = a[f].mn;
          o[5] = a[f].mx;
          o[6] = (double)a[f].imn;
          o[7] = (double)a[f].imx;
        }
      }
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      xrow[f] += level_step;
      if constexpr (MINUS)
        yrow[f] += level_step;
    }
  }
}

// A lane owns one (field, level, result row, slot): rule 4, the partials in row-major order.  The eight lanes of a result
// are neighbours, so the lane of S1 gets N and W for the mean from its own wave.
__global__ __launch_bounds__(256) void hstats_combine_kernel(const HstatsCombineParams P)
{
  const int nrows = P.mode == HSTATS_AREA ? 1 : P.box_rows;
  const long results = (long)P.nfields * P.nlev * nrows;
  const long g = ((long)blockIdx.x * 256 + threadIdx.x) >> 3;
  const int slot = (int)(threadIdx.x & 7u);
  const bool mine = g < results;
  const long gs = mine ? g : 0;
  const long fk = gs / nrows; // f * nlev + k
  const int row = (int)(gs - fk * nrows);
  const long count = P.mode == HSTATS_AREA ? (long)P.box_rows * P.segs : (long)P.segs;
  const double* p = P.part + (fk * P.box_rows + (P.mode == HSTATS_AREA ? 0 : row)) * P.segs * 8;
  const bool moments = (P.products & HSTATS_MOMENTS) != 0, extremes = (P.products & HSTATS_EXTREMES) != 0;
  double res = 0.0;
  // The walk is a chain of dependent additions, but the loads are not: HSTATS_COMBINE_AHEAD partials are fetched before the
  // first of them is added, in the same order (one memory latency per batch instead of one per partial).
  if (mine && slot < 4 && moments) {
    long i = 0;
    for (; i + HSTATS_COMBINE_AHEAD <= count; i += HSTATS_COMBINE_AHEAD) {
      double v[HSTATS_COMBINE_AHEAD];
#pragma unroll
      for (int u = 0; u < HSTATS_COMBINE_AHEAD; ++u)
        v[u] = p[(i + u) * 8 + slot];
#pragma unroll
      for (int u = 0; u < HSTATS_COMBINE_AHEAD; ++u)
        res = res + v[u];
    }
    for (; i < count; ++i)
      res = res + p[i * 8 + slot];
  } else if (mine && slot >= 4 && extremes) {
    const bool is_min = (slot & 1) == 0;
    const double* pv = p + (is_min ? 4 : 5);
    const double* pi = p + (is_min ? 6 : 7);
    double best = is_min ? __builtin_inf() : -__builtin_inf(), at = -1.0;
    auto step = [&](double v, double index) { // later partials hold larger indices: the first of equal values stays
      const bool take = is_min ? v < best : v > best;
      at = take ? index : at;
      best = take ? v : best;
    };
    long i = 0;
    for (; i + HSTATS_COMBINE_AHEAD / 2 <= count; i += HSTATS_COMBINE_AHEAD / 2) {
      double v[HSTATS_COMBINE_AHEAD / 2], index[HSTATS_COMBINE_AHEAD / 2];
#pragma unroll
      for (int u = 0; u < HSTATS_COMBINE_AHEAD / 2; ++u) {
        v[u] = pv[(i + u) * 8];
        index[u] = pi[(i + u) * 8];
      }
#pragma unroll
      for (int u = 0; u < HSTATS_COMBINE_AHEAD / 2; ++u)
        step(v[u], index[u]);
    }
    for (; i < count; ++i)
      step(pv[i * 8], pi[i * 8]);
    res = slot < 6 ? best : at;
  }
  if (mine && (slot < 4 ? moments : extremes))
    P.stats[g * 8 + slot] = res;
  if (P.mean[0] != nullptr) { // (uniform; every lane of the wave takes part in the shuffles)
    const int base = (int)(threadIdx.x & 63u) & ~7;
    const double n = __shfl(res, base), w = __shfl(res, base + 1);
    if (mine && slot == 2) {
      const int f = (int)(fk / P.nlev);
      const bool hole = n == 0.0 || w == 0.0;
      const double q = res / w;
      const double m = P.pivot[fk] + q;
      float* out = P.mean[0]; // (selected, not indexed: the argument array stays in scalar registers)
#pragma unroll
      for (int j = 1; j < HSTATS_MAX_FIELDS; ++j)
        out = f == j ? P.mean[j] : out;
      out[(fk - (long)f * P.nlev) * nrows + row] = hole ? P.undef : (float)m;
      if (hole)
        atomicAdd(P.n_undefined + fk, (u64)1);
    }
  }
}

template <int V, int NF, bool WEIGHTED, bool MINUS, bool TESTED>
hipError_t launch_products(const HstatsParams& P, const dim3 grid, hipStream_t stream)
{
  switch (P.products) {
  case HSTATS_MOMENTS:
    hipLaunchKernelGGL((hstats_segment_kernel<V, NF, WEIGHTED, MINUS, TESTED, HSTATS_MOMENTS>), grid, dim3(256), 0, stream, P);
    break;
  case HSTATS_EXTREMES:
    hipLaunchKernelGGL((hstats_segment_kernel<V, NF, WEIGHTED, MINUS, TESTED, HSTATS_EXTREMES>), grid, dim3(256), 0, stream, P);
    break;
  case HSTATS_MOMENTS | HSTATS_EXTREMES:
    hipLaunchKernelGGL((hstats_segment_kernel<V, NF, WEIGHTED, MINUS, TESTED, HSTATS_MOMENTS | HSTATS_EXTREMES>), grid, dim3(256), 0, stream, P);
    break;
  default:
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

template <int V, int NF>
hipError_t launch_flags(const HstatsParams& P, const dim3 grid, hipStream_t stream)
{
  const bool w = P.weight != nullptr, m = P.minus[0] != nullptr, t = P.tested != 0;
  if (w)
    return m ? (t ? launch_products<V, NF, true, true, true>(P, grid, stream) : launch_products<V, NF, true, true, false>(P, grid, stream))
             : (t ? launch_products<V, NF, true, false, true>(P, grid, stream) : launch_products<V, NF, true, false, false>(P, grid, stream));
  return m ? (t ? launch_products<V, NF, false, true, true>(P, grid, stream) : launch_products<V, NF, false, true, false>(P, grid, stream))
           : (t ? launch_products<V, NF, false, false, true>(P, grid, stream) : launch_products<V, NF, false, false, false>(P, grid, stream));
}

template <int V>
hipError_t launch_nf(const HstatsParams& P, const dim3 grid, hipStream_t stream)
{
  static_assert(HSTATS_PASS == 4, "one case per field count of a launch");
  switch (P.nfields) {
  case 1:
    return launch_flags<V, 1>(P, grid, stream);
  case 2:
    return launch_flags<V, 2>(P, grid, stream);
  case 3:
    return launch_flags<V, 3>(P, grid, stream);
  case 4:
    return launch_flags<V, 4>(P, grid, stream);
  default:
    return hipErrorInvalidValue;
  }
}

bool on_16(const void* p)
{
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

} // namespace

HstatsPlan hstats_plan(int rows, int segs, int nlev)
{
  const long units = (long)rows * segs;
  return {(int)((units + 3) / 4), std::min(nlev, 65535)};
}

hipError_t launch_hstats_segments(const HstatsParams& prm, hipStream_t stream)
{
  HstatsParams P = prm;
  // the box inside the row, the rows inside the box, the segments exactly the ones that the box touches
  if (P.nx < 1 || P.nlev < 1 || P.rows < 1 || P.i0 < 0 || P.i1 <= P.i0 || P.i1 > P.nx || P.plane_row0 < 0 || P.grid_row0 < 0 || P.part_row0 < 0 ||
      P.part_row0 + P.rows > P.box_rows || P.seg0 != P.i0 / HSTATS_SEGMENT || P.segs != (P.i1 - 1) / HSTATS_SEGMENT - P.seg0 + 1 || P.f0 < 0 ||
      P.nfields < 1 || P.f0 + P.nfields > HSTATS_MAX_FIELDS || (long)(P.grid_row0 + P.rows) * P.nx > 0x7fffffffL || !P.part || !P.pivot ||
      !P.lev_bits)
    return hipErrorInvalidValue;
  bool grid16 = (P.nx & 3) == 0 && (P.stride & 3) == 0 && on_16(P.weight);
  for (int f = 0; f < P.nfields; ++f) {
    if (!P.fields[f] || (P.minus[0] != nullptr) != (P.minus[f] != nullptr))
      return hipErrorInvalidValue;
    grid16 = grid16 && on_16(P.fields[f]) && on_16(P.minus[f]);
  }
  if (P.vec4 && !grid16)
    return hipErrorInvalidValue;
  const HstatsPlan plan = hstats_plan(P.rows, P.segs, P.nlev);
  P.level_blocks = plan.level_blocks;
  const dim3 grid((unsigned int)plan.blocks, (unsigned int)plan.level_blocks);
  return P.vec4 ? launch_nf<4>(P, grid, stream) : launch_nf<1>(P, grid, stream);
}

hipError_t launch_hstats_combine(const HstatsCombineParams& P, hipStream_t stream)
{
  if (P.nfields < 1 || P.nfields > HSTATS_MAX_FIELDS || P.nlev < 1 || P.box_rows < 1 || P.segs < 1 || (P.mode != HSTATS_AREA && P.mode != HSTATS_ROWS) ||
      (P.products & ~(HSTATS_MOMENTS | HSTATS_EXTREMES)) != 0 || P.products == 0 || !P.part || !P.stats)
    return hipErrorInvalidValue;
  if (P.mean[0] != nullptr) {
    if ((P.products & HSTATS_MOMENTS) == 0 || !P.pivot || !P.n_undefined)
      return hipErrorInvalidValue;
    for (int f = 0; f < P.nfields; ++f)
      if (!P.mean[f])
        return hipErrorInvalidValue;
  }
  const long lanes = (long)P.nfields * P.nlev * (P.mode == HSTATS_AREA ? 1 : P.box_rows) * 8;
  hipLaunchKernelGGL(hstats_combine_kernel, dim3((unsigned int)((lanes + 255) / 256)), dim3(256), 0, stream, P);
  return hipGetLastError();
}

} // namespace mifc
