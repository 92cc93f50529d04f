// mifc_hdist.hip -- area histograms and exact percentiles of level batches (mifc_hdist_histogram_levels,
// mifc_hdist_quantile_levels, include/mifc.h; EXTENSION: the reference's callers copy the batch to the host for a
// histogram or a median).  Every result is a count of cells or an order statistic, so nothing depends on the order of
// work: the counters are integers, added with LDS and global atomics, and the results are the same bits for every launch
// shape, memory kind and staging.  The arithmetic of the rules -- keys, bins, ranks, digits, the scan step -- is
// mifc_hdist_rules.h, the text that the host code and the tests compile too.
//
// One walk kernel (hdist_walk_kernel) reads the cells, as hstats_segment_kernel does: 16-byte loads where every row is on
// the 16-byte grid, dwords otherwise, addresses made safe instead of loads made conditional, the ALL_DEFINED test of a
// level one scalar OR from the level table, the levels on grid.y.  What it does with a cell is its WHAT:
//   HDIST_COUNT   the cell's bin against the field's edges (their keys in LDS), counted in LDS, flushed once per unit of
//                 work -- the workgroup's rows (AREA) or each row (ROWS) -- with atomicAdd on the int result, zero bins skipped;
//   HDIST_EXTENT  n, the smallest and the largest key of (field, level): registers, a wave merge, three atomics per wave;
//   HDIST_DIGIT   the digit of pass `pass` below whichever of the unit's prefixes the cell's key matches, counted in LDS
//                 for HDIST_GROUP_SLOTS prefixes at a time (a unit with more reads its cells once per group), flushed to
//                 the unit's digit counters.
// Smooth fields put whole waves into one bin, and a same-address LDS atomic serialises: a lane first merges its four
// consecutive cells, then the lanes whose four cells share the bin of the first such lane are counted by one ballot and
// added by one lane; only what is left goes to the counters lane by lane (lds_count4).
// Between the walks of the selection small kernels turn ranks into (prefix, rank inside the prefix): nothing returns to
// the host before the call's one synchronisation.
#define MIFC_HDIST_FN __host__ __device__ inline
#include "mifc_hdist_rules.h"

#include "mifc_column_walk.h"
#include "mifc_device.h"
#include "mifc_kernels.h"

#include <algorithm>
#include <cstdint>
#include <type_traits>

namespace mifc {

static_assert(HDIST_MAX_RANKS == 32 && HDIST_MAX_Q == 16 && HDIST_MAX_PASSES == 3 && HDIST_MAX_FIELDS == 8, "HdistUnit, HdistParams (mifc_kernels.h)");
static_assert(HDIST_DIGIT_BINS == 2048, "a lane of the scan kernel sums 32 bins");

namespace {

const int HDIST_TRIP = 1024;           // cells of a workgroup's trip: four per lane
const int HDIST_GROUP_CELLS = 1 << 16; // cells of a workgroup's unit of work (AREA), where the box has them
const int HDIST_MIN_GROUPS = 4096;     // workgroups of a launch before a unit of work grows to that

// (selected, not indexed: the argument arrays stay in scalar registers)
template <class T>
__device__ __forceinline__ T* pick8(T* const (&p)[8], int f)
{
  T* r = p[0];
#pragma unroll
  for (int j = 1; j < 8; ++j)
    r = f == j ? p[j] : r;
  return r;
}

// Four counter indices of a lane (-1: nothing to count) into LDS counters.  All lanes of the wave call it together.
__device__ __forceinline__ void lds_count4(unsigned int* counters, const int (&idx)[4], bool plain)
{
  const bool same4 = idx[0] >= 0 && idx[0] == idx[1] && idx[0] == idx[2] && idx[0] == idx[3];
  const unsigned long long any = __ballot(same4);
  bool done = false;
  if (any != 0ull && !plain) { // (wave-uniform)
    const int leader = __ffsll((long long)any) - 1;
    const int lead_idx = __shfl(idx[0], leader);
    done = same4 && idx[0] == lead_idx;
    const unsigned long long with = __ballot(done);
    if ((int)(threadIdx.x & 63u) == leader)
      atomicAdd(&counters[lead_idx], 4u * (unsigned int)__popcll(with));
  }
  if (!done) { // the lane's runs of equal indices, one add each
    int run = idx[0];
    unsigned int len = 1;
#pragma unroll
    for (int c = 1; c < 4; ++c) {
      if (idx[c] == run) {
        len += 1;
      } else {
        if (run >= 0)
          atomicAdd(&counters[run], len);
        run = idx[c];
        len = 1;
      }
    }
    if (run >= 0)
      atomicAdd(&counters[run], len);
  }
}

template <int V, bool MASKED, bool TESTED, int WHAT>
__global__ __launch_bounds__(256) void hdist_walk_kernel(const HdistParams P)
{
  constexpr int U = MASKED ? 2 : 4; // trips in flight: the same number of loads with and without the mask plane
  __shared__ unsigned int s_counters[WHAT == HDIST_COUNT ? HDIST_MAX_EDGES + 2 : (WHAT == HDIST_DIGIT ? HDIST_GROUP_SLOTS * HDIST_DIGIT_BINS : 1)];
  __shared__ unsigned int s_keys[WHAT == HDIST_COUNT ? HDIST_MAX_EDGES : (WHAT == HDIST_DIGIT ? HDIST_GROUP_SLOTS : 1)];
  const int tid = (int)threadIdx.x;
  const int f = (int)blockIdx.z;
  const int r0 = (int)blockIdx.x * P.rows_per_group, r1 = min(r0 + P.rows_per_group, P.rows);
  const int lo = P.i0, hi = P.i1; // the box's columns, not empty
  // (columns as unsigned words: the last trip of a row of 2^31 - 1 cells ends beyond the largest int)
  const unsigned int cbase = (unsigned int)lo & ~3u;
  const int trips = (int)(((unsigned int)hi - cbase + HDIST_TRIP - 1u) / HDIST_TRIP);
  const int lo4 = lo & ~3, hi4 = (int)((((unsigned int)hi + 3u) & ~3u) - 4u);
  const float undef = P.undef;
  const ConstWords lev_bits = (ConstWords)(unsigned long long)P.lev_bits;
  const bool mask_all = P.mask_all != 0, plain = P.plain != 0;
  const float* const field = pick8(P.fields, f);
  const int nedges = P.nedges, nslots_out = nedges + 2;

  // The lane's four cells of trip t (see hstats_segment_kernel): a cell outside [lo, hi) reads the nearest one inside
  // (the nearest group of four), and the box test throws the value away -- nothing outside the row is read.
  auto load = [&](float (&v)[4], const float* row, int t) {
    const unsigned int c0 = cbase + (unsigned int)t * HDIST_TRIP + 4u * (unsigned int)tid;
    if constexpr (V == 4) {
      const float4 q = *reinterpret_cast<const float4*>(row + min(max(c0, (unsigned int)lo4), (unsigned int)hi4));
      v[0] = q.x;
      v[1] = q.y;
      v[2] = q.z;
      v[3] = q.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        v[c] = row[min(max(c0 + c, (unsigned int)lo), (unsigned int)hi - 1u)];
    }
  };

  if constexpr (WHAT == HDIST_COUNT) {
    for (int e = tid; e < nedges; e += 256)
      s_keys[e] = P.edge_keys[(long)f * nedges + e];
  }

  for (int k = (int)blockIdx.y; k < P.nlev; k += P.level_blocks) {
    bool allx = true; // (wave-uniform: a level flagged ALL_DEFINED tests nothing)
    if constexpr (TESTED)
      allx = ((lev_bits[P.lev0 + k] >> f) & 1u) != 0;
    const float* const plane = field + (long)k * P.stride;
    HdistUnit* const unit = WHAT == HDIST_COUNT ? nullptr : P.units + ((long)f * P.unit_levels + k);
    unsigned int n = 0, kmin = 0xffffffffu, kmax = 0u; // HDIST_EXTENT
    int shift = 0, width = 0, nslots = 1;               // HDIST_DIGIT
    if constexpr (WHAT == HDIST_DIGIT) {
      if (P.pass >= unit->passes) // (uniform over the workgroup: this unit has its keys)
        continue;
      shift = unit->pass_shift[P.pass];
      width = unit->pass_width[P.pass];
      nslots = unit->nslots;
    }

    // The cells of the rows [ra, rb) of the launch, four at a time into cells4(values, included).  The trips of all the
    // rows are one sequence, U of them in flight: a row of 1440 cells is two trips, and a walk row by row would wait for
    // every load on its own.
    auto walk_rows = [&](int ra, int rb, auto&& cells4) {
      const int items = (rb - ra) * trips;
      int r = ra, t = 0; // the next trip
      auto some = [&](auto count) {
        constexpr int UU = decltype(count)::value;
        float x[UU][4], m[UU][4];
        unsigned int c0[UU];
#pragma unroll
        for (int u = 0; u < UU; ++u) {
          const long row_off = (long)(P.plane_row0 + r) * P.nx;
          load(x[u], plane + row_off, t);
          if constexpr (MASKED)
            load(m[u], P.mask + row_off, t);
          c0[u] = cbase + (unsigned int)t * HDIST_TRIP + 4u * (unsigned int)tid;
          t += 1;
          if (t == trips) { // (uniform)
            t = 0;
            r += 1;
          }
        }
#pragma unroll
        for (int u = 0; u < UU; ++u) {
          bool in[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            in[c] = (c0[u] + c >= (unsigned int)lo) & (c0[u] + c < (unsigned int)hi); // the box
            if constexpr (TESTED)
              in[c] &= allx | is_def(x[u][c], undef);
            if constexpr (MASKED)
              in[c] &= mask_all | is_def(m[u][c], undef);
          }
          cells4(x[u], in);
          // (the scheduler otherwise forms the lane masks of every cell of the trips up front and runs out of scalar registers)
          __builtin_amdgcn_sched_barrier(0);
        }
      };
      int done = 0;
      for (; done + U <= items; done += U)
        some(std::integral_constant<int, U>());
      for (; done < items; ++done)
        some(std::integral_constant<int, 1>());
    };

    if constexpr (WHAT == HDIST_COUNT) {
      // a unit of work: the workgroup's rows (AREA) or one row (ROWS); the counters zeroed, filled, flushed
      const int step = P.per_row ? 1 : max(r1 - r0, 1);
      for (int ra = r0; ra < r1; ra += step) {
        __syncthreads(); // (the edges are in place; the flush before is over)
        for (int b = tid; b < nslots_out; b += 256)
          s_counters[b] = 0u;
        __syncthreads();
        walk_rows(ra, min(ra + step, r1), [&](const float (&x)[4], const bool (&in)[4]) {
          int idx[4];
#pragma unroll
          for (int c = 0; c < 4; ++c)
            idx[c] = in[c] ? hdist_slot(s_keys, nedges, __float_as_uint(x[c])) : -1;
          lds_count4(s_counters, idx, plain);
        });
        __syncthreads();
        const int out_row = P.per_row ? P.out_row0 + ra : 0;
        int* const out = P.hist + (((long)f * P.call_nlev + P.lev0 + k) * P.out_rows + out_row) * nslots_out;
        for (int b = tid; b < nslots_out; b += 256) {
          const unsigned int cnt = s_counters[b];
          if (cnt != 0u)
            atomicAdd(out + b, (int)cnt);
        }
      }
    } else if constexpr (WHAT == HDIST_EXTENT) {
      walk_rows(r0, r1, [&](const float (&x)[4], const bool (&in)[4]) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const unsigned int key = hdist_order_key(__float_as_uint(x[c]));
          n += in[c] ? 1u : 0u;
          kmin = min(kmin, in[c] ? key : 0xffffffffu);
          kmax = max(kmax, in[c] ? key : 0u);
          __builtin_amdgcn_sched_barrier(0); // (one cell's lane mask at a time)
        }
      });
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) {
        n += __shfl_down(n, s);
        kmin = min(kmin, __shfl_down(kmin, s));
        kmax = max(kmax, __shfl_down(kmax, s));
      }
      if ((tid & 63) == 0 && n != 0u) {
        atomicAdd(&unit->n, n);
        atomicMin(&unit->kmin, kmin);
        atomicMax(&unit->kmax, kmax);
      }
    } else {
      for (int g0 = 0; g0 < nslots; g0 += HDIST_GROUP_SLOTS) {
        const int ng = min(HDIST_GROUP_SLOTS, nslots - g0);
        __syncthreads(); // (the flush of the group before is over)
        if (tid < HDIST_GROUP_SLOTS)
          s_keys[tid] = unit->slot_prefix[g0 + min(tid, ng - 1)];
        for (int b = tid; b < ng * HDIST_DIGIT_BINS; b += 256)
          s_counters[b] = 0u;
        __syncthreads();
        unsigned int pre[HDIST_GROUP_SLOTS];
#pragma unroll
        for (int q = 0; q < HDIST_GROUP_SLOTS; ++q)
          pre[q] = s_keys[q];
        walk_rows(r0, r1, [&](const float (&x)[4], const bool (&in)[4]) {
          int idx[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const unsigned int key = hdist_order_key(__float_as_uint(x[c]));
            const unsigned int above = hdist_prefix_of(key, shift, width);
            int slot = -1;
#pragma unroll
            for (int q = 0; q < HDIST_GROUP_SLOTS; ++q)
              slot = (q < ng && pre[q] == above) ? q : slot;
            idx[c] = (in[c] && slot >= 0) ? slot * HDIST_DIGIT_BINS + (int)hdist_digit_of(key, shift, width) : -1;
          }
          lds_count4(s_counters, idx, plain);
        });
        __syncthreads();
        unsigned int* const out = P.digit_hist + (((long)f * P.unit_levels + k) * P.slot_stride + g0) * HDIST_DIGIT_BINS;
        for (int b = tid; b < ng * HDIST_DIGIT_BINS; b += 256) {
          const unsigned int cnt = s_counters[b];
          if (cnt != 0u)
            atomicAdd(out + b, cnt);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------- the selection between the walks
__global__ __launch_bounds__(256) void hdist_init_kernel(const HdistSelectParams P)
{
  const int u = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (u >= P.nunits)
    return;
  HdistUnit* const unit = P.units + u;
  unit->n = 0u;
  unit->kmin = 0xffffffffu;
  unit->kmax = 0u;
  unit->passes = 0;
  unit->nranks = 0;
  unit->nslots = 0;
}

// A lane owns a unit: the digits between its extreme keys, the ranks that the percentiles ask for (each once), all of
// them inside the one prefix that the extremes share.
__global__ __launch_bounds__(64) void hdist_plan_kernel(const HdistSelectParams P)
{
  const int u = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (u >= P.nunits)
    return;
  HdistUnit* const unit = P.units + u;
  const unsigned int n = unit->n;
  if (n == 0u)
    return;
  const HdistPlan plan = hdist_digit_plan(unit->kmin, unit->kmax);
  unit->passes = plan.passes;
#pragma unroll
  for (int j = 0; j < HDIST_MAX_PASSES; ++j) {
    unit->pass_shift[j] = plan.shift[j];
    unit->pass_width[j] = plan.width[j];
  }
  const unsigned int low = plan.prefix_bits >= 32 ? 0u : 0xffffffffu >> plan.prefix_bits; // the bits still to find
  const unsigned int start = unit->kmin & ~low;
  int nranks = 0;
  auto want = [&](unsigned int rank) {
    for (int r = 0; r < nranks; ++r)
      if (unit->rank_left[r] == rank)
        return r;
    unit->rank_left[nranks] = rank;
    unit->rank_key[nranks] = start;
    unit->rank_slot[nranks] = 0;
    return nranks++;
  };
  for (int q = 0; q < P.nq; ++q) {
    const HdistRank rk = hdist_rank(P.method, (int)n, P.percentiles[q]);
    unit->qk[q] = want((unsigned int)rk.k);
    unit->qk1[q] = want((unsigned int)rk.k1);
    unit->qt[q] = rk.t;
  }
  unit->nranks = nranks;
  unit->nslots = 1;
  unit->slot_prefix[0] = plan.passes > 0 ? hdist_prefix_of(start, plan.shift[0], plan.width[0]) : 0u;
}

// A workgroup owns a unit behind the digit walk of `pass`; a wave a rank at a time: the lanes sum 32 digits each, the
// scan step over the 64 sums gives the lane, the scan step over that lane's digits the digit.  Then the prefixes of the
// next pass, each once.
__global__ __launch_bounds__(256) void hdist_scan_kernel(const HdistSelectParams P)
{
  __shared__ unsigned int s_sum[4][64];
  HdistUnit* const unit = P.units + blockIdx.x;
  const int pass = P.pass;
  if (pass >= unit->passes) // (uniform)
    return;
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const int nranks = unit->nranks, shift = unit->pass_shift[pass];
  for (int rb = 0; rb < nranks; rb += 4) {
    const int r = rb + wave;
    const bool mine = r < nranks;
    const unsigned int* const hist = P.digit_hist + ((long)blockIdx.x * P.slot_stride + (mine ? unit->rank_slot[r] : 0)) * HDIST_DIGIT_BINS;
    unsigned int sum = 0u;
    if (mine) {
#pragma unroll 4
      for (int i = 0; i < 32; ++i)
        sum += hist[lane * 32 + i];
    }
    __syncthreads();
    s_sum[wave][lane] = sum;
    __syncthreads();
    if (mine && lane == 0) {
      const HdistStep coarse = hdist_scan_step(s_sum[wave], 64, unit->rank_left[r]);
      const HdistStep fine = hdist_scan_step(hist + coarse.digit * 32, 32, coarse.rank);
      unit->rank_key[r] |= (unsigned int)(coarse.digit * 32 + fine.digit) << shift;
      unit->rank_left[r] = fine.rank;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && pass + 1 < unit->passes) {
    const int nshift = unit->pass_shift[pass + 1], nwidth = unit->pass_width[pass + 1];
    int nslots = 0;
    for (int r = 0; r < nranks; ++r) {
      const unsigned int above = hdist_prefix_of(unit->rank_key[r], nshift, nwidth);
      int slot = -1;
      for (int s = 0; s < nslots; ++s)
        slot = unit->slot_prefix[s] == above ? s : slot;
      if (slot < 0) {
        slot = nslots++;
        unit->slot_prefix[slot] = above;
      }
      unit->rank_slot[r] = slot;
    }
    unit->nslots = nslots;
  }
}

// A lane owns one (unit, percentile): x[k], or the interpolation in double; undef and a count where nothing is included.
__global__ __launch_bounds__(256) void hdist_final_kernel(const HdistSelectParams P)
{
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long)P.nunits * P.nq)
    return;
  const int u = (int)(g / P.nq), q = (int)(g - (long)u * P.nq);
  const int f = u / P.unit_levels, k = P.lev0 + (u - f * P.unit_levels);
  const HdistUnit* const unit = P.units + u;
  float* const out = pick8(P.quant, f) + (long)k * P.nq + q;
  if (unit->n == 0u) {
    *out = P.undef;
    atomicAdd(P.n_undefined + ((long)f * P.call_nlev + k), (u64)1);
    return;
  }
  const unsigned int a = hdist_key_bits(unit->rank_key[unit->qk[q]]), b = hdist_key_bits(unit->rank_key[unit->qk1[q]]);
  *out = hdist_interpolate(a, b, unit->qt[q]);
}

template <int V, bool MASKED, bool TESTED>
hipError_t launch_what(const HdistParams& P, const dim3 grid, hipStream_t stream)
{
  switch (P.what) {
  case HDIST_COUNT:
    hipLaunchKernelGGL((hdist_walk_kernel<V, MASKED, TESTED, HDIST_COUNT>), grid, dim3(256), 0, stream, P);
    break;
  case HDIST_EXTENT:
    hipLaunchKernelGGL((hdist_walk_kernel<V, MASKED, TESTED, HDIST_EXTENT>), grid, dim3(256), 0, stream, P);
    break;
  case HDIST_DIGIT:
    hipLaunchKernelGGL((hdist_walk_kernel<V, MASKED, TESTED, HDIST_DIGIT>), grid, dim3(256), 0, stream, P);
    break;
  default:
    return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

template <int V>
hipError_t launch_tests(const HdistParams& P, const dim3 grid, hipStream_t stream)
{
  if (!P.tested)
    return launch_what<V, false, false>(P, grid, stream);
  return P.mask ? launch_what<V, true, true>(P, grid, stream) : launch_what<V, false, true>(P, grid, stream);
}

bool on_16(const void* p)
{
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

bool select_ok(const HdistSelectParams& P)
{
  return P.nunits >= 1 && P.unit_levels >= 1 && P.nunits % P.unit_levels == 0 && P.nunits / P.unit_levels <= HDIST_MAX_FIELDS && P.units != nullptr;
}

} // namespace

HdistWalkShape hdist_walk_shape(const HdistParams& P)
{
  // The rows of a workgroup's unit of work: HDIST_GROUP_CELLS cells, so that the flush and the zeroing of the counters are
  // a few per cent of what is read -- but fewer, down to an eighth (the selection's walks: a half), while the launch has fewer than
  // HDIST_MIN_GROUPS workgroups (a single level otherwise leaves most of the device idle).
  const int width = std::max(P.i1 - P.i0, 1);
  int rows_per_group = P.rows_per_group;
  if (rows_per_group < 1) {
    if (P.what == HDIST_COUNT && P.per_row) {
      rows_per_group = 1;
    } else {
      const int small = P.what == HDIST_COUNT ? HDIST_GROUP_CELLS / 8 : HDIST_GROUP_CELLS / 2; // (a digit flush is up to four times 2048 counters)
      const int full = (HDIST_GROUP_CELLS + width - 1) / width, least = (small + width - 1) / width;
      const long planes = (long)std::max(P.nlev, 1) * std::max(P.nfields, 1);
      const long want = (HDIST_MIN_GROUPS + planes - 1) / planes; // workgroups per (field, level)
      const int spread = (int)std::max<long>(1, P.rows / want);
      rows_per_group = std::max(1, std::min(P.rows, std::min(full, std::max(least, spread))));
    }
  }
  return {(P.rows + rows_per_group - 1) / rows_per_group, std::min(P.nlev, 65535)};
}

hipError_t launch_hdist_walk(const HdistParams& prm, hipStream_t stream)
{
  HdistParams P = prm;
  // the box inside the row, the fields there, the counters that the purpose needs
  if (P.nx < 1 || P.nlev < 1 || P.lev0 < 0 || P.rows < 1 || P.i0 < 0 || P.i1 <= P.i0 || P.i1 > P.nx || P.plane_row0 < 0 || P.nfields < 1 ||
      P.nfields > HDIST_MAX_FIELDS || !P.lev_bits || (P.mask && !P.tested))
    return hipErrorInvalidValue;
  if (P.what == HDIST_COUNT) {
    if (P.nedges < 1 || P.nedges > HDIST_MAX_EDGES || !P.edge_keys || !P.hist || P.out_rows < 1 || P.call_nlev < P.lev0 + P.nlev || P.out_row0 < 0 ||
        (P.per_row ? P.out_row0 + P.rows > P.out_rows : P.out_rows != 1))
      return hipErrorInvalidValue;
  } else if (P.what == HDIST_EXTENT || P.what == HDIST_DIGIT) {
    if (!P.units || P.unit_levels < P.nlev)
      return hipErrorInvalidValue;
    if (P.what == HDIST_DIGIT && (!P.digit_hist || P.pass < 0 || P.pass >= HDIST_MAX_PASSES || P.slot_stride < 1 || P.slot_stride > HDIST_MAX_RANKS))
      return hipErrorInvalidValue;
  } else {
    return hipErrorInvalidValue;
  }
  bool grid16 = (P.nx & 3) == 0 && (P.stride & 3) == 0 && on_16(P.mask);
  for (int f = 0; f < P.nfields; ++f) {
    if (!P.fields[f])
      return hipErrorInvalidValue;
    grid16 = grid16 && on_16(P.fields[f]);
  }
  if (P.vec4 && !grid16)
    return hipErrorInvalidValue;
  P.rows_per_group = 0;
  const HdistWalkShape shape = hdist_walk_shape(P);
  P.rows_per_group = (P.rows + shape.groups - 1) / shape.groups;
  P.level_blocks = shape.level_blocks;
  const dim3 grid((unsigned int)shape.groups, (unsigned int)shape.level_blocks, (unsigned int)P.nfields);
  return P.vec4 ? launch_tests<4>(P, grid, stream) : launch_tests<1>(P, grid, stream);
}

hipError_t launch_hdist_init(const HdistSelectParams& P, hipStream_t stream)
{
  if (!select_ok(P))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(hdist_init_kernel, dim3((unsigned int)((P.nunits + 255) / 256)), dim3(256), 0, stream, P);
  return hipGetLastError();
}

hipError_t launch_hdist_plan(const HdistSelectParams& P, hipStream_t stream)
{
  if (!select_ok(P) || P.nq < 1 || P.nq > HDIST_MAX_Q || (P.method != HDIST_LOWER && P.method != HDIST_LINEAR) || !P.percentiles)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(hdist_plan_kernel, dim3((unsigned int)((P.nunits + 63) / 64)), dim3(64), 0, stream, P);
  return hipGetLastError();
}

hipError_t launch_hdist_scan(const HdistSelectParams& P, hipStream_t stream)
{
  if (!select_ok(P) || !P.digit_hist || P.pass < 0 || P.pass >= HDIST_MAX_PASSES || P.slot_stride < 1 || P.slot_stride > HDIST_MAX_RANKS)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(hdist_scan_kernel, dim3((unsigned int)P.nunits), dim3(256), 0, stream, P);
  return hipGetLastError();
}

hipError_t launch_hdist_final(const HdistSelectParams& P, hipStream_t stream)
{
  if (!select_ok(P) || P.nq < 1 || P.nq > HDIST_MAX_Q || !P.n_undefined || P.lev0 < 0 || P.call_nlev < P.lev0 + P.unit_levels)
    return hipErrorInvalidValue;
  for (int f = 0; f < P.nunits / P.unit_levels; ++f)
    if (!P.quant[f])
      return hipErrorInvalidValue;
  const long lanes = (long)P.nunits * P.nq;
  hipLaunchKernelGGL(hdist_final_kernel, dim3((unsigned int)((lanes + 255) / 256)), dim3(256), 0, stream, P);
  return hipGetLastError();
}

} // namespace mifc
