// mifc_quantile.hip -- percentiles across ensemble members, per cell, over [nlev][ny][nx] batches
// (mifc_ensembleQuantiles, include/mifc.h; EXTENSION: the reference has no such function, its rule for choosing a
// percentile is neighbourFunctions compute 4, FieldCalculations.cc:2955-3061).
//
// One lane per cell, grid-stride over a level, grid.y over the levels.  Every value is turned into an
// order-preserving uint32 key (IEEE total order, -0 < +0; every NaN canonicalised to 0xffffffff, above +inf);
// members that do not count at the cell and the padding of the network get 0xffffffff too, so that they sort past
// the n counted keys.
//   nmem <= 64: the keys of all members are loaded (all loads issued before the first is used), sorted in registers by
//     Batcher's odd-even merge network for the capacity tier K = 8 / 16 / 32 / 64 (v_min_u32 / v_max_u32, the
//     comparator list generated at compile time), and every percentile reads its rank(s) from the sorted keys through
//     a select tree on the bits of the rank (no dynamic register index: no scratch).
//   nmem > 64: no cap.  The exact order statistic by bisection over the keys, as mifc_neighbour.hip does for a window:
//     one pass for n and the min / max counted key, then, per rank, the largest t with #{key < t} <= rank, bit by bit
//     below their common prefix; every pass reads the members again.
// The undefined count (cells without a counted member) is handed over per workgroup and level.
#include "mifc_device.h"
#include "mifc_kernels.h"

#include <utility>

namespace mifc {

namespace {

__device__ __forceinline__ unsigned q_key(float x)
{
  const unsigned b = __float_as_uint(x);
  const unsigned k = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  return (x != x) ? 0xffffffffu : k;
}
__device__ __forceinline__ float q_unkey(unsigned k) // 0xffffffff -> 0x7fffffff, a NaN
{
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

__device__ __forceinline__ float* q_out(const QuantileParams& P, int q)
{
  return P.inline_args ? P.out_inline[q] : P.tab.out[q];
}
__device__ __forceinline__ float q_p(const QuantileParams& P, int q)
{
  return P.inline_args ? P.p_inline[q] : P.tab.p[q];
}

// Batcher's odd-even merge sort on K keys, as a comparator list built at compile time
template <int K>
struct OddEvenNet
{
  template <class F>
  static constexpr int walk(F&& f)
  {
    int c = 0;
    for (int p = 1; p < K; p <<= 1)
      for (int k = p; k >= 1; k >>= 1)
        for (int j = k % p; j + k < K; j += 2 * k)
          for (int i = 0; i < k && i + j + k < K; ++i)
            if ((i + j) / (2 * p) == (i + j + k) / (2 * p))
              f(c++, i + j, i + j + k);
    return c;
  }
  struct Count
  {
    constexpr void operator()(int, int, int) const {}
  };
  static constexpr int N = walk(Count{});
  struct Tab
  {
    unsigned char a[N], b[N];
  };
  struct Fill
  {
    Tab* t;
    constexpr void operator()(int c, int x, int y) const
    {
      t->a[c] = (unsigned char)x;
      t->b[c] = (unsigned char)y;
    }
  };
  static constexpr Tab make()
  {
    Tab t{};
    walk(Fill{&t});
    return t;
  }
  static constexpr Tab tab = make();
};

template <int A, int B, int K>
__device__ __forceinline__ void q_cas(unsigned (&key)[K])
{
  const unsigned lo = min(key[A], key[B]), hi = max(key[A], key[B]);
  key[A] = lo;
  key[B] = hi;
}
template <int K, int... I>
__device__ __forceinline__ void q_sort(unsigned (&key)[K], std::integer_sequence<int, I...>)
{
  (q_cas<OddEvenNet<K>::tab.a[I], OddEvenNet<K>::tab.b[I]>(key), ...);
}

// key[r] of a register array, r uniform or not: a select tree on the bits of r.  The select is written as a bit
// blend: `bit ? key[2j + 1] : key[2j]` is folded into key[2j + bit], a dynamic index that puts the array in scratch.
template <int K>
__device__ __forceinline__ unsigned q_select(const unsigned (&key)[K], unsigned r)
{
  if constexpr (K == 1) {
    return key[0];
  } else {
    const unsigned m = 0u - (r & 1u);
    unsigned half[K / 2];
#pragma unroll
    for (int j = 0; j < K / 2; ++j)
      half[j] = (key[2 * j] & ~m) | (key[2 * j + 1] & m);
    return q_select<K / 2>(half, r >> 1);
  }
}

template <int K>
struct SortedRank
{
  const unsigned (&key)[K];
  __device__ __forceinline__ unsigned operator()(int r) const
  {
    return q_select<K>(key, (unsigned)r);
  }
};

__device__ __forceinline__ unsigned q_member_key(const QuantileParams& P, int lev, int j, long at, bool& def)
{
  const float x = arg_mem(P, j)[at];
  def = ((arg_all(P, lev, j >> 6) >> (j & 63)) & 1ull) || is_def(x, P.undef);
  return def ? q_key(x) : 0xffffffffu;
}

struct BisectRank
{
  const QuantileParams& P;
  int lev;
  long at;
  unsigned kmin, kmax; // of the counted keys
  // the r-th smallest key (r < n): the largest t with #{key < t} <= r
  __device__ __forceinline__ unsigned operator()(int r) const
  {
    if (kmin == kmax)
      return kmin;
    const int nb = 32 - __clz((int)(kmin ^ kmax)); // bits below the common prefix
    unsigned prefix = nb >= 32 ? 0u : (kmin & ~((1u << nb) - 1u));
    for (int b = nb - 1; b >= 0; --b) {
      const unsigned cand = prefix | (1u << b);
      int c = 0;
      for (int j = 0; j < P.nmem; ++j) {
        bool d;
        c += q_member_key(P, lev, j, at, d) < cand ? 1 : 0; // members that do not count (0xffffffff) never are
      }
      if (c <= r)
        prefix = cand;
    }
    return prefix;
  }
};

// percentile p of the n >= 1 counted values, rank(r) = key of the r-th smallest (include/mifc.h, "Semantics")
template <class Rank>
__device__ __forceinline__ float q_percentile(int method, int n, float p, const Rank& rank)
{
  if (method == 0) { // MIFC_QUANTILE_LOWER: float arithmetic, truncated, clamped to n - 1
    int ii = (int)(((float)n * p) / 100.0f);
    ii = ii < n - 1 ? ii : n - 1;
    return q_unkey(rank(ii));
  }
  // MIFC_QUANTILE_LINEAR: double, every step rounded (the library is built with -ffp-contract=off)
  const double h = ((double)(n - 1) * (double)p) / 100.0;
  const int k = (int)h;
  const double t = h - (double)k;
  const float xk = q_unkey(rank(k));
  if (t == 0.0)
    return xk;
  const double a = (double)xk, b = (double)q_unkey(rank(k + 1));
  return (float)(a + t * (b - a));
}

__device__ __forceinline__ void q_count(const QuantileParams& P, int l, unsigned int bad)
{
  if (P.partials)
    block_count_store(P.partials + (long)l * gridDim.x + blockIdx.x, bad);
  else
    block_count_add(P.n_undefined + P.lev0 + l, bad);
}

template <int K>
__global__ __launch_bounds__(256) void quantile_sort_kernel(const QuantileParams P)
{
  for (int l = blockIdx.y; l < P.nlev; l += gridDim.y) { // uniform per workgroup
    const u64 all = arg_all(P, P.lev0 + l, 0);
    unsigned int bad = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < P.n; i += (long)gridDim.x * 256) {
      const long at = (long)l * P.stride + i;
      // every load in flight before the first is used: no branch per member (each would end in a wait for all loads);
      // the slots past nmem load member 0 again (a cache hit) and are masked below
      float x[K];
      if (P.nmem > 0) {
#pragma unroll
        for (int j = 0; j < K; ++j)
          x[j] = arg_mem(P, j < P.nmem ? j : 0)[at];
      } else {
#pragma unroll
        for (int j = 0; j < K; ++j)
          x[j] = 0.f;
      }
      unsigned key[K];
      int n = 0;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const bool def = j < P.nmem && (((all >> j) & 1ull) || is_def(x[j], P.undef));
        n += def ? 1 : 0;
        key[j] = def ? q_key(x[j]) : 0xffffffffu;
      }
      q_sort<K>(key, std::make_integer_sequence<int, OddEvenNet<K>::N>{});
      if (n == 0) {
        bad += 1;
        for (int q = 0; q < P.nq; ++q)
          q_out(P, q)[at] = P.undef;
        continue;
      }
      const SortedRank<K> rank{key};
      for (int q = 0; q < P.nq; ++q)
        q_out(P, q)[at] = q_percentile(P.method, n, q_p(P, q), rank);
    }
    q_count(P, l, bad);
  }
}

__global__ __launch_bounds__(256) void quantile_bisect_kernel(const QuantileParams P)
{
  for (int l = blockIdx.y; l < P.nlev; l += gridDim.y) {
    const int lev = P.lev0 + l;
    unsigned int bad = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < P.n; i += (long)gridDim.x * 256) {
      const long at = (long)l * P.stride + i;
      int n = 0;
      unsigned kmin = 0xffffffffu, kmax = 0u;
      for (int j = 0; j < P.nmem; ++j) {
        bool d;
        const unsigned k = q_member_key(P, lev, j, at, d);
        if (d) {
          n += 1;
          kmin = min(kmin, k);
          kmax = max(kmax, k);
        }
      }
      if (n == 0) {
        bad += 1;
        for (int q = 0; q < P.nq; ++q)
          q_out(P, q)[at] = P.undef;
        continue;
      }
      const BisectRank rank{P, lev, at, kmin, kmax};
      for (int q = 0; q < P.nq; ++q)
        q_out(P, q)[at] = q_percentile(P.method, n, q_p(P, q), rank);
    }
    q_count(P, l, bad);
  }
}

} // namespace

hipError_t launch_quantiles(const QuantileParams& prm, hipStream_t stream)
{
  if (prm.n <= 0 || prm.nlev <= 0)
    return hipSuccess;
  const int gx = quantile_blocks(prm.n);
  const int gy = prm.nlev < 65535 ? prm.nlev : 65535;
  QuantileParams P = prm;
  // big levels: per-workgroup counts in partials[level][workgroup], added up behind the launch
  const bool parts = quantile_partials(P);
  if (!parts)
    P.partials = nullptr;
  const dim3 grid(gx, gy), block(256);
  switch (quantile_tier(P.nmem)) {
  case 8:
    hipLaunchKernelGGL(quantile_sort_kernel<8>, grid, block, 0, stream, P);
    break;
  case 16:
    hipLaunchKernelGGL(quantile_sort_kernel<16>, grid, block, 0, stream, P);
    break;
  case 32:
    hipLaunchKernelGGL(quantile_sort_kernel<32>, grid, block, 0, stream, P);
    break;
  case 64:
    hipLaunchKernelGGL(quantile_sort_kernel<64>, grid, block, 0, stream, P);
    break;
  default:
    hipLaunchKernelGGL(quantile_bisect_kernel, grid, block, 0, stream, P);
    break;
  }
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && parts)
    e = launch_count_partials_levels(P.partials, gx, P.nlev, P.n_undefined + P.lev0, stream);
  return e;
}

} // namespace mifc
