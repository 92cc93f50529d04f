// mifc_neighbour.hip -- neighbourhood statistics over [nlev][ny][nx] batches:
// neighbourProbFunctions (FieldCalculations.cc:2862-2953) and neighbourFunctions
// (:2955-3061), bit-identical to the reference.
//
// Box counts (compute 5/6 at every cell): one wave thresholds 64 cells of a row
// and keeps them as one ballot word; a lane then owns one column of a band of
// rows and keeps the window count as a running integer sum down the column (add
// the row entering, subtract the row leaving), each row's horizontal count being
// a popcount over the masked bit range [i - r, i + r].  Every input float is read
// once, every output float written once, O(1) work per cell for any range; the
// count is exact (the reference's float summed-area table is exact only while
// nx * ny <= 2^24).  The bit rows (1/32 of the field) stay in L2.
//
// Window walks (neighbourFunctions): one lane per computed centre, the window
// read from an LDS tile of the workgroup's 32 x 8 centres (plus the halo), the
// value taken in the reference's order -- row outer, column inner, one float
// chain per centre (sum from +0, strict > / < from the corner value, integer
// count) -- and written into the centre's step x step block.  A tile that would
// not fit 64 KiB of LDS reads the window from global memory instead.
// Percentile: an exact order statistic by bisection over order-preserving uint32
// keys (#{key < t} <= ii, bit by bit below the common prefix of the window's
// min and max key), so there is no cap on the window.
#include "mifc_kernels.h"

namespace mifc {

namespace {

const int NB_BX = 32, NB_BY = 8; // centres per workgroup of the window kernel (wave = two 32-centre rows)
const int NB_LDS_MAX = 64 * 1024;

__device__ __forceinline__ bool nb_hit(float f, int compute, float limit)
{
  return compute == 5 ? (f > limit) : (f < limit); // a NaN is never counted
}

// one wave per 64-cell word of a row; grid.x covers ny * nwords words in fours, grid.y the levels
__global__ __launch_bounds__(256) void nb_bits_kernel(NeighbourParams P)
{
  const int nwords = neighbour_words(P.nx);
  const long w = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= (long)P.ny * nwords) // wave-uniform
    return;
  const int lane = threadIdx.x & 63;
  const int j = (int)(w / nwords);
  const int i = (int)(w - (long)j * nwords) * 64 + lane;
  bool hit = false;
  if (i < P.nx)
    hit = nb_hit(P.in[(long)blockIdx.y * P.level_stride + (long)j * P.nx + i], P.compute, P.limit);
  const u64 m = __ballot(hit);
  if (lane == 0)
    P.bits[(long)blockIdx.y * P.ny * nwords + w] = m;
}

// cells lo..hi (inclusive, 0 <= lo <= hi < nx) of one bit row
__device__ __forceinline__ int nb_row_count(const u64* row, int lo, int hi)
{
  const int wlo = lo >> 6, whi = hi >> 6;
  const u64 mlo = ~0ull << (lo & 63);
  const u64 mhi = ~0ull >> (63 - (hi & 63));
  if (wlo == whi)
    return __popcll(row[wlo] & mlo & mhi);
  int c = __popcll(row[wlo] & mlo) + __popcll(row[whi] & mhi);
  for (int w = wlo + 1; w < whi; ++w)
    c += __popcll(row[w]);
  return c;
}

// lane = column, workgroup = 256 columns x `band` rows of one level
__global__ __launch_bounds__(256) void nb_box_kernel(NeighbourParams P, int band)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P.nx)
    return;
  const int nwords = neighbour_words(P.nx);
  const int r = P.range, ny = P.ny, nx = P.nx;
  const u64* bits = P.bits + (long)blockIdx.z * ny * nwords;
  float* out = P.out + (long)blockIdx.z * P.level_stride + i;
  const int j0 = blockIdx.y * band, j1 = min(j0 + band, ny);
  const bool col_in = i >= r && i < nx - r;
  int s = 0;
  bool started = false;
  for (int j = j0; j < j1; ++j) {
    float v = P.undef; // :2928-2950
    if (col_in && j >= r && j < ny - r) {
      if (!started) {
        for (int k = j - r; k <= j + r; ++k)
          s += nb_row_count(bits + (long)k * nwords, i - r, i + r);
        started = true;
      } else {
        s += nb_row_count(bits + (long)(j + r) * nwords, i - r, i + r) - nb_row_count(bits + (long)(j - r - 1) * nwords, i - r, i + r);
      }
      v = (float)s / P.nf; // :2924 fres /= N, the count being an exact integer
    }
    out[(long)j * nx] = v;
  }
}

__global__ __launch_bounds__(256) void nb_threshold_kernel(NeighbourParams P, long n)
{
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k < n)
    P.out[k] = nb_hit(P.in[k], P.compute, P.limit) ? 1.f : 0.f; // :2881-2890
}

// neighbourFunctions :2988-3005: rows j < r and j >= ny - r whole, columns i < r and i >= nx - r of the rows between.
// One 64-lane workgroup per (row, level).
__global__ __launch_bounds__(64) void nb_border_kernel(NeighbourParams P)
{
  const int j = blockIdx.x, nx = P.nx, r = P.range;
  float* row = P.out + (long)blockIdx.y * P.level_stride + (long)j * nx;
  if (j < r || j >= P.ny - r || nx <= 2 * r) {
    for (int i = threadIdx.x; i < nx; i += 64)
      row[i] = P.undef;
  } else {
    for (int c = threadIdx.x; c < 2 * r; c += 64)
      row[c < r ? c : nx - 2 * r + c] = P.undef;
  }
}

__device__ __forceinline__ unsigned nb_key(float f) // order-preserving: a < b  <=>  key(a) < key(b) (no NaN; -0 < +0)
{
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float nb_unkey(unsigned k)
{
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

template <int OP, bool LDS>
__device__ __forceinline__ unsigned nb_load_key(const float* src, const unsigned* keys, long at)
{
  return LDS ? keys[at] : nb_key(src[at]);
}

// OP: 1 mean, 2 max, 3 min, 4 percentile, 5 / 6 count, 0 anything else (+0).  LDS: window from the workgroup's tile.
template <int OP, bool LDS>
__global__ __launch_bounds__(256) void nb_window_kernel(NeighbourParams P, int ncx, int ncy)
{
  extern __shared__ float nb_tile[];
  const int nx = P.nx, r = P.range, st = P.step, w = 2 * r + 1;
  const float* in = P.in + (long)blockIdx.z * P.level_stride;
  float* out = P.out + (long)blockIdx.z * P.level_stride;
  const int tx = threadIdx.x % NB_BX, ty = threadIdx.x / NB_BX;
  const int mx = blockIdx.x * NB_BX + tx, my = blockIdx.y * NB_BY + ty;
  // the workgroup's first centre is (r + x0, r + y0): its window starts at (x0, y0)
  const int x0 = blockIdx.x * NB_BX * st, y0 = blockIdx.y * NB_BY * st;
  const float* src;
  long pitch;
  if (LDS) {
    const int tw = min((NB_BX - 1) * st + w, nx - x0), th = min((NB_BY - 1) * st + w, P.ny - y0);
    const int lane = threadIdx.x & 63;
    for (int row = threadIdx.x >> 6; row < th; row += 4) {
      const float* g = in + (long)(y0 + row) * nx + x0;
      for (int c = lane; c < tw; c += 64) {
        const float f = g[c];
        if (OP == 4)
          reinterpret_cast<unsigned*>(nb_tile)[row * tw + c] = nb_key(f);
        else
          nb_tile[row * tw + c] = f;
      }
    }
    __syncthreads();
    src = nb_tile + (long)ty * st * tw + tx * st;
    pitch = tw;
  } else {
    src = in + (long)(y0 + ty * st) * nx + x0 + tx * st;
    pitch = nx;
  }
  if (mx >= ncx || my >= ncy)
    return;
  float v = 0.f; // :3015
  if (OP == 1 || OP == 2 || OP == 3 || OP == 5 || OP == 6) {
    if (OP == 2 || OP == 3)
      v = src[0]; // :3016-3018, the window's corner
    int cnt = 0;
    for (int k = 0; k < w; ++k) {
      const float* rowp = src + k * pitch;
      for (int l = 0; l < w; ++l) {
        const float t = rowp[l];
        if (OP == 1)
          v += t;
        if (OP == 2 && t > v) // strict compares: not fmaxf / fminf (NaN and signed zeros)
          v = t;
        if (OP == 3 && t < v)
          v = t;
        if ((OP == 5 && t > P.limit) || (OP == 6 && t < P.limit))
          cnt++;
      }
    }
    if (OP == 5 || OP == 6)
      v = (float)cnt;
    if (OP == 1 || OP == 5 || OP == 6)
      v = v / P.nf; // :3038-3040
  } else if (OP == 4) {
    // the ii-th smallest key: the largest t with #{key < t} <= ii, built bit by bit
    const unsigned* keys = reinterpret_cast<const unsigned*>(src);
    unsigned kmin = 0xffffffffu, kmax = 0u;
    for (int k = 0; k < w; ++k)
      for (int l = 0; l < w; ++l) {
        const unsigned key = nb_load_key<OP, LDS>(src, keys, (long)k * pitch + l);
        kmin = min(kmin, key);
        kmax = max(kmax, key);
      }
    unsigned t = kmin;
    if (kmin != kmax) {
      const int nb = 32 - __clz(kmin ^ kmax); // bits below the common prefix
      unsigned prefix = nb >= 32 ? 0u : (kmin & ~((1u << nb) - 1u));
      for (int b = nb - 1; b >= 0; --b) {
        const unsigned cand = prefix | (1u << b);
        int c = 0;
        for (int k = 0; k < w; ++k)
          for (int l = 0; l < w; ++l)
            c += nb_load_key<OP, LDS>(src, keys, (long)k * pitch + l) < cand ? 1 : 0;
        if (c <= P.ii)
          prefix = cand;
      }
      t = prefix;
    }
    v = nb_unkey(t);
  } // any other compute: the untouched +0 (divided by N when compute > 4, :3038-3040, still +0)
  // :3043-3048: the centre's step x step block, inside the field because step / 2 <= range
  const int cx = r + mx * st, cy = r + my * st;
  for (int y = cy - (st - 1) / 2; y <= cy + st / 2; ++y) {
    float* o = out + (long)y * nx;
    for (int x = cx - (st - 1) / 2; x <= cx + st / 2; ++x)
      o[x] = v;
  }
}

template <int OP>
hipError_t nb_launch_window(const NeighbourParams& P, int ncx, int ncy, hipStream_t stream)
{
  const dim3 grid((ncx + NB_BX - 1) / NB_BX, (ncy + NB_BY - 1) / NB_BY, P.nlev);
  const long tw = (long)(NB_BX - 1) * P.step + 2 * P.range + 1, th = (long)(NB_BY - 1) * P.step + 2 * P.range + 1;
  const long lds = tw * th * 4;
  if (OP != 0 && lds <= NB_LDS_MAX)
    hipLaunchKernelGGL((nb_window_kernel<OP, true>), grid, dim3(256), (size_t)lds, stream, P, ncx, ncy);
  else
    hipLaunchKernelGGL((nb_window_kernel<OP, false>), grid, dim3(256), 0, stream, P, ncx, ncy);
  return hipGetLastError();
}

} // namespace

hipError_t launch_neighbour_threshold(const NeighbourParams& P, hipStream_t stream)
{
  const long n = (long)P.nlev * P.level_stride;
  if (n <= 0)
    return hipSuccess;
  hipLaunchKernelGGL(nb_threshold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, P, n);
  return hipGetLastError();
}

hipError_t launch_neighbour_box(const NeighbourParams& P, hipStream_t stream)
{
  if (P.nx <= 0 || P.ny <= 0 || P.nlev <= 0)
    return hipSuccess;
  const long words = (long)P.ny * neighbour_words(P.nx);
  hipLaunchKernelGGL(nb_bits_kernel, dim3((unsigned)((words + 3) / 4), P.nlev), dim3(256), 0, stream, P);
  // a band's start-up sums 2r + 1 rows: bands several windows tall keep that a small share
  const int band = 2 * P.range + 1 <= 16 ? 64 : (2 * P.range + 1 <= 48 ? 128 : 256);
  hipLaunchKernelGGL(nb_box_kernel, dim3((P.nx + 255) / 256, (P.ny + band - 1) / band, P.nlev), dim3(256), 0, stream, P, band);
  return hipGetLastError();
}

hipError_t launch_neighbour_functions(const NeighbourParams& P, hipStream_t stream)
{
  if (P.nx <= 0 || P.ny <= 0 || P.nlev <= 0)
    return hipSuccess;
  hipLaunchKernelGGL(nb_border_kernel, dim3(P.ny, P.nlev), dim3(64), 0, stream, P);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess)
    return e;
  // centres i = r, r + step, ... < nx - r (:3009-3010)
  const int ncx = P.nx > 2 * P.range ? (P.nx - 2 * P.range + P.step - 1) / P.step : 0;
  const int ncy = P.ny > 2 * P.range ? (P.ny - 2 * P.range + P.step - 1) / P.step : 0;
  if (ncx == 0 || ncy == 0)
    return hipSuccess;
  switch (P.compute) {
  case 1:
    return nb_launch_window<1>(P, ncx, ncy, stream);
  case 2:
    return nb_launch_window<2>(P, ncx, ncy, stream);
  case 3:
    return nb_launch_window<3>(P, ncx, ncy, stream);
  case 4:
    return nb_launch_window<4>(P, ncx, ncy, stream);
  case 5:
    return nb_launch_window<5>(P, ncx, ncy, stream);
  case 6:
    return nb_launch_window<6>(P, ncx, ncy, stream);
  default:
    return nb_launch_window<0>(P, ncx, ncy, stream);
  }
}

} // namespace mifc
