// mifc_hinterp.hip -- level batches sampled at arbitrary points: nearest, bilinear, bicubic (mifc_hinterp_levels,
// include/mifc.h; EXTENSION: the reference's callers interpolate on the host).
//
// Every other kernel of the library streams contiguous rows; this one gathers.  A lane owns one point for the whole walk:
// it works out the cell, the fractions a and b, the cubic weights, the cell offsets of the values it needs and the two
// predicates "position unusable" and "cubic block inside" ONCE, then walks the levels of its workgroup's chunk and the
// fields of the launch.  Per level the address is a wave-uniform 64-bit base (field pointer + level * stride, scalar
// registers) plus the lane's 32-bit cell offset, so the level loop advances scalar registers only.  A gather is bound by
// latency, not by bandwidth: the level loop is unrolled twice with registers of their own, all loads of two levels and of
// every field of the launch are issued before the first value is used.  The offsets are made safe instead of the loads
// conditional: a lane that does not need column i0 + 1 (a == 0) or row j0 + 1 (b == 0) reads column i0 / row j0 again, a
// lane outside the launch or with an unusable position reads cell 0, a lane whose cubic block is not inside the grid
// folds the block onto the cell's four corners -- so the loads are straight-line code and nothing outside the grid is read.
// Stores are one dword per lane, consecutive lanes consecutive points: coalesced.  No LDS.  Cells left undef are counted
// per level and field by ballot + popcount, one atomic per wave and only where the count is not zero; unusable positions
// are the same for every level and field and are counted once, into one counter that the host adds to all
// (DESIGN.md 4.8, 4.20).
#include "mifc_column_walk.h"
#include "mifc_device.h"
#include "mifc_env.h"
#include "mifc_kernels.h"

#include <algorithm>
#include <type_traits>

namespace mifc {

namespace {

// rule 6: the Catmull-Rom weights of the columns i0 - 1 .. i0 + 2 (rows j0 - 1 .. j0 + 2) for the fraction t
__device__ __forceinline__ void cubic_weights(double t, double (&w)[4])
{
  w[0] = ((-0.5 * t + 1.0) * t - 0.5) * t;
  w[1] = ((1.5 * t - 2.5) * t) * t + 1.0;
  w[2] = ((-1.5 * t + 2.0) * t + 0.5) * t;
  w[3] = ((0.5 * t - 0.5) * t) * t;
}

// ROTATE: the fields of the launch are pairs; both components are sampled, then rotated by rule R with the point's coefficients
template <int METHOD, int NF, bool TESTED, bool ROTATE = false>
__global__ __launch_bounds__(256) void hinterp_kernel(const std::conditional_t<ROTATE, HinterpRotateParams, HinterpParams> P)
{
  static_assert(!ROTATE || NF % 2 == 0, "a pair stays in one launch");
  // values per (field, level): the node | the four corners | the 4 x 4 block, rows j0 - 1 .. j0 + 2 by columns i0 - 1 .. i0 + 2
  constexpr int NV = METHOD == HINTERP_NEAREST ? 1 : (METHOD == HINTERP_BILINEAR ? 4 : 16);
  // where the corners (j0, i0), (j0, i0 + 1), (j0 + 1, i0), (j0 + 1, i0 + 1) are among them
  constexpr int C00 = METHOD == HINTERP_BICUBIC ? 5 : 0, C10 = C00 + 1, C01 = METHOD == HINTERP_BICUBIC ? 9 : 2, C11 = C01 + 1;
  const int nx = P.nx, ny = P.ny;
  const float undef = P.undef;
  const unsigned int p = blockIdx.x * 256u + threadIdx.x;
  const bool mine = p < (unsigned int)P.npos;
  const bool lane0 = (threadIdx.x & 63) == 0;

  // rule 1, once per point
  const float x = P.xpos[mine ? p : 0u], y = P.ypos[mine ? p : 0u];
  const double xd = (double)x, yd = (double)y;
  bool usable = all_def(undef, x, y) && xd >= 0.0 && xd <= (double)(nx - 1) && yd >= 0.0 && yd <= (double)(ny - 1);
  double rc = 0.0, rs = 0.0; // rule R1, once per point, next to the position: undefined coefficients make the position unusable
  if constexpr (ROTATE) {
    const float cf = P.cosa[mine ? p : 0u], sf = P.sina[mine ? p : 0u];
    usable &= P.rot_all != 0 || all_def(undef, cf, sf);
    rc = (double)cf;
    rs = (double)sf;
  }
  const bool sampled = mine && usable; // the lane's results are computed values or counted holes
  const double xs = sampled ? xd : 0.0, ys = sampled ? yd : 0.0; // (every other lane reads cell 0 and throws it away)
  if (P.count_unusable != 0 && blockIdx.y == 0) {
    const u64 m = __builtin_amdgcn_ballot_w64(mine && !usable);
    if (m != 0 && lane0)
      atomicAdd(P.n_unusable, (u64)__popcll(m));
  }

  // rule 2, once per point: the cell, the fractions, the offsets of the values (cells from the level's base; nx * ny < 2^31)
  const int i0 = (int)xs, j0 = (int)ys;
  const double a = xs - (double)i0, b = ys - (double)j0;
  const bool a0 = a == 0.0, b0 = b == 0.0;
  int off[NV];
  bool cubic_inside = false;
  double wx[4], wy[4];
  if constexpr (METHOD == HINTERP_NEAREST) {
    off[0] = (int)(ys + 0.5) * nx + (int)(xs + 0.5); // rule 4
  } else {
    const int o00 = j0 * nx + i0, dx = a0 ? 0 : 1, dy = b0 ? 0 : nx; // a != 0: i0 + 1 <= nx - 1; b != 0: j0 + 1 <= ny - 1
    if constexpr (METHOD == HINTERP_BILINEAR) {
      off[0] = o00;
      off[1] = o00 + dx;
      off[2] = o00 + dy;
      off[3] = o00 + dy + dx;
    } else {
      cubic_inside = !(a0 && b0) && i0 >= 1 && i0 <= nx - 3 && j0 >= 1 && j0 <= ny - 3;
      const int col[4] = {cubic_inside ? -1 : 0, 0, cubic_inside ? 1 : dx, cubic_inside ? 2 : dx};
      const int row[4] = {cubic_inside ? -nx : 0, 0, cubic_inside ? nx : dy, cubic_inside ? 2 * nx : dy};
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n)
          off[4 * m + n] = o00 + row[m] + col[n];
      cubic_weights(a, wx);
      cubic_weights(b, wy);
    }
  }

  const ConstWords lev_bits = (ConstWords)(unsigned long long)P.lev_bits;

  // one value of one (field, level): rules 3 to 6; bad: the result is a hole (counted unless the position is unusable)
  auto result = [&](const float (&v)[NV], bool all, bool& bad) -> float {
    const bool untested = !TESTED || all; // wave-uniform
    if constexpr (METHOD == HINTERP_NEAREST) {
      bad = !(untested || is_def(v[0], undef));
      return bad ? undef : v[0];
    } else {
      const bool d00 = untested || is_def(v[C00], undef), d10 = untested || is_def(v[C10], undef);
      const bool d01 = untested || is_def(v[C01], undef), d11 = untested || is_def(v[C11], undef);
      bool ok = d00 & (a0 | d10) & (b0 | d01) & (a0 | b0 | d11); // rule 5: the corners that are needed
      const double x00 = (double)v[C00], x10 = (double)v[C10], x01 = (double)v[C01], x11 = (double)v[C11];
      const double e0 = x10 - x00, e1 = x11 - x01;
      const double g0 = a * e0, g1 = a * e1;
      const double s0 = x00 + g0, s1 = x01 + g1;
      const double r0 = a0 ? x00 : s0, r1 = a0 ? x01 : s1;
      const double er = r1 - r0;
      const double gr = b * er;
      const double sr = r0 + gr;
      float res = (float)(b0 ? r0 : sr);
      if constexpr (METHOD == HINTERP_BICUBIC) {
        bool cubic = cubic_inside;
        if (!untested) {
          bool every = true;
#pragma unroll
          for (int n = 0; n < NV; ++n)
            every &= is_def(v[n], undef);
          cubic &= every;
        }
        if (__builtin_amdgcn_ballot_w64(cubic) != 0) { // rule 6
          double s[4];
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            const double t0 = wx[0] * (double)v[4 * m], t1 = wx[1] * (double)v[4 * m + 1], t2 = wx[2] * (double)v[4 * m + 2],
                         t3 = wx[3] * (double)v[4 * m + 3];
            const double u0 = t0 + t1;
            const double u1 = u0 + t2;
            s[m] = u1 + t3;
          }
          const double t0 = wy[0] * s[0], t1 = wy[1] * s[1], t2 = wy[2] * s[2], t3 = wy[3] * s[3];
          const double u0 = t0 + t1;
          const double u1 = u0 + t2;
          const double rc = u1 + t3;
          res = cubic ? (float)rc : res;
          ok |= cubic;
        }
      }
      bad = !ok;
      return bad ? undef : res;
    }
  };

  // U levels from level k of the launch on: every load first, then the values
  auto levels = [&](auto count, int k) {
    constexpr int U = decltype(count)::value;
    float v[U][NF][NV];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int f = 0; f < NF; ++f) {
        const float* level = P.fields[f] + (long)(k + u) * P.in_stride; // wave-uniform, 64-bit
#pragma unroll
        for (int n = 0; n < NV; ++n)
          v[u][f][n] = level[off[n]];
      }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kc = P.lev0 + k + u; // the call's level
      unsigned int bits = 0;
      if constexpr (TESTED)
        bits = lev_bits[kc] >> P.f0;
      if constexpr (ROTATE) {
#pragma unroll
        for (int f = 0; f < NF; f += 2) { // the pair (f, f + 1): each component by rules 3 to 6 and rounded to float, then rule R
          bool bad_u, bad_v;
          const float su = result(v[u][f], ((bits >> f) & 1u) != 0, bad_u), sv = result(v[u][f + 1], ((bits >> (f + 1)) & 1u) != 0, bad_v);
          const bool bad = bad_u | bad_v;
          const double ud = (double)su, vd = (double)sv;
          const double cu = rc * ud, svv = rs * vd, suu = rs * ud, cv = rc * vd;
          const double ra = cu - svv, rb = suu + cv;
          const bool hole = bad | !usable;
          const float r0 = hole ? undef : (float)ra, r1 = hole ? undef : (float)rb;
          if constexpr (TESTED) {
            const u64 m = __builtin_amdgcn_ballot_w64(bad && sampled);
            if (m != 0 && lane0)
              atomicAdd(P.n_undefined + (long)((P.f0 + f) / 2) * P.call_nlev + kc, (u64)__popcll(m));
          }
          if (mine) {
            (P.out[f] + (long)(k + u) * P.out_stride)[p] = r0;
            (P.out[f + 1] + (long)(k + u) * P.out_stride)[p] = r1;
          }
        }
      } else {
#pragma unroll
        for (int f = 0; f < NF; ++f) {
          bool bad;
          float r = result(v[u][f], ((bits >> f) & 1u) != 0, bad);
          r = usable ? r : undef;
          if constexpr (TESTED) {
            const u64 m = __builtin_amdgcn_ballot_w64(bad && sampled);
            if (m != 0 && lane0)
              atomicAdd(P.n_undefined + (long)(P.f0 + f) * P.call_nlev + kc, (u64)__popcll(m));
          }
          if (mine)
            (P.out[f] + (long)(k + u) * P.out_stride)[p] = r;
        }
      }
    }
  };

  const int k_begin = (int)blockIdx.y * P.chunk, k_end = min(P.nlev, k_begin + P.chunk);
  int k = k_begin;
  for (; k + HINTERP_UNROLL <= k_end; k += HINTERP_UNROLL)
    levels(std::integral_constant<int, HINTERP_UNROLL>(), k);
  for (; k < k_end; ++k)
    levels(std::integral_constant<int, 1>(), k);
}

template <int METHOD, int NF, class Params>
hipError_t launch_tested(const Params& P, hipStream_t stream)
{
  constexpr bool ROTATE = std::is_same<Params, HinterpRotateParams>::value;
  const dim3 grid((unsigned int)(((long)P.npos + 255) / 256), (unsigned int)((P.nlev + P.chunk - 1) / P.chunk)), block(256);
  if (P.tested)
    hipLaunchKernelGGL((hinterp_kernel<METHOD, NF, true, ROTATE>), grid, block, 0, stream, P);
  else
    hipLaunchKernelGGL((hinterp_kernel<METHOD, NF, false, ROTATE>), grid, block, 0, stream, P);
  return hipGetLastError();
}

template <int METHOD, class Params>
hipError_t launch_nf(const Params& P, hipStream_t stream)
{
  static_assert(HINTERP_PASS == 4 && HINTERP_PASS_BICUBIC == 2, "one case per field count of a launch");
  constexpr bool ROTATE = std::is_same<Params, HinterpRotateParams>::value; // (pairs: no instances with an odd field count)
  switch (P.nfields) {
  case 1:
    if constexpr (!ROTATE)
      return launch_tested<METHOD, 1>(P, stream);
    return hipErrorInvalidValue;
  case 2:
    return launch_tested<METHOD, 2>(P, stream);
  case 3:
    if constexpr (hinterp_pass_fields(METHOD) >= 3 && !ROTATE)
      return launch_tested<METHOD, 3>(P, stream);
    return hipErrorInvalidValue; // (the instances beyond a launch's capacity do not exist)
  case 4:
    if constexpr (hinterp_pass_fields(METHOD) >= 4)
      return launch_tested<METHOD, 4>(P, stream);
    return hipErrorInvalidValue;
  default:
    return hipErrorInvalidValue;
  }
}

} // namespace

HinterpPlan hinterp_plan(int npos, int nlev)
{
  // Measured (profiles/README.md, "the levels per workgroup"): with few points the call is fastest with many short
  // workgroups -- a CU holds eight of these four-wave workgroups, and a launch that only just covers the CUs once pays
  // for every workgroup the dispatcher doubles up -- so the target is eight workgroups per CU, in chunks of
  // HINTERP_UNROLL levels at least.
  const int wanted_workgroups = 8 * 256, max_grid_y = 65535;
  const int blocks = (int)(((long)npos + 255) / 256);
  const int wanted = std::min(nlev, std::max(1, (wanted_workgroups + blocks - 1) / blocks)); // level chunks
  int chunk = nlev / wanted;
  chunk = std::max(chunk, std::min(nlev, HINTERP_UNROLL));
  if (env().hinterp_level_chunk > 0)
    chunk = std::min(nlev, env().hinterp_level_chunk);
  chunk = std::max(chunk, (nlev + max_grid_y - 1) / max_grid_y);
  return {blocks, chunk, (nlev + chunk - 1) / chunk};
}

namespace {

template <class Params>
hipError_t launch_checked(const Params& prm, hipStream_t stream)
{
  if (prm.npos < 1 || prm.nlev < 1 || prm.nx < 1 || prm.ny < 1 || (long)prm.nx * (long)prm.ny > 0x7fffffffL || prm.f0 < 0 ||
      prm.f0 + prm.nfields > HINTERP_MAX_FIELDS || prm.lev0 < 0 || prm.lev0 + prm.nlev > prm.call_nlev)
    return hipErrorInvalidValue;
  Params P = prm;
  P.chunk = hinterp_plan(P.npos, P.nlev).chunk;
  switch (P.method) {
  case HINTERP_NEAREST:
    return launch_nf<HINTERP_NEAREST>(P, stream);
  case HINTERP_BILINEAR:
    return launch_nf<HINTERP_BILINEAR>(P, stream);
  case HINTERP_BICUBIC:
    return launch_nf<HINTERP_BICUBIC>(P, stream);
  default:
    return hipErrorInvalidValue;
  }
}

} // namespace

hipError_t launch_hinterp(const HinterpParams& prm, hipStream_t stream)
{
  return launch_checked(prm, stream);
}

hipError_t launch_hinterp_rotate(const HinterpRotateParams& prm, hipStream_t stream)
{
  if ((prm.f0 & 1) != 0 || (prm.nfields & 1) != 0 || !prm.cosa || !prm.sina)
    return hipErrorInvalidValue;
  return launch_checked(prm, stream);
}

} // namespace mifc
