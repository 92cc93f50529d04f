// mifc_htraj.hip -- particles carried by the wind of a level through a series of slices (mifc_htraj_levels,
// include/mifc.h; EXTENSION: the reference's callers integrate on the host, slice by slice).
//
// An iterated gather.  A lane owns one particle of one level for a whole interval: its position stays in two double
// registers through all nsub * (1 + niter) evaluations of the index velocity, each of which needs the four corners of u
// and v in both slices and of the two map planes at a position that the evaluation before produced -- a dependent chain,
// bound by the latency of a gather, not by bandwidth.  What hides it is the number of chains in flight: a workgroup is 256
// particles of ONE level (grid.y walks the levels, htraj_level_chunk), and within an evaluation all 24 loads are issued
// before the first value is used.  They can be, because the offsets are made safe instead of the loads conditional
// (mifc_htraj_rules.h): a corner that is not needed is read from the corner beside it, a lost or surplus lane reads cell 0,
// and the cell is clamped into the grid after the inside test -- nothing outside a plane is read, whatever the position.
// The level is wave-uniform: the planes' bases are 64-bit scalars, a lane adds its 32-bit cell offset.  At the end of the
// interval a lane stores x and y (one coalesced dword each), samples the trace fields of slice B at the float position it
// stored, and the wave counts its lost particles and its trace holes by ballot + popcount, one atomic per wave and only
// where the count is not zero (as the hinterp kernel counts holes).  The arithmetic is the text of mifc_htraj_rules.h,
// which the host compiler builds for the tests.
#include "mifc_column_walk.h"
#include "mifc_device.h"
#include "mifc_env.h"
#include "mifc_kernels.h"

#define MIFC_HTRAJ_FN __host__ __device__ __forceinline__
#include "mifc_htraj_rules.h"

namespace mifc {

namespace {

template <bool TESTED, bool TRACE>
__global__ __launch_bounds__(256) void htraj_kernel(const HtrajParams P)
{
  const int nx = P.nx, ny = P.ny;
  const float undef = P.undef;
  const unsigned int p = blockIdx.x * 256u + threadIdx.x;
  const bool mine = p < (unsigned int)P.npos;
  const unsigned int pr = mine ? p : 0u; // (a surplus lane reads particle 0 and cell 0 and writes nothing)
  const bool lane0 = (threadIdx.x & 63) == 0;
  const ConstWords bits = (ConstWords)(unsigned long long)P.bits;

  // one slot of one level (e = 0: the slot the interval starts from, written by the first launch only, with the trace
  // fields of slice A; e = 1: the slot it ends in, slice B): the position or undef, the lost particles counted, the trace
  // fields at the float position
  auto emit = [&](int e, int k, float x, float y, bool live, unsigned int trace_all) {
    // What only a slot needs is read from the kernel's arguments HERE (P is the kernel's one argument: it starts the
    // segment), through a pointer the compiler cannot see through: hoisted in front of the evaluation loop, these scalars
    // did not fit beside what the loop holds, and the tested instance with trace fields spilled twelve of them.
    const __attribute__((address_space(4))) HtrajParams* S = (const __attribute__((address_space(4))) HtrajParams*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(S));
    const long at = (long)e * S->slot_stride + (long)k * (long)S->npos;
    if (mine) {
      (S->x + at)[p] = live ? x : undef;
      (S->y + at)[p] = live ? y : undef;
    }
    const u64 lost = __builtin_amdgcn_ballot_w64(mine && !live);
    if (lost != 0 && lane0)
      atomicAdd(S->counts + (long)e * S->call_nlev + k, (u64)__popcll(lost));
    if constexpr (TRACE) {
      const int ntrace = S->ntrace;
#pragma unroll 1
      for (int f = 0; f < ntrace; ++f) { // wave-uniform; the fields one after the other: a slot is written once per interval
        bool hole;
        const float* plane = S->trace[HTRAJ_MAX_TRACE * e + f] + (long)k * S->in_stride;
        const float r = htraj_trace<TESTED>(plane, x, y, mine && live, ((trace_all >> f) & 1u) != 0, undef, nx, ny, hole);
        if (mine)
          (S->t[f] + at)[p] = r;
        if constexpr (TESTED) {
          const u64 m = __builtin_amdgcn_ballot_w64(hole);
          if (m != 0 && lane0)
            atomicAdd(S->counts + ((long)(1 + f) * S->nslots + e) * S->call_nlev + k, (u64)__popcll(m));
        }
      }
    }
  };

  const int k_begin = (int)blockIdx.y * P.chunk, k_end = min(P.nlev, k_begin + P.chunk);
  for (int k = k_begin; k < k_end; ++k) {
    unsigned int all = ~0u;
    if constexpr (TESTED)
      all = bits[k];
    const long lev = (long)k * P.in_stride; // wave-uniform, 64-bit
    const HtrajWind W = {P.uA + lev, P.uB + lev, P.vA + lev, P.vB + lev, P.xmapr, P.ymapr, all, nx, ny, undef};

    // rule 1 (the first interval) or the slot the interval before left: an undef there is a lost particle
    const long from = P.first != 0 ? 0L : (long)k * (long)P.npos; // (the start positions are shared by all levels)
    const float x0 = ((P.first != 0 ? P.xpos0 : P.x) + from)[pr], y0 = ((P.first != 0 ? P.ypos0 : P.y) + from)[pr];
    bool live = mine && htraj_usable(x0, y0, undef, nx, ny);
    if (P.first != 0)
      emit(0, k, x0, y0, live, all >> HTRAJ_TRACE_A_BIT);

    double xd = (double)x0, yd = (double)y0;
    live = htraj_interval<TESTED>(W, P.tau, P.nsub, P.niter, xd, yd, live);
    emit(1, k, (float)xd, (float)yd, live, all >> HTRAJ_TRACE_B_BIT); // rule 5: the state passes through float
  }
}

template <bool TESTED>
hipError_t launch_trace(const HtrajParams& P, hipStream_t stream)
{
  const dim3 grid((unsigned int)(((long)P.npos + 255) / 256), (unsigned int)((P.nlev + P.chunk - 1) / P.chunk)), block(256);
  if (P.ntrace > 0)
    hipLaunchKernelGGL((htraj_kernel<TESTED, true>), grid, block, 0, stream, P);
  else
    hipLaunchKernelGGL((htraj_kernel<TESTED, false>), grid, block, 0, stream, P);
  return hipGetLastError();
}

} // namespace

hipError_t launch_htraj(const HtrajParams& prm, hipStream_t stream)
{
  if (prm.npos < 1 || prm.nlev < 1 || prm.nx < 1 || prm.ny < 1 || prm.nx > HTRAJ_MAX_EDGE || prm.ny > HTRAJ_MAX_EDGE ||
      (long)prm.nx * (long)prm.ny > 0x7fffffffL || prm.nlev > prm.call_nlev || prm.nslots < 2 ||
      prm.nsub < 1 || prm.nsub > HTRAJ_MAX_NSUB || prm.niter < 0 || prm.niter > HTRAJ_MAX_NITER || prm.ntrace < 0 || prm.ntrace > HTRAJ_MAX_TRACE)
    return hipErrorInvalidValue;
  HtrajParams P = prm;
  P.chunk = htraj_level_chunk(P.nlev, env().htraj_level_chunk);
  return P.tested ? launch_trace<true>(P, stream) : launch_trace<false>(P, stream);
}

} // namespace mifc
