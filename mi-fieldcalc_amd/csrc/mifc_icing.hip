// mifc_icing.hip -- the iterative vessel-icing models, vesselIcingModStall (FieldCalculationsVesselIcing.cc:182-337) and
// vesselIcingMincog (:466-705), over [nlev][ny][nx] batches.
//
// One lane per cell, grid-stride over the cells of a level, grid.y over the levels.  A cell reads its 11 inputs and
// writes one float; no LDS beyond the undefined count.  The per-cell arithmetic is mifc_icing_cell.h, the same text
// the host restatement compiles, with the reference's loop trip counts: the lanes of a wave diverge in the
// shallow-water and freezing-fraction loops, and that is kept.  The inputs are read before the
// output is written, so `out` may be any input of its own level.
#include "mifc_device.h"
#include "mifc_icing_cell.h"
#include "mifc_kernels.h"

namespace mifc {

namespace {

// the level factor k: from the kernel arguments (uniform index: a scalar load) or from the buffer
struct LevelTab
{
  const IcingParams& P;
  __device__ __forceinline__ double operator[](int k) const { return P.lev_buf ? P.lev_buf[k] : P.lev[k]; }
};

template <int MODEL>
__global__ __launch_bounds__(256) void vessel_icing_kernel(IcingParams P)
{
  mifc_icing::IcingConsts C;
  C.model = P.model;
  C.alt = P.alt;
  C.number = P.number;
  C.bisect_iter = P.bisect_iter;
  C.vs = P.vs;
  C.vs_cos_d = P.vs_cos_d;
  C.cos_d = P.cos_d;
  C.cos_alpha = P.cos_alpha;
  C.sin_beta = P.sin_beta;
  C.drag = P.drag;
  C.Swdown = P.Swdown;
  for (int k = 0; k < 2; ++k) {
    C.br_sin2[k] = P.br_sin2[k];
    C.br_cos[k] = P.br_cos[k];
    C.br_cos2[k] = P.br_cos2[k];
  }
  const LevelTab E = {P};
  mifc_icing::NoTrips tr;
  for (int l = blockIdx.y; l < P.nlev; l += gridDim.y) { // uniform per workgroup
    const bool all = P.all_defined[l] != 0;
    unsigned int bad = 0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < P.n; i += (long)gridDim.x * blockDim.x) {
      float x[11];
#pragma unroll
      for (int k = 0; k < 11; ++k)
        x[k] = P.in[k][(long)l * P.in_stride[k] + i];
      float r;
      if (mifc_icing::icing_defined(MODEL, all, x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[9], x[10], P.undef)) {
        if (MODEL == mifc_icing::MODSTALL)
          r = mifc_icing::modstall_cell(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8], x[10], C, E, tr);
        else
          r = mifc_icing::mincog_cell(x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], x[8], x[10], C, E, tr);
      } else {
        r = P.undef;
        bad += 1;
      }
      P.out[(long)l * P.level_stride + i] = r;
    }
    block_count_add(P.n_undefined + l, bad);
  }
}

} // namespace

hipError_t launch_vessel_icing(const IcingParams& P, hipStream_t stream)
{
  if (P.n <= 0 || P.nlev <= 0)
    return hipSuccess;
  const int threads = 256;
  const long want = ((long)P.n + threads - 1) / threads;
  const int gx = (int)(want < 65535 ? want : 65535);
  const int gy = P.nlev < 65535 ? P.nlev : 65535;
  if (P.model == mifc_icing::MODSTALL)
    hipLaunchKernelGGL(vessel_icing_kernel<mifc_icing::MODSTALL>, dim3(gx, gy), dim3(threads), 0, stream, P);
  else
    hipLaunchKernelGGL(vessel_icing_kernel<mifc_icing::MINCOG>, dim3(gx, gy), dim3(threads), 0, stream, P);
  return hipGetLastError();
}

} // namespace mifc
