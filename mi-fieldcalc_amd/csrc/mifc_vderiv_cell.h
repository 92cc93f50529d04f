// mifc_vderiv_cell.h -- rules 1 to 5 of mifc_vderiv_* (include/mifc.h) for the V cells of a lane, stated once for the
// kernels that difference a level batch along the coordinate (mifc_vderiv.hip, mifc_pvort.hip): what the coordinate of a
// cell allows at a level, which sides of a (field, cell) take part, the weights and the derivative in double before its
// rounding.  The walk that brings the levels k - 1, k and k + 1 together stays in each kernel: written once here, as a
// template over the kernels' load and level steps, it cost pvort_kernel<VDERIV_HYBRID, 4> two SGPR spills
// (profiles/README.md).  KIND is VDERIV_HYBRID / _FIELD / _LEVELS
// (mifc_kernels.h); with VDERIV_LEVELS the coordinate is the same in every cell of a level, the host has divided
// (vderiv_level_weights, mifc_levelbatch.h) and the weights come in through scalar loads.  Device code only.
#ifndef MIFC_VDERIV_CELL_H
#define MIFC_VDERIV_CELL_H

#include "mifc_column_walk.h"
#include "mifc_device.h"

namespace mifc {

namespace {

// what a (field, cell) of a level is, two bits: the sides that take part; 0 = the result is undef
const unsigned int SIDE_LOWER = 1u, SIDE_UPPER = 2u, SIDE_BOTH = 3u;
// what the coordinate of a cell allows at a level (SIDE_* in the low bits)
const unsigned int CELL_LOWER = 1u, CELL_UPPER = 2u, CELL_CENTRE = 4u, CELL_FOLD = 8u;

// rule 2 for the values of a level as it arrives: bit f of the cell's word = x_f passes is_defined, or bit f of `all` (the
// level's word of the table, shifted to the launch's field 0) says ALL_DEFINED.  Every value is tested once; as lane masks
// the tests of the three levels in flight would not fit into the SGPRs
template <int NF, int V>
__device__ __forceinline__ void vderiv_defined(unsigned int (&df)[V], const WalkLevel<NF, V>& L, unsigned int all, float undef)
{
#pragma unroll
  for (int c = 0; c < V; ++c) {
    unsigned int w = 0;
#pragma unroll
    for (int f = 0; f < NF; ++f)
      w |= (((all >> f) & 1u) != 0 || is_def(L.x[f][c], undef)) ? 1u << f : 0u;
    df[c] = walk_here_v(w);
  }
}

// rules 1 and 3 for the coordinate: is c_k usable, does c_k-1 / c_k+1 exist, is it usable and different -- per cell in a
// VGPR (as lane masks these sixteen tests would take more SGPRs than a wave has to spare): CELL_LOWER / CELL_UPPER = the
// side's coordinate is usable and differs, CELL_CENTRE = c_k is usable, CELL_FOLD = zero denominator.  h1, h2: the two
// steps, den: the two-sided denominator of the method.  VDERIV_LEVELS: all of it from the level's word.
template <int KIND, int V>
__device__ __forceinline__ void vderiv_cell_mask(unsigned int (&cm)[V], double (&h1)[V], double (&h2)[V], double (&den)[V], const float (&cp)[V],
                                                 const float (&cc)[V], const float (&cn)[V], unsigned int bits_k, bool weighted)
{
#pragma unroll
  for (int c = 0; c < V; ++c) {
    if constexpr (KIND == VDERIV_LEVELS) {
      cm[c] = ((bits_k >> VDERIV_LOWER_BIT) & 1u) * CELL_LOWER | ((bits_k >> VDERIV_UPPER_BIT) & 1u) * CELL_UPPER | CELL_CENTRE |
              ((bits_k >> VDERIV_FOLD_BIT) & 1u) * CELL_FOLD;
      h1[c] = h2[c] = den[c] = 0.0;
    } else {
      const double dm = (double)cp[c], d0 = (double)cc[c], dp = (double)cn[c];
      h1[c] = d0 - dm;
      h2[c] = dp - d0;
      const double s = h1[c] + h2[c], dc = dp - dm;
      den[c] = weighted ? s : dc;
      cm[c] = ((cp[c] == cp[c] && cp[c] != cc[c]) ? CELL_LOWER : 0u) | // (no level k - 1: cp is NaN)
              ((cn[c] == cn[c] && cn[c] != cc[c]) ? CELL_UPPER : 0u) | (cc[c] == cc[c] ? CELL_CENTRE : 0u) | (den[c] == 0.0 ? CELL_FOLD : 0u);
      cm[c] = walk_here_v(cm[c]);
    }
  }
}

// The sides of every field of cell c: SIDE_* of field f in the bits 2f, 2f + 1 of cls; `every` = the AND of the lane's
// classes so far (start with SIDE_BOTH), `any` = which classes the lane has (bit s - 1 for SIDE_* s; start with 0).
// inside = false: a cell that is not stored as itself decides nothing, it counts as SIDE_BOTH.
template <int NF>
__device__ __forceinline__ unsigned int vderiv_classify(unsigned int& every, unsigned int& any, unsigned int cm, unsigned int dfp, unsigned int dfk,
                                                        unsigned int dfn, bool inside = true)
{
  unsigned int cls = 0;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const unsigned int okbits = ((dfp >> f) & 1u) * CELL_LOWER | ((dfn >> f) & 1u) * CELL_UPPER | ((dfk >> f) & 1u) * CELL_CENTRE | CELL_FOLD;
    const unsigned int t = cm & okbits;
    unsigned int s = t & SIDE_BOTH; // rule 3 (CELL_LOWER, CELL_UPPER are SIDE_LOWER, SIDE_UPPER)
    s = ((t & CELL_CENTRE) != 0 && t != (SIDE_BOTH | CELL_CENTRE | CELL_FOLD)) ? s : 0u; // rule 2; rule 4's zero denominator
    s = inside ? s : SIDE_BOTH;
    cls |= s << (2 * f);
    any |= (1u << s) >> 1;
    every &= s;
  }
  return cls;
}

// the two-sided weights of rule 4 for one cell (CENTRED: wa = w; WEIGHTED: wa = w1, wb = w2)
template <int KIND>
__device__ __forceinline__ void vderiv_both_weights(double& wa, double& wb, double h1, double h2, double den, bool weighted, ConstDoubles lev_w, int k)
{
  if constexpr (KIND == VDERIV_LEVELS) {
    wa = lev_w[4 * k + 2];
    wb = lev_w[4 * k + 3];
  } else if (weighted) {
    const double p1 = h1 * den, p2 = h2 * den;
    wa = h2 / p1;
    wb = h1 / p2;
  } else {
    wa = 1.0 / den;
    wb = 0.0;
  }
}
// the one-sided weight of rule 5 for one cell: UPPER = false from h = h1, true from h = h2
template <int KIND, bool UPPER>
__device__ __forceinline__ double vderiv_one_weight(double h, ConstDoubles lev_w, int k)
{
  if constexpr (KIND == VDERIV_LEVELS)
    return lev_w[4 * k + (UPPER ? 1 : 0)];
  else
    return 1.0 / h;
}

// The derivative of one (field, cell) from the levels k - 1, k, k + 1 in double, every operation rounded on its own.
// Both sides take part (the fast bodies: no select by side):
__device__ __forceinline__ double vderiv_both(float lo, float cur, float hi, double wa, double wb, bool weighted)
{
  const double xm = (double)lo, x0 = (double)cur, xp = (double)hi;
  const double d1 = x0 - xm, d2 = xp - x0, d = xp - xm;
  const double t1 = d1 * wa, t2 = d2 * wb;
  const double sum = t1 + t2, centred = d * wa;
  return weighted ? sum : centred;
}
// the sides s = SIDE_* take part (s = 0: not meaningful, the caller writes undef); wl, wh: the one-sided weights of rule 5
__device__ __forceinline__ double vderiv_sided(unsigned int s, float lo, float cur, float hi, double wl, double wh, double wa, double wb, bool weighted)
{
  const double xm = (double)lo, x0 = (double)cur, xp = (double)hi;
  const double d1 = x0 - xm, d2 = xp - x0, d = xp - xm;
  const double one_lower = d1 * wl, one_upper = d2 * wh; // rule 5
  const double t1 = d1 * wa, t2 = d2 * wb;
  const double sum = t1 + t2, centred = d * wa;
  const double both = weighted ? sum : centred;
  return s == SIDE_BOTH ? both : (s == SIDE_LOWER ? one_lower : one_upper);
}

} // namespace

} // namespace mifc

#endif // MIFC_VDERIV_CELL_H
