// mifc_vregrid_rules.h -- the rules of mifc_vregrid_* (include/mifc.h, "interpolation of level batches to per-cell target
// surfaces"), stated once for the kernel of mifc_vregrid.hip and the tests: when a target is usable, when a pair of levels
// brackets it, the weight and the result of a bracket, the extremes a column keeps for OUTSIDE_CLAMP and the level a
// target outside them is clamped to.  Plain C++ without any device header: tests/test_vregrid_cpu.py compiles it with the
// host compiler (tests/vregrid_rules_shim.cc, tests/host/vregrid_rules_main.cc under the address and undefined-behaviour
// sanitizers).  The kernel file defines MIFC_VREGRID_FN as the host-and-device qualifiers before it includes this text.
//
// "Not usable" is carried as NaN everywhere: a coordinate that is undefined under its flag, a target that rule 2 turns
// away.  A NaN fails every ordered compare, so it never brackets, never becomes an extreme and is never outside them --
// no flag per cell has to live through the walk.
#ifndef MIFC_VREGRID_RULES_H
#define MIFC_VREGRID_RULES_H

#ifndef MIFC_VREGRID_FN
#include <cmath>
#define MIFC_VREGRID_FN inline
#endif

namespace mifc {

const int VREGRID_FROM_FIRST = 0, VREGRID_FROM_LAST = 1;       // MIFC_VREGRID_FROM_*
const int VREGRID_OUTSIDE_UNDEF = 0, VREGRID_OUTSIDE_CLAMP = 1; // MIFC_VREGRID_OUTSIDE_*

MIFC_VREGRID_FN float vregrid_nan()
{
  const unsigned int b = 0x7fc00000u;
  float x;
  __builtin_memcpy(&x, &b, sizeof x);
  return x;
}

// rule 2: the target as the walk carries it -- ct itself, or NaN where it is undefined under its flag, NaN, or (LOG) <= 0
MIFC_VREGRID_FN float vregrid_target(float ct, bool all_defined, float undef, bool by_log)
{
  const bool defined = all_defined || ct != undef; // (a NaN target stays a NaN either way)
  const bool usable = defined && (!by_log || ct > 0.f);
  return usable ? ct : vregrid_nan();
}

// rule 3: the pair brackets the target (both ends usable: a NaN end fails the compare of the pair)
MIFC_VREGRID_FN bool vregrid_brackets(float c_a, float c_b, float ct)
{
  const bool pair = c_a == c_a && c_b == c_b;
  const float lo = c_a < c_b ? c_a : c_b, hi = c_a < c_b ? c_b : c_a;
  return pair && lo <= ct && ct <= hi;
}

// rule 4 (rule 6 of mifc_vinterp_*): the weight of the pair oriented (k, k + 1), in double, every operation on its own
template <bool LOG>
MIFC_VREGRID_FN double vregrid_weight(float c_k, float c_k1, float ct)
{
  if (LOG) {
    const double lk = log((double)c_k), lk1 = log((double)c_k1), lt = log((double)ct);
    const double num = lt - lk, den = lk1 - lk;
    return num / den;
  }
  const double num = (double)ct - (double)c_k, den = (double)c_k1 - (double)c_k;
  return num / den;
}

// ... and the result where c_k != c_k+1 (the caller selects x_k where they are equal)
MIFC_VREGRID_FN float vregrid_value(double w, float x_k, float x_k1)
{
  const double dk = (double)x_k;
  const double diff = (double)x_k1 - dk;
  const double prod = w * diff;
  return (float)(dk + prod);
}

// rule 5: kmin / kmax, the LOWEST index that attains the smallest / largest usable coordinate of the column.  The levels
// come in walk order: ascending (FROM_FIRST) a later level wins only where it is strictly beyond, descending (FROM_LAST)
// also where it ties.  kmin < 0: no usable level yet.
struct VregridExtremes
{
  float cmin, cmax;
  int kmin, kmax;
};
MIFC_VREGRID_FN void vregrid_extremes_start(VregridExtremes& e)
{
  e.cmin = e.cmax = 0.f;
  e.kmin = e.kmax = -1;
}
MIFC_VREGRID_FN void vregrid_extremes_level(VregridExtremes& e, float c, int k, bool descending)
{
  const bool usable = c == c, first = usable && e.kmin < 0;
  const bool below = first || (descending ? c <= e.cmin : c < e.cmin), above = first || (descending ? c >= e.cmax : c > e.cmax);
  e.cmin = below ? c : e.cmin;
  e.kmin = below ? k : e.kmin;
  e.cmax = above ? c : e.cmax;
  e.kmax = above ? k : e.kmax;
}
// the level whose value a target without a bracket takes under OUTSIDE_CLAMP, -1: undef (inside the range, where holes
// left no bracket; no usable level; a target that is not usable)
MIFC_VREGRID_FN int vregrid_clamp_level(const VregridExtremes& e, float ct)
{
  const bool any = e.kmin >= 0;
  return (any && ct < e.cmin) ? e.kmin : ((any && ct > e.cmax) ? e.kmax : -1);
}

} // namespace mifc

#endif // MIFC_VREGRID_RULES_H
