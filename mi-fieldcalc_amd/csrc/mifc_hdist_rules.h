// mifc_hdist_rules.h -- the rules of mifc_hdist_histogram_levels and mifc_hdist_quantile_levels (include/mifc.h), stated
// once for the kernels of mifc_hdist.hip, the host code of mifc_capi_hdist.hip and the tests: the ordered key of a value
// and the key that bins it, the edge check, the bin search, the two rank rules, the digit plan of the selection and its
// scan step.  Plain C++ without any device header: tests/test_hdist_cpu.py compiles it with the host compiler
// (tests/hdist_rules_shim.cc, tests/host/hdist_rules_main.cc under the address and undefined-behaviour sanitizers).  The
// kernel file defines MIFC_HDIST_FN as the host-and-device qualifiers before it includes this text.
//
// Keys.  order_key maps the bits of a float to an unsigned word whose < is the IEEE total order of rule 3 of
// mifc_ensembleQuantiles: -inf < ... < -0 < +0 < ... < +inf, and every NaN, whatever its sign and payload, on the one key
// 0xffffffff above +inf (0xff800000).  bin_key is the same map with -0 folded onto +0 first: for two values that are no
// NaN, bin_key(a) <= bin_key(b) is exactly the IEEE a <= b, which is what a histogram edge compares.
//
// Selection.  The key of rank r of a (field, level) is found digit by digit from the top: pass 0 of the kernels gives the
// smallest and the largest key, the digits start below their common prefix (hdist_digit_plan), a pass counts for every
// prefix still wanted the digit that follows it, and hdist_scan_step turns a rank inside a prefix into the digit that holds
// it and the rank inside that digit.  Digits are HDIST_DIGIT_BITS = 11 bits wide: 32 bits below an empty prefix take three
// passes, the 22 bits and less of a level whose values share sign, exponent and a mantissa bit take two.
#ifndef MIFC_HDIST_RULES_H
#define MIFC_HDIST_RULES_H

#ifndef MIFC_HDIST_FN
#define MIFC_HDIST_FN inline
#endif

namespace mifc {

typedef unsigned int hdist_u32;

const int HDIST_MAX_FIELDS = 8, HDIST_MAX_EDGES = 1024, HDIST_MAX_Q = 16, HDIST_MAX_RANKS = 32;
const int HDIST_DIGIT_BITS = 11, HDIST_DIGIT_BINS = 1 << HDIST_DIGIT_BITS, HDIST_MAX_PASSES = 3;
const int HDIST_LOWER = 0, HDIST_LINEAR = 1; // MIFC_QUANTILE_LOWER, MIFC_QUANTILE_LINEAR
const hdist_u32 HDIST_NAN_KEY = 0xffffffffu, HDIST_NAN_BITS = 0x7fc00000u;

MIFC_HDIST_FN hdist_u32 hdist_float_bits(float x)
{
  hdist_u32 b;
  __builtin_memcpy(&b, &x, sizeof b);
  return b;
}
MIFC_HDIST_FN float hdist_bits_float(hdist_u32 b)
{
  float x;
  __builtin_memcpy(&x, &b, sizeof x);
  return x;
}
MIFC_HDIST_FN bool hdist_is_nan_bits(hdist_u32 b)
{
  return (b & 0x7fffffffu) > 0x7f800000u;
}

// the total order as unsigned words; every NaN is HDIST_NAN_KEY
MIFC_HDIST_FN hdist_u32 hdist_order_key(hdist_u32 b)
{
  if (hdist_is_nan_bits(b))
    return HDIST_NAN_KEY;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
// the bits of the value of a key; HDIST_NAN_KEY gives the quiet NaN without a payload
MIFC_HDIST_FN hdist_u32 hdist_key_bits(hdist_u32 k)
{
  if (k == HDIST_NAN_KEY)
    return HDIST_NAN_BITS;
  return (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
}
// the key that bins: -0 is +0 (not for a NaN: it has a slot of its own)
MIFC_HDIST_FN hdist_u32 hdist_bin_key(hdist_u32 b)
{
  return hdist_order_key(b == 0x80000000u ? 0u : b);
}

// The edges of one field: -1 where they are no NaN and strictly ascending under <, else the index of the first edge that
// is a NaN or not above the one before it.
MIFC_HDIST_FN int hdist_check_edges(const float* edges, int nedges)
{
  for (int e = 0; e < nedges; ++e) {
    if (edges[e] != edges[e])
      return e;
    if (e > 0 && !(edges[e - 1] < edges[e]))
      return e;
  }
  return -1;
}

// b = #{e : edge_keys[e] <= key} for ascending bin keys: numpy.searchsorted(edges, x, side="right")
MIFC_HDIST_FN int hdist_bin(const hdist_u32* edge_keys, int nedges, hdist_u32 key)
{
  int lo = 0, hi = nedges; // edge_keys[< lo] <= key < edge_keys[>= hi]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (edge_keys[mid] <= key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}
// the slot of a value: its bin, or nedges + 1 for a NaN
MIFC_HDIST_FN int hdist_slot(const hdist_u32* edge_keys, int nedges, hdist_u32 value_bits)
{
  return hdist_is_nan_bits(value_bits) ? nedges + 1 : hdist_bin(edge_keys, nedges, hdist_bin_key(value_bits));
}

// Rule 4 of mifc_ensembleQuantiles for n >= 1 sorted values and a percentile p in [0, 100]: the result is x[k] where
// t == 0, else (float)(x[k] + t * (x[k1] - x[k])) in double; k1 = k where t == 0, else k + 1.
struct HdistRank
{
  int k, k1;
  double t;
};
MIFC_HDIST_FN HdistRank hdist_rank(int method, int n, float p)
{
  HdistRank r;
  if (method == HDIST_LOWER) {
    const float v = ((float)n * p) / 100.0f; // all in float, truncated
    int ii = v >= 2147483648.0f ? n - 1 : (int)v;
    if (ii > n - 1)
      ii = n - 1;
    r.k = r.k1 = ii;
    r.t = 0.0;
  } else {
    const double h = ((double)(n - 1) * (double)p) / 100.0;
    r.k = (int)h;
    r.t = h - (double)r.k;
    r.k1 = r.t == 0.0 ? r.k : r.k + 1;
  }
  return r;
}
// the value of a percentile from the bits of x[k] and x[k1]
MIFC_HDIST_FN float hdist_interpolate(hdist_u32 xk_bits, hdist_u32 xk1_bits, double t)
{
  if (t == 0.0)
    return hdist_bits_float(xk_bits);
  const double a = (double)hdist_bits_float(xk_bits), b = (double)hdist_bits_float(xk1_bits);
  const double d = b - a;
  const double s = t * d;
  return (float)(a + s);
}

// The digits of the selection between the smallest and the largest key of a (field, level): the keys share their top
// prefix_bits bits; pass j counts the `width[j]` bits from bit `shift[j]` up, from the top down, HDIST_DIGIT_BITS at a
// time, the last pass what is left.  Equal keys: no pass at all.
struct HdistPlan
{
  int prefix_bits, passes;
  int shift[HDIST_MAX_PASSES], width[HDIST_MAX_PASSES];
};
MIFC_HDIST_FN HdistPlan hdist_digit_plan(hdist_u32 kmin, hdist_u32 kmax)
{
  HdistPlan p;
  const hdist_u32 diff = kmin ^ kmax;
  p.prefix_bits = diff == 0u ? 32 : __builtin_clz(diff);
  int left = 32 - p.prefix_bits;
  p.passes = (left + HDIST_DIGIT_BITS - 1) / HDIST_DIGIT_BITS;
  for (int j = 0; j < HDIST_MAX_PASSES; ++j) {
    const int w = j < p.passes ? (left < HDIST_DIGIT_BITS ? left : HDIST_DIGIT_BITS) : 0;
    left -= w;
    p.width[j] = w;
    p.shift[j] = left;
  }
  return p;
}
// what is above the digit of a pass: key >> (shift + width), 0 where that is the whole word
MIFC_HDIST_FN hdist_u32 hdist_prefix_of(hdist_u32 key, int shift, int width)
{
  const int s = shift + width;
  return s >= 32 ? 0u : key >> s;
}
MIFC_HDIST_FN hdist_u32 hdist_digit_of(hdist_u32 key, int shift, int width)
{
  return (key >> shift) & ((1u << width) - 1u);
}

// One step of the selection: `rank` (0-based) among the values counted in hist[0 .. nbins), whose sum is above it; the
// digit d that holds it -- the smallest d with hist[0] + ... + hist[d] > rank -- and the rank inside that digit.
struct HdistStep
{
  int digit;
  hdist_u32 rank;
};
MIFC_HDIST_FN HdistStep hdist_scan_step(const hdist_u32* hist, int nbins, hdist_u32 rank)
{
  HdistStep s;
  s.digit = nbins - 1; // (a rank that is not below the sum: the last digit; the callers never ask)
  s.rank = rank;
  bool found = false;
  for (int d = 0; d < nbins; ++d) { // (straight-line: every digit is read, nothing after the one that holds the rank counts)
    const hdist_u32 c = hist[d];
    const bool here = !found && s.rank < c;
    s.digit = here ? d : s.digit;
    found = found || here;
    s.rank -= found ? 0u : c;
  }
  return s;
}

} // namespace mifc

#endif // MIFC_HDIST_RULES_H
