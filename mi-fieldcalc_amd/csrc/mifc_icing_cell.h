// mifc_icing_cell.h -- the two iterative freezing-spray models of FieldCalculationsVesselIcing.cc, one cell at a time:
// vesselIcingModStall (:182-337) and vesselIcingMincog (:466-705), restated from their equations with the reference's
// precision operation by operation (DESIGN.md 4.12 has the map).  hipcc compiles it for the kernels of mifc_icing.hip;
// g++ compiles it for the host restatement that the CPU tests compare with the compiled reference bit for bit.
//
// Precision: ModStall computes in double, except that its inputs are float, |(u, v)| and sal * sal are float
// products and icing_f1(airtemp) is the float function (expf).  MINCOG is the reference's template instantiated with
// float: float variables, but every expression with a double literal or a double libm call (exp, pow, tanh, cos, sin)
// is evaluated in double and rounded to float where it is stored.  No multiply-add is fused (-ffp-contract=off here,
// no FMA in the reference build).
//
// libm: the f_* overloads below call glibc on the host.  On the device a float function is the double function rounded
// once (never ocml's native float functions or __expf-class intrinsics), except sinhf, which restates glibc's own float
// algorithm (sinhf_fdlibm); a double function is ocml's double.
#ifndef MIFC_ICING_CELL_H
#define MIFC_ICING_CELL_H

#include <cmath>

#ifdef __HIPCC__
#define MIFC_HD __host__ __device__
#else
#define MIFC_HD
#endif

namespace mifc_icing {

enum { MODSTALL = 1, MINCOG = 2 };

// ---- glibc's sinhf, restated in float: the classic fdlibm algorithm (sinh through expm1f below 22, expf above) that
// glibc 2.35 ships.  It is not the double sinh rounded once -- 21 % of all floats differ by an ulp -- and MINCOG "adj"
// feeds it into every level, so the device uses this restatement.  It equals glibc's sinhf on every float below 22 in
// magnitude; above, its expf is the double exp rounded once, which glibc's expf differs from on 0.06 % of the
// arguments (tests/test_vessel_icing_cpu.py).
MIFC_HD inline unsigned fl_bits(float x)
{
  return __builtin_bit_cast(unsigned, x);
}
MIFC_HD inline float bits_fl(unsigned u)
{
  return __builtin_bit_cast(float, u);
}
MIFC_HD inline float expm1f_fdlibm(float x) // finite |x| < 22 only (what sinhf_fdlibm hands it)
{
  const float ln2_hi = bits_fl(0x3f317180u), ln2_lo = bits_fl(0x3717f7d1u), invln2 = bits_fl(0x3fb8aa3bu);
  const float Q1 = bits_fl(0xbd088889u), Q2 = bits_fl(0x3ad00d01u), Q3 = bits_fl(0xb8a670cdu), Q4 = bits_fl(0x36867e54u),
              Q5 = bits_fl(0xb457edbbu);
  unsigned hx = fl_bits(x);
  const bool neg = (hx >> 31) != 0;
  hx &= 0x7fffffffu;
  float hi, lo, c = 0.0f;
  int k;
  if (hx > 0x3eb17218u) { // |x| > ln2 / 2: reduce by k ln2
    if (hx < 0x3f851592u) {
      hi = neg ? x + ln2_hi : x - ln2_hi;
      lo = neg ? -ln2_lo : ln2_lo;
      k = neg ? -1 : 1;
    } else {
      k = (int)(invln2 * x + (neg ? -0.5f : 0.5f));
      const float t = (float)k;
      hi = x - t * ln2_hi;
      lo = t * ln2_lo;
    }
    x = hi - lo;
    c = (hi - x) - lo;
  } else if (hx < 0x33000000u) {
    return x;
  } else {
    k = 0;
  }
  const float hfx = 0.5f * x, hxs = x * hfx;
  const float r1 = 1.0f + hxs * (Q1 + hxs * (Q2 + hxs * (Q3 + hxs * (Q4 + hxs * Q5))));
  float t = 3.0f - r1 * hfx;
  float e = hxs * ((r1 - t) / (6.0f - x * t));
  if (k == 0)
    return x - (x * e - hxs);
  e = (x * (e - c) - c);
  e -= hxs;
  if (k == -1)
    return 0.5f * (x - e) - 0.5f;
  if (k == 1)
    return x < -0.25f ? -2.0f * (e - (x + 0.5f)) : 1.0f + 2.0f * (x - e);
  float y;
  if (k <= -2 || k > 56) {
    y = 1.0f - (e - x);
    return bits_fl(fl_bits(y) + ((unsigned)k << 23)) - 1.0f;
  }
  if (k < 23) {
    t = bits_fl(0x3f800000u - (0x1000000u >> k));
    y = t - (e - x);
  } else {
    t = bits_fl((unsigned)(0x7f - k) << 23);
    y = x - (e + t);
    y += 1.0f;
  }
  return bits_fl(fl_bits(y) + ((unsigned)k << 23));
}

// ---- libm selection
#ifdef __HIP_DEVICE_COMPILE__
MIFC_HD inline float f_exp(float x) { return (float)::exp((double)x); }
MIFC_HD inline float f_sqrt(float x) { return (float)::sqrt((double)x); } // exact: double rounding is harmless for sqrt
MIFC_HD inline float f_sin(float x) { return (float)::sin((double)x); }
MIFC_HD inline float f_cos(float x) { return (float)::cos((double)x); }
MIFC_HD inline float f_asin(float x) { return (float)::asin((double)x); }
MIFC_HD inline float f_sinh(float x); // glibc's algorithm, below
#else
inline float f_exp(float x) { return std::exp(x); }
inline float f_sqrt(float x) { return std::sqrt(x); }
inline float f_sin(float x) { return std::sin(x); }
inline float f_cos(float x) { return std::cos(x); }
inline float f_asin(float x) { return std::asin(x); }
inline float f_sinh(float x) { return std::sinh(x); }
#endif
MIFC_HD inline double d_exp(double x) { return ::exp(x); }
MIFC_HD inline double d_tanh(double x) { return ::tanh(x); }
MIFC_HD inline double d_pow(double x, double y) { return ::pow(x, y); }

const double PI = 3.14159265358979323846; // M_PI

MIFC_HD inline float sinhf_fdlibm(float x)
{
  const unsigned jx = fl_bits(x), ix = jx & 0x7fffffffu;
  if (ix >= 0x7f800000u)
    return x + x;
  const float h = (jx >> 31) ? -0.5f : 0.5f;
  const float ax = bits_fl(ix);
  if (ix < 0x41b00000u) { // |x| < 22
    if (ix < 0x31800000u)
      return x;
    const float t = expm1f_fdlibm(ax);
    if (ix < 0x3f800000u)
      return h * (2.0f * t - t * t / (t + 1.0f));
    return h * (t + t / (t + 1.0f));
  }
  if (ix < 0x42b17180u)
    return h * f_exp(ax);
  if (ix <= 0x42b2d4fcu) {
    const float w = f_exp(0.5f * ax);
    const float t = h * w;
    return t * w;
  }
  return x * 1.0e37f; // overflow
}
#ifdef __HIP_DEVICE_COMPILE__
MIFC_HD inline float f_sinh(float x)
{
  return sinhf_fdlibm(x);
}
#endif

// icing_f1 (:54-57) in float and in double
MIFC_HD inline float f1_float(float t)
{
  return 0.6112f * f_exp(17.67f * t / (t + 243.5f));
}
MIFC_HD inline double f1_double(double t)
{
  return 0.6112 * d_exp(17.67 * t / (t + 243.5));
}
// kT4 (:66-70) in float; t0 = 273.15f (MetConstants.h:39)
MIFC_HD inline float kT4_float(float t)
{
  const float x = t + 273.15f;
  const float x2 = x * x;
  return 5.67e-8f * (x2 * x2);
}

// Per-call constants, computed once on the host with the reference's precision (icing_consts below).
struct IcingConsts
{
  int model, alt;
  int number;      // levels: (zmax - zmin) * 2 + 1, in double (ModStall) or float (MINCOG)
  int bisect_iter; // MINCOG's bisection trip count: (int)log2f((1.3f - -0.5f) / 1e-5f) = 17
  float vs;
  double vs_cos_d; // ModStall: vs * cos(alpha)
  double cos_d;    // MINCOG: cos(beta), beta = alpha (Wrx, in double)
  float cos_alpha; // MINCOG: (float)cos(alpha)
  float sin_beta;  // MINCOG: (float)sin(alpha)
  float drag;      // MINCOG: -0.0046 * beta_deg + 2.1912
  float Swdown;    // MINCOG: 0 * view factor
  // MINCOG's beta_r branches with a constant angle: [0] beta_r <= pi / 2 (91 degrees), [1] beta_r > pi (pi):
  // sin(br)^2, cos(br), cos(2 br)
  float br_sin2[2], br_cos[2], br_cos2[2];
};

// Which cells are computed (:208-209, :696).  all: the caller's flag was ALL_DEFINED (no is_defined test).  Pw is not
// tested.  aice < 0.4 and MINCOG's freezing-point test compare in double; the latter's 1000 - sal is a float.
MIFC_HD inline bool is_def(float x, float undef)
{
  return !(x != x) && x != undef;
}
MIFC_HD inline bool icing_defined(int model, bool all, float sal, float wave, float xw, float yw, float airtemp, float rh, float sst, float p,
                                  float aice, float depth, float undef)
{
  const bool d = all || (is_def(sal, undef) && is_def(wave, undef) && is_def(xw, undef) && is_def(yw, undef) && is_def(airtemp, undef) &&
                         is_def(rh, undef) && is_def(sst, undef) && is_def(p, undef) && is_def(aice, undef) && is_def(depth, undef));
  if (!d || !((double)aice < 0.4))
    return false;
  if (model == MINCOG)
    return (double)sst > (-54.1126 * (double)sal / (double)(1000 - sal));
  return true;
}

// Loop trip counters: the kernels pass NoTrips; the host restatement may count (tools/bench_vessel_icing.py).
struct NoTrips
{
  MIFC_HD void disp(int) const {}
  MIFC_HD void level(int) const {}
};

// ---- vesselIcingModStall, one defined cell (:218-328).  E[k] = exp(-0.55 * (zmin + 0.5 * k)).
template <class Tab, class Trips>
MIFC_HD inline float modstall_cell(float sal, float wave, float xw, float yw, float airtemp, float rh, float sst, float p, float Pw, float depth,
                                   const IcingConsts& C, const Tab& E, Trips& tr)
{
  const double pw = Pw, dep = depth;
  double c = (9.81 / (2 * PI)) * pw;
  if (dep <= c * pw && c != 0) { // shallow water: fixed point on the phase speed, given up after 10 000 trips
    c = 1.0;
    double err = 1.0;
    int j = 0;
    const double cw = 9.81 * pw / (2 * PI), a = 2 * PI * dep;
    while (err > 1e-5) {
      const double c_new = cw * d_tanh(a / (pw * c));
      err = ::fabs(c_new - c);
      c = c_new;
      j = j + 1;
      if (j > 10000) {
        c = 0.0;
        break;
      }
    }
    tr.disp(j);
  }
  const double Vr = c - C.vs_cos_d;
  const double v = f_sqrt(xw * xw + yw * yw);
  const double Tf = (-0.002 - 0.0524 * (double)sal) - 6.0E-5 * (double)(sal * sal);
  const double ha = 5.17 * d_pow(v, 0.8);
  const double ratio = 89.5 / 5.17;
  const double tau = 11.25 - v / 4.0;
  double k1 = sst;
  if (tau > 0.0) { // droplet temperature: RK4, 50 steps
    const double K = 311000.0 / (((double)p / 10.0) * 1005.0);
    const double M = 0.2 * (double)airtemp + K * (double)rh * (double)f1_float(airtemp);
    const double h = tau / 50.0;
    double y = sst;
    for (int s = 0; s < 50; s++) {
      k1 = (M - 0.2 * y) - K * f1_double(y);
      double y2 = y + 0.5 * h * k1;
      const double k2 = (M - 0.2 * y2) - K * f1_double(y2);
      const double y3 = y + 0.5 * h * k2;
      y2 = (M - 0.2 * y3) - K * f1_double(y3);
      const double y4 = y + h * y2;
      y += h * ((1.0 / 6.0) * (((k1 + 2.0 * k2) + 2.0 * y2) + ((M - 0.2 * y4) - K * f1_double(y4))));
      k1 = y;
    }
  }
  const double rh_ea = (double)(rh * f1_float(airtemp)); // float product in the reference
  const double rw0 = 6.46E-5 * (double)wave * (Vr * Vr);
  const double hl = ha / 333000.0;
  double ice = 0;
  for (int k = 0; k < C.number; k++) { // per spray level: fixed point on the freezing fraction N
    const double rw = rw0 * E[k] * v;
    double N = 0.0, err = 1.0;
    int j = 0;
    while (err >= 1.0E-5 && N >= 0 && N <= 1) {
      const double Ts = (1.0 + N) * Tf;
      const double ri = (0.012012012 * rw * (Ts - k1) + hl * ((Ts - (double)airtemp) + ratio * (f1_double(Ts) - rh_ea)));
      const double N1 = ri / rw;
      err = ::fabs(N1 - N);
      N = N1;
      j = j + 1;
      if (j > 1000) {
        N = 0.0;
        break;
      }
    }
    tr.level(j);
    if (N < 0.0)
      N = 0.0;
    else if (N > 1.0)
      N = 1.0;
    ice += N * (rw / 890.0) * 3600.0 * 100.0;
  }
  return (float)::fabs(ice / C.number);
}

// ---- MINCOG: FreezeFracZero<float> (:345-361); Swdown is 0 * view factor
struct FreezeFrac
{
  float Sw, Ta, ha, he, ea, RH, rw, Tsp, Lwdown, Swdown;
  MIFC_HD float operator()(float N) const
  {
    const float cw = 4000;
    const float lfs = (float)(3.33e5 * 0.7);
    const float Sb = (float)((double)Sw / (1 - (double)N * (1 - 0.3)));
    const float Ts = -54.1126f * (Sb / (1000 - Sb));
    const float es = 10 * f1_float(Ts);
    const float Qc = ha * (Ts - Ta);
    const float Qe = he * (es - RH * ea);
    const float Qd = rw * cw * (Ts - Tsp);
    const float Lwup = kT4_float(Ts);
    const float Qr = (float)((double)(Lwup - Lwdown) - 0.44 * (double)Swdown);
    const float ri = (1 / lfs) * (Qc + Qe + Qd + Qr);
    return ri / rw - N;
  }
};

// the reference's bisection (:381-415) on [-0.5, 1.3], tolerance 1e-5; `iterations` = C.bisect_iter
MIFC_HD inline float mincog_bisection(const FreezeFrac& f, int iterations)
{
  float a = -0.5f, b = 1.3f;
  float ffa = f(a);
  const float ffb = f(b);
  if ((ffa > 0) == (ffb > 0))
    return 0;
  float c = 0;
  int j = 0;
  for (; j < iterations; ++j) {
    c = (a + b) / 2;
    const float ffc = f(c);
    if (ffc == 0)
      return c;
    if ((ffc > 0) != (ffa > 0)) {
      b = c;
    } else {
      a = c;
      ffa = ffc;
    }
  }
  if (j >= 100)
    c = 0;
  return c;
}

// ---- vesselIcingMincog<float>, one defined cell (:466-675)
template <class Tab, class Trips>
MIFC_HD inline float mincog_cell(float sal, float wave, float xw, float yw, float airtemp, float rh, float sst, float p, float Pw, float depth,
                                 const IcingConsts& C, const Tab& E, Trips& tr)
{
  const float v = f_sqrt(xw * xw + yw * yw);
  if (v < 1 || (double)wave < 0.1)
    return 0;
  const float c_0 = (float)(9.81 / (2 * PI) * (double)Pw);
  float c = c_0;
  if (depth <= c * Pw && c_0 != 0) { // shallow water: at most 1000 trips
    c = 1;
    int j = 0;
    const float a = (float)(2 * PI * (double)depth / (double)Pw);
    for (; j < 1000; ++j) {
      const float c_new = (float)((double)c_0 * d_tanh((double)(a / c)));
      const float err = ::fabsf(c_new - c);
      c = c_new;
      if ((double)err <= 1e-5)
        break;
    }
    tr.disp(j < 1000 ? j + 1 : j);
    if (j >= 1000)
      c = 0;
  }
  const float Vr = c - C.vs * C.cos_alpha;
  const float tper = ::fabsf(c * Pw / Vr);
  if (tper <= 0)
    return 0;
  const float Wrx = (float)::fabs((double)v * C.cos_d - (double)C.vs);
  const float Wry = ::fabsf(v * C.sin_beta);
  const float Wr_inv = 1 / f_sqrt(Wrx * Wrx + Wry * Wry);
  const float hax = (float)(6.0617 * d_pow((double)Wrx, 1.82));
  const float hay = (float)(4.8496 * d_pow((double)Wry, 1.8));
  const float ha = (hax + hay) / (Wrx + Wry);
  const float vmax = (v < 5.f) ? 5.f : v;
  const float tdur = (float)(0.1230 + 0.7008 * (double)::fabsf(Vr * wave) / (double)vmax);
  const float Nf = 1 / (4 * tper);
  const float beta_r = (float)(PI - (double)f_asin(v * C.sin_beta * Wr_inv));
  float sb2, cb, c2b;
  if ((double)beta_r <= PI / 2) {
    sb2 = C.br_sin2[0];
    cb = C.br_cos[0];
    c2b = C.br_cos2[0];
  } else if ((double)beta_r > PI) {
    sb2 = C.br_sin2[1];
    cb = C.br_cos[1];
    c2b = C.br_cos2[1];
  } else {
    const float s = f_sin(beta_r);
    sb2 = s * s;
    cb = f_cos(beta_r);
    c2b = f_cos(2 * beta_r);
  }
  const float r0 = 13.18f, a0 = 32.88f, b0 = 6.605f;
  const float a0_2 = a0 * a0, b0_2 = b0 * b0, r0_2 = r0 * r0;
  const float den = (b0_2 - a0_2) * c2b + a0_2 + b0_2;
  const float c0 = (float)(1.4142135623730951 * (double)a0 * (double)b0 * (double)f_sqrt(den - 2 * r0_2 * sb2)); // std::sqrt(2): double
  const float r = (r0 * 2 * b0_2 * cb + c0) / den;
  const float tau = (r * Wr_inv) * C.drag;
  const float ea = 10 * f1_float(airtemp);
  const float K = (float)(0.2 * 0.622 * 2.5E6 / ((double)p * 1005.0));
  const float M = (float)(0.2 * (double)airtemp + (double)(K * rh * ea));
  // runge_kutta (:450-463) over IcingF10MK<float>: (M - 0.2 t) - K * 10 * icing_f1(t)
  const float h = tau / 50, h2 = h / 2, K10 = K * 10;
  float y = sst;
  for (int s = 0; s < 50; s++) {
    const float k1 = h2 * ((M - 0.2f * y) - K10 * f1_float(y));
    const float ya = y + k1;
    const float k2 = h * ((M - 0.2f * ya) - K10 * f1_float(ya));
    const float yb = y + k2 / 2;
    const float k3 = h * ((M - 0.2f * yb) - K10 * f1_float(yb));
    const float yc = y + k3;
    const float k4 = h2 * ((M - 0.2f * yc) - K10 * f1_float(yc));
    y += (k1 + k2 + k3 + k4) / 3;
  }
  const float Tsp = (float)(0.5 * (double)(y + sst));
  const float Vdcomp = (float)((double)Wrx * 0.9962 + (double)6.67f * 0.0872);
  float lwc0;
  if (C.alt == 1) { // MINCOG org
    lwc0 = (float)(6.36E-5 * (double)wave * (double)(Vr * Vr));
  } else { // MINCOG adj
    const float lambda = c * Pw;
    const float dl = (float)(4 * PI * (double)depth / (double)lambda);
    const float cg = (c / 2) * (1 + dl / f_sinh(dl));
    const float Vgr = cg - C.vs * C.cos_alpha;
    lwc0 = (float)(9.5205E-4 * (double)(wave * wave) * (double)f_sqrt(wave / lambda) * (double)Vgr);
  }
  lwc0 = ::fabsf(lwc0);
  FreezeFrac ffz;
  ffz.Sw = sal;
  ffz.Ta = airtemp;
  ffz.ha = ha;
  ffz.he = (float)((double)ha * 1738.6 / (double)p);
  ffz.ea = ea;
  ffz.RH = rh;
  ffz.Tsp = Tsp;
  ffz.Lwdown = 0.7f * kT4_float(airtemp);
  ffz.Swdown = C.Swdown;
  float icing = 0;
  for (int k = 0; k < C.number; k++) {
    const float lwc = (float)((double)lwc0 * E[k]);
    ffz.rw = lwc * Vdcomp * Nf * tdur;
    const float N = mincog_bisection(ffz, C.bisect_iter);
    tr.level(C.bisect_iter);
    icing += ffz.rw * (N < 0 ? 0.f : (1 < N ? 1.f : N));
  }
  return ::fabsf(icing / (float)C.number) * (float)(3600.0 * 100.0 / 890.0);
}

// ---- host side: argument checks and the per-call constants
// 1: computed.  0: the reference's `false` (:195-201, :688).  -1: the level count (zmax - zmin) * 2 + 1 does not fit an
// int, where the reference's conversion is undefined.
inline int icing_consts(int model, float vs, float alpha, float zmin, float zmax, int alt, IcingConsts* C)
{
  if (vs < 0 || alpha < 0 || zmin < 0 || zmax < 0 || zmax < zmin || std::fmod((double)(zmax - zmin), 1.0) != 0)
    return 0;
  const float num = zmax - zmin;
  if (model == MODSTALL) {
    const double n = (double)num * 2 + 1;
    if (!(n < 2147483648.0))
      return -1;
    C->number = (int)n;
  } else {
    const float n = num * 2 + 1;
    if (!(n < 2147483648.0f))
      return -1;
    C->number = (int)n;
  }
  C->model = model;
  C->alt = alt;
  const volatile float lo = -0.5f, hi = 1.3f, eps = 1e-5f; // not folded: the reference's compiler folds log2f, the host evaluates it
  const int it = (int)std::log2((hi - lo) / eps);
  C->bisect_iter = it < 100 ? it : 100;
  C->vs = vs;
  C->vs_cos_d = (double)vs * std::cos((double)alpha);
  C->cos_d = std::cos((double)alpha);
  C->cos_alpha = (float)std::cos((double)alpha);
  C->sin_beta = (float)std::sin((double)alpha);
  const float beta_deg = (float)((double)alpha * (180 / PI));
  C->drag = (float)(-0.0046 * (double)beta_deg + 2.1912);
  const float Vf = (float)((1 + std::cos(85 * PI / 180)) / 2);
  C->Swdown = 0 * Vf;
  const float br[2] = {(float)(91 * PI / 180), (float)PI};
  for (int k = 0; k < 2; ++k) {
    const float s = std::sin(br[k]);
    C->br_sin2[k] = s * s;
    C->br_cos[k] = std::cos(br[k]);
    C->br_cos2[k] = std::cos(2 * br[k]);
  }
  return 1;
}

// the per-level factor exp(-0.55 * (zmin + 0.5 * k)), the same for every cell
inline double icing_level_factor(float zmin, int k)
{
  return std::exp(-0.55 * ((double)zmin + 0.5 * k));
}

} // namespace mifc_icing

#endif // MIFC_ICING_CELL_H
