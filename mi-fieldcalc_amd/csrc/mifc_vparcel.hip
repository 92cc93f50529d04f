// mifc_vparcel.hip -- the lifted parcel over level batches: CAPE, CIN, LCL, LFC, EL and the parcel temperature at every
// level (mifc_vparcel_hlevels / mifc_vparcel_fields / mifc_vparcel_levels, include/mifc.h; EXTENSION: the reference lifts
// a parcel across ONE layer only, in showalterIndex).
//
// The walk is the one of mifc_vcumul.hip: consecutive lanes own consecutive cells, four each through 16-byte loads
// (V = 4) or one each (V = 1), a lane keeps its cells for the whole walk, three level slots rotate with the next levels
// in flight, the per-level scalars come through the constant address space.  A level brings t and, in the `fields` form,
// p; what leaves is the optional tparcel level and, behind the walk, the planes.  The source -- a level of the batch or
// three planes -- is read in front of the walk, which then begins at the position behind it (a source level) or at
// position 0 with every cell waiting for its first pressure below p_src (source planes): one body serves both.
//
// The work is arithmetic.  Per cell and level: the dry step (x^kappa from the LDS tables of mifc_device.h, one float
// quotient), one lookup in the saturation-pressure table (LDS), one double log.  The seven adjustment trips of
// showalterIndex (FieldCalculations.cc:948-960, the arithmetic of PW_SHOWALTER in mifc_pointwise.hip with its bit-exact
// replacements of the float divisions) are entered only when a ballot shows a saturated lane in the wave and left when
// every lane has met the reference's `break`; what a lane keeps of a trip is a per-lane select, so a cell's bits do not
// depend on the wave's company.  The crossings (LCL, LFC, EL) are rare per-lane events: their divisions and exp sit in
// branches.  Per cell the lane carries tcl, qcl, pi and p of the previous point (float), ln p, B and the deficit of the
// previous point and the two sums (double), plcl / plfc / pel (float) and one word of bits.  Undefined cells are counted
// by ballot into LDS and leave the workgroup as one atomic per counter that is not zero.
#include "mifc_column_walk.h"
#include "mifc_device.h"
#include "mifc_kernels.h"

namespace mifc {

namespace {

#define VP_K_CPLR (MIFC_K_XLH / (MIFC_K_R / MIFC_K_CP)) // MetConstants.h:42
#define VP_K_EXL (MIFC_K_EPS * MIFC_K_XLH)

// (VP_STEP, VP_ADJ, VP_RUN: this level's step took place / entered the trips / is still in them -- per-lane facts kept in the
// cell's word, not as wave masks that live through the level)
enum : unsigned int { VP_SAT = 1u, VP_LFC = 2u, VP_EL = 4u, VP_ALIVE = 8u, VP_STARTED = 16u, VP_STEP = 32u, VP_ADJ = 64u, VP_RUN = 128u };

// tcl / cp, bit for bit (PW_SHOWALTER: checked against a / 1004 for every finite float with a normal or zero quotient)
__device__ __forceinline__ float over_cp(float tcl)
{
  const float inv_cp = (float)(1.0 / (double)MIFC_K_CP);
  const float q0 = tcl * inv_cp;
  return __builtin_fmaf(__builtin_fmaf(-MIFC_K_CP, q0, tcl), inv_cp, q0);
}

// One trip of FieldCalculations.cc:949-959 on (tcl, qcl) at pressure p; false = the reference's `break` (the state stays).
// rp: the refined double reciprocal of p, or 0 = plain division.  (eps * esat) / p as the double product with rp IS the
// float quotient: a quotient of two floats is never closer than 2^-49 (relative) to a rounding boundary of float, the
// product is within 2^-51 of it; the caller gives rp only where no quotient of a table value can be subnormal.
__device__ __forceinline__ bool adjust_trip(const float* tab, float& tcl, float& qcl, float p, double rp)
{
  const float tq = over_cp(tcl);
  const Ewt e2(tq - MIFC_K_T0);
  const float esat = e2.value(tab);
  const float qsat = rp != 0. ? (float)((double)(MIFC_K_EPS * esat) * rp) : MIFC_K_EPS * esat / p;
  float dq = qcl - qsat;
  // the two / tcl: the compiler's own sequence without its operand scaling, the refined reciprocal shared (PW_SHOWALTER);
  // tcl is a temperature the table covers times cp wherever the result is kept
  float rc = __builtin_amdgcn_rcpf(tcl);
  rc = __builtin_fmaf(__builtin_fmaf(-tcl, rc, 1.0f), rc, rc);
  auto over_tcl = [&](float a) {
    float q = a * rc;
    q = __builtin_fmaf(__builtin_fmaf(-tcl, q, a), rc, q);
    return __builtin_fmaf(__builtin_fmaf(-tcl, q, a), rc, q);
  };
  const float num1 = VP_K_CPLR * qcl;
  float a1 = over_tcl(num1);
  if (__builtin_expect(!(__builtin_fabsf(num1) >= 0x1p-64f && __builtin_fabsf(num1) < 0x1p64f), 0))
    a1 = num1 / tcl;
  const float a2 = over_tcl(VP_K_EXL);
  const double den = 1. + (double)(a1 * a2);
  dq = (float)quotient((double)dq, den, shared_reciprocal(den));
  const bool ok = e2.ok();
  qcl = ok ? qcl - dq : qcl;
  tcl = ok ? tcl + dq * MIFC_K_XLH : tcl;
  return ok;
}

// what a cell carries through the walk
struct Parcel
{
  float tcl, qcl, pi, p;  // state (rule 2); pi and p of the previous point
  double lnp, B, d;       // ln p, buoyancy and deficit qsat - qcl of the previous point
  double cape, cin;       // the sums of rule 8
  float plcl, plfc, pel;
  unsigned int bits;      // VP_*
};

// rule 8 on one piece (Ba, la) -> (Bb, lb) of the piecewise linear B; sat: the piece lies at or above the LCL
__device__ __forceinline__ void piece(Parcel& s, double Ba, double Bb, double la, double lb, bool sat)
{
  const double h = la - lb;
  const bool both = Ba > 0. && Bb > 0., up = !(Ba > 0.) && Bb > 0., down = Ba > 0. && !(Bb > 0.);
  double pos = 0., neg = 0., lx = la;
  if (up || down) {
    const double w0 = Ba / (Ba - Bb);
    lx = la + w0 * (lb - la);
    const double h1 = w0 * h, h2 = h - h1;
    const double A1 = (Ba * 0.5) * h1, A2 = (Bb * 0.5) * h2;
    pos = up ? A2 : A1;
    neg = up ? A1 : A2;
  } else {
    const double A = ((Ba + Bb) * 0.5) * h;
    pos = both ? A : 0.;
    neg = both ? 0. : A;
  }
  if ((s.bits & VP_LFC) == 0) {
    s.cin = s.cin + neg;
    if (sat && up) {
      s.bits |= VP_LFC;
      s.plfc = (float)exp(lx);
      s.cape = s.cape + pos;
    }
  } else {
    s.cape = s.cape + pos;
    if (down) {
      s.bits |= VP_EL;
      s.pel = (float)exp(lx);
    }
  }
}

template <int KIND, int V>
__global__ __launch_bounds__(256, 2) void vparcel_kernel(const VparcelParams P)
{
  constexpr int R = 3; // level slots
  extern __shared__ unsigned int s_cnt[]; // [VPARCEL_PLANES + nlev]
  __shared__ __attribute__((aligned(8))) float s_ewt[MIFC_EWT_LDS];
  __shared__ double s_kappa[MIFC_KAPPA_LDS];
  const int nlev = P.nlev;
  const bool lds = P.lds_counts != 0;
  if (lds)
    for (int j = threadIdx.x; j < VPARCEL_PLANES + nlev; j += 256)
      s_cnt[j] = 0;
  ewt_table_init(s_ewt, false);
  const PowTables PT = kappa_tables_init(s_kappa); // one barrier for the tables and the counters

  const long i0 = ((long)blockIdx.x * 256 + threadIdx.x) * V;
  const long left = (long)P.n - i0;
  const int n_cells = left < 0 ? 0 : (left < V ? (int)left : V); // this lane's cells inside the launch
  // a wave-uniform base plus the lane's 32-bit byte offset inside the workgroup; lanes past the end walk the workgroup's
  // first column group and neither store nor count (mifc_vlayer.hip)
  const long block0 = (long)blockIdx.x * (256 * V);
  const unsigned int lane_bytes = n_cells > 0 ? threadIdx.x * (unsigned int)(V * sizeof(float)) : 0u;
  auto lane_of = [&](const float* uniform_base) { return reinterpret_cast<const float*>(reinterpret_cast<const char*>(uniform_base) + lane_bytes); };
  const float undef = P.undef;
  const ConstFloats ab = (ConstFloats)(unsigned long long)P.ab;
  const ConstWords lev_bits = (ConstWords)(unsigned long long)P.lev_bits;
  const ConstFloats lev_p = (ConstFloats)(unsigned long long)P.lev_p;
  typedef WalkLevel<1, V> Level;
  const float nan = __int_as_float(0x7fc00000);
  const bool want_tp = P.tparcel != nullptr;

  // position j of the walk is this level; the source level sits at position js (none: -1)
  const int first = P.from != 0 ? nlev - 1 : 0, step = P.from != 0 ? -1 : 1;
  auto level_of = [&](int j) { return first + j * step; };
  const int js = P.src_level < 0 ? -1 : (P.from != 0 ? nlev - 1 - P.src_level : P.src_level);

  auto load = [&](Level& L, int j) {
    const long off = (long)walk_here(level_of(j)) * P.in_stride + block0; // (opaque: no induction variable per pointer)
    if constexpr (KIND == VDERIV_FIELD)
      walk_load<V>(L.c, lane_of(P.coord + off));
    walk_load<V>(L.x[0], lane_of(P.t + off));
  };

  float ps[V];
  if constexpr (KIND == VDERIV_HYBRID) {
    walk_load<V>(ps, lane_of(P.coord + block0));
#pragma unroll
    for (int c = 0; c < V; ++c)
      ps[c] = (P.ps_all != 0 || ps[c] != undef) ? ps[c] : nan;
  }
  // rule 1: the pressure of level k, NaN where it is not defined
  auto pressure_of = [&](int k, unsigned int bits, const Level& L, int c) -> float {
    if constexpr (KIND == VDERIV_LEVELS) {
      return lev_p[k];
    } else if constexpr (KIND == VDERIV_HYBRID) {
      const float prod = ab[nlev + k] * ps[c]; // p_hlevel, FieldCalculations.cc:303: the product rounded, then the sum
      return ab[k] + prod;
    } else {
      return (((bits >> VINTERP_COORD_BIT) & 1u) != 0 || L.c[c] != undef) ? L.c[c] : nan;
    }
  };
  auto pi_of = [&](int k, float p) -> float {
    if constexpr (KIND == VDERIV_LEVELS)
      return lev_p[nlev + k];
    else
      return MIFC_K_CP * pidcp_of(PT, p);
  };

  auto count = [&](int counter, unsigned int n) {
    if (n != 0 && (walk_here_v(threadIdx.x) & 63) == 0) {
      if (lds)
        atomicAdd(&s_cnt[counter], n);
      else
        atomicAdd(P.n_undefined + counter, (u64)n);
    }
  };
  // one tparcel level: the cells that are not `have` are undef and counted
  auto put_level = [&](int k, const float (&tp)[V], const bool (&have)[V]) {
    if (!want_tp)
      return;
    const int n_mine = (int)walk_here_v((unsigned int)n_cells);
    float res[V];
    bool whole = true;
#pragma unroll
    for (int c = 0; c < V; ++c) {
      res[c] = have[c] ? tp[c] : undef;
      whole = whole && (have[c] || c >= n_mine);
    }
    if (__builtin_amdgcn_ballot_w64(!whole) != 0) {
      unsigned int n = 0;
#pragma unroll
      for (int c = 0; c < V; ++c)
        n += (unsigned int)__popcll(__builtin_amdgcn_ballot_w64(!have[c] && c < n_mine));
      count(VPARCEL_PLANES + k, n);
    }
    walk_store<V>(P.tparcel + (long)walk_here(k) * P.out_stride + i0, res, n_mine);
  };

  // ---- the source (rules 1 and 2)
  Parcel s[V];
  {
    float T[V], q[V], p[V], pi[V];
    bool ok[V];
    if (js >= 0) {
      const int k = P.src_level;
      const unsigned int bits = lev_bits[k];
      Level L;
      const long off = (long)k * P.in_stride + block0;
      if constexpr (KIND == VDERIV_FIELD)
        walk_load<V>(L.c, lane_of(P.coord + off));
      walk_load<V>(T, lane_of(P.t + off));
#pragma unroll
      for (int c = 0; c < V; ++c) {
        p[c] = pressure_of(k, bits, L, c);
        pi[c] = pi_of(k, p[c]);
        ok[c] = ((bits & 1u) != 0 || T[c] != undef) && T[c] == T[c];
      }
    } else {
      walk_load<V>(T, lane_of(P.t_src + block0));
      walk_load<V>(p, lane_of(P.p_src + block0));
#pragma unroll
      for (int c = 0; c < V; ++c) {
        ok[c] = (P.tsrc_all != 0 || T[c] != undef) && T[c] == T[c] && (P.psrc_all != 0 || p[c] != undef);
        pi[c] = MIFC_K_CP * pidcp_of(PT, p[c]);
      }
    }
    walk_load<V>(q, lane_of(P.q_src + block0));
#pragma unroll
    for (int c = 0; c < V; ++c) {
      ok[c] = ok[c] && (P.qsrc_all != 0 || q[c] != undef) && q[c] == q[c] && p[c] > 0.f;
      Parcel& a = s[c];
      a.tcl = MIFC_K_CP * T[c];
      a.qcl = q[c];
      a.pi = pi[c];
      a.p = p[c];
      const Ewt e(over_cp(a.tcl) - MIFC_K_T0);
      ok[c] = ok[c] && e.ok(); // a source the table does not cover is not usable
      const float qsat = MIFC_K_EPS * e.value(s_ewt) / p[c];
      a.d = (double)qsat - (double)a.qcl;
      a.lnp = log((double)p[c]);
      a.B = 0.;
      a.cape = 0.;
      a.cin = 0.;
      a.plcl = p[c]; // rule 5: the source where it is saturated
      a.plfc = 0.f;
      a.pel = 0.f;
      a.bits = (ok[c] ? VP_ALIVE : 0u) | (js >= 0 ? VP_STARTED : 0u) | (!(a.qcl < qsat) ? VP_SAT : 0u);
    }
    // the levels in front of the source are not walked; the source level holds the parcel itself
    bool none[V];
    float tp[V];
#pragma unroll
    for (int c = 0; c < V; ++c) {
      none[c] = false;
      tp[c] = over_cp(s[c].tcl);
    }
    for (int j = 0; j < js; ++j)
      put_level(level_of(j), tp, none);
    if (js >= 0)
      put_level(P.src_level, tp, ok);
  }

  // ---- one position of the walk (rules 3 to 8)
  auto advance = [&](const Level& L, int j) {
    const int k = walk_here(level_of(j)); // (opaque: the level's scalars are fetched here, not for three positions ahead)
    const unsigned int bits = lev_bits[k];
    float pb[V], tb[V];
    double db[V];
#pragma unroll
    for (int c = 0; c < V; ++c) {
      Parcel& a = s[c];
      const float p = pressure_of(k, bits, L, c), t = L.x[0][c];
      const bool below = p < a.p; // (false for a NaN)
      const bool walk = (a.bits & VP_ALIVE) != 0 && ((a.bits & VP_STARTED) != 0 || below);
      bool usable = below && p > 0.f && ((bits & 1u) != 0 || t != undef) && t == t;
      const float pi = pi_of(k, p);
      const float ratio = pi / a.pi;
      const float tcl = a.tcl * ratio; // the dry step: the quotient rounded, then the product
      const Ewt e(over_cp(tcl) - MIFC_K_T0);
      usable = usable && e.ok(); // a parcel that leaves the table ends the walk
      const float qsat = MIFC_K_EPS * e.value(s_ewt) / p;
      const bool stepped = walk && usable, adj = stepped && a.qcl > qsat;
      db[c] = (double)qsat - (double)a.qcl;
      pb[c] = p;
      tb[c] = t;
      unsigned int w = a.bits & ~(VP_STEP | VP_ADJ | VP_RUN);
      w = (walk && !usable) ? w & ~VP_ALIVE : w;
      w |= walk ? VP_STARTED : 0u;
      w |= stepped ? VP_STEP : 0u;
      w |= adj ? (VP_ADJ | VP_RUN) : 0u;
      a.bits = walk_here_v(w);
      a.tcl = stepped ? tcl : a.tcl;
      a.pi = stepped ? pi : a.pi;
    }

    unsigned int any = 0;
#pragma unroll
    for (int c = 0; c < V; ++c)
      any |= s[c].bits;
    if (__builtin_amdgcn_ballot_w64((any & VP_ADJ) != 0) != 0) {
      // somewhere in the wave a parcel is saturated: the seven trips, each lane keeping what is its own
      double rp[V];
#pragma unroll
      for (int c = 0; c < V; ++c)
        rp[c] = (pb[c] >= 0x1p-40f && pb[c] < 0x1p40f) ? shared_reciprocal((double)pb[c]) : 0.;
      for (int it = 0; it < 7; ++it) {
        unsigned int go = 0;
#pragma unroll
        for (int c = 0; c < V; ++c) {
          float tcl = s[c].tcl, qcl = s[c].qcl;
          const bool ok = adjust_trip(s_ewt, tcl, qcl, pb[c], rp[c]);
          s[c].bits = ok ? s[c].bits : s[c].bits & ~VP_RUN;
          const bool run = (s[c].bits & VP_RUN) != 0;
          s[c].tcl = run ? tcl : s[c].tcl;
          s[c].qcl = run ? qcl : s[c].qcl;
          go |= s[c].bits;
        }
        if (__builtin_amdgcn_ballot_w64((go & VP_RUN) != 0) == 0)
          break;
      }
    }

    float tp[V];
    bool stepped[V];
#pragma unroll
    for (int c = 0; c < V; ++c) {
      Parcel& a = s[c];
      tp[c] = over_cp(a.tcl);
      const double lnp = log((double)pb[c]);
      stepped[c] = (a.bits & VP_STEP) != 0;
      if (stepped[c]) {
        const double B = (double)tp[c] - (double)tb[c]; // rule 4
        if ((a.bits & (VP_ADJ | VP_SAT)) == VP_ADJ) {
          // rule 5: the zero of the deficit between the last unsaturated and the first saturated point
          const double w = a.d / (a.d - db[c]);
          const double lm = a.lnp + w * (lnp - a.lnp);
          const double Bm = a.B + w * (B - a.B);
          piece(a, a.B, Bm, a.lnp, lm, false);
          a.bits |= VP_SAT;
          a.plcl = (float)exp(lm);
          if (Bm > 0.) { // rule 6: the LFC is the LCL
            a.bits |= VP_LFC;
            a.plfc = a.plcl;
          }
          piece(a, Bm, B, lm, lnp, true);
        } else {
          piece(a, a.B, B, a.lnp, lnp, (a.bits & VP_SAT) != 0);
        }
        a.lnp = lnp;
        a.B = B;
        a.d = db[c];
        a.p = pb[c];
      }
    }
    put_level(k, tp, stepped);
  };

  Level L[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int c = 0; c < V; ++c) {
      L[r].c[c] = 0.f;
      L[r].x[0][c] = 0.f;
    }
  }
  const int jb = js + 1;
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (jb + r < nlev)
      load(L[r], jb + r);
  for (int j0 = jb; j0 < nlev; j0 += R) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int j = j0 + r; // position j sits in slot (j - jb) % R = r
      if (j < nlev) {
        advance(L[r], j);
        if (j + R < nlev)
          load(L[r], j + R);
      }
    }
  }

  // ---- the planes (rules 5 to 9)
  {
    const int n_mine = n_cells;
    float out[VPARCEL_PLANES][V];
    bool have[VPARCEL_PLANES][V];
#pragma unroll
    for (int c = 0; c < V; ++c) {
      const Parcel& a = s[c];
      const bool alive = (a.bits & VP_ALIVE) != 0, sat = alive && (a.bits & VP_SAT) != 0, lfc = alive && (a.bits & VP_LFC) != 0;
      const double cape = (double)MIFC_K_R * a.cape, cin = (double)MIFC_K_R * a.cin;
      have[0][c] = alive;
      out[0][c] = lfc ? (float)cape : 0.f;
      have[1][c] = lfc;
      out[1][c] = (float)cin;
      have[2][c] = sat;
      out[2][c] = a.plcl;
      have[3][c] = lfc;
      out[3][c] = a.plfc;
      have[4][c] = lfc && (a.bits & VP_EL) != 0 && !(a.B > 0.); // rule 7: undef where B > 0 at the last walked point
      out[4][c] = a.pel;
    }
#pragma unroll
    for (int o = 0; o < VPARCEL_PLANES; ++o) {
      float* dst = P.planes[walk_here(o)]; // (fetched from the kernel arguments here, not kept in SGPRs through the walk)
      if (dst == nullptr)
        continue;
      unsigned int n = 0;
#pragma unroll
      for (int c = 0; c < V; ++c) {
        out[o][c] = have[o][c] ? out[o][c] : undef;
        n += (unsigned int)__popcll(__builtin_amdgcn_ballot_w64(!have[o][c] && c < n_mine));
      }
      count(o, n);
      walk_store<V>(dst + i0, out[o], n_mine);
    }
  }

  if (lds) {
    __syncthreads();
    for (int j = threadIdx.x; j < VPARCEL_PLANES + nlev; j += 256) {
      const unsigned int n = s_cnt[j];
      if (n != 0)
        atomicAdd(P.n_undefined + j, (u64)n);
    }
  }
}

template <int KIND>
hipError_t launch_v(const VparcelParams& P, hipStream_t stream)
{
  const int per_block = 256 * (P.vec4 ? 4 : 1);
  const dim3 grid((unsigned int)(((long)P.n + per_block - 1) / per_block)), block(256);
  const size_t lds = P.lds_counts ? (size_t)(VPARCEL_PLANES + P.nlev) * sizeof(unsigned int) : 0;
  if (P.vec4)
    hipLaunchKernelGGL((vparcel_kernel<KIND, 4>), grid, block, lds, stream, P);
  else
    hipLaunchKernelGGL((vparcel_kernel<KIND, 1>), grid, block, lds, stream, P);
  return hipGetLastError();
}

} // namespace

hipError_t launch_vparcel(const VparcelParams& prm, hipStream_t stream)
{
  if (prm.n <= 0)
    return hipSuccess;
  if (prm.nlev < 2 || (prm.from != 0 && prm.from != 1) || prm.src_level < -1 || prm.src_level >= prm.nlev || prm.q_src == nullptr ||
      (prm.src_level < 0 && (prm.t_src == nullptr || prm.p_src == nullptr)))
    return hipErrorInvalidValue;
  VparcelParams P = prm;
  // the workgroup's counters in LDS where they fit beside the tables
  P.lds_counts = (size_t)(VPARCEL_PLANES + P.nlev) * sizeof(unsigned int) <= 16384 ? 1 : 0;
  switch (P.kind) {
  case VDERIV_HYBRID:
    return launch_v<VDERIV_HYBRID>(P, stream);
  case VDERIV_FIELD:
    return launch_v<VDERIV_FIELD>(P, stream);
  case VDERIV_LEVELS:
    return launch_v<VDERIV_LEVELS>(P, stream);
  default:
    return hipErrorInvalidValue;
  }
}

} // namespace mifc
