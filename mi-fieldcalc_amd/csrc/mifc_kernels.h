// mifc_kernels.h -- host-callable launchers of the gfx950 kernels.
// Everything here takes DEVICE pointers and a stream and only enqueues work.
#ifndef MIFC_KERNELS_H
#define MIFC_KERNELS_H

#include <hip/hip_runtime.h>

#include "mifc_env.h"
#include "mifc_stencil_limits.h" // the launch-size thresholds the stencil launchers share

namespace mifc {

typedef unsigned long long u64;

// ---------------------------------------------------------------- elementwise
enum EwiseOp {
  EW_VECTORABS = 0, // FieldCalculations.cc:1819
  EW_TEMP = 1,      // pleveltemp :328, hleveltemp :1046, aleveltemp :1310
  EW_HUM = 2,       // plevelhum :400, hlevelhum :1145, alevelhum :1394
  EW_CVHUM_TD = 3,  // cvhum compute 1..3 :1759-1785
  EW_CVHUM_RH = 4,  // cvhum compute 4,5 :1787-1811
  EW_MOMENTUM_X = 5, // momentumXcoordinate :2351: in0 = v, in1 = xmapr, in2 = fcoriolis
  EW_MOMENTUM_Y = 6, // momentumYcoordinate :2387: in0 = u, in1 = ymapr, in2 = fcoriolis
  // kernel-internal: EW_TEMP with a scalar pressure and compute 1..3 (pleveltemp's plain conversions) as a
  // small kernel of its own; launch_ewise() selects it, callers keep passing EW_TEMP
  EW_TEMP_SCALAR = 7,
  // likewise: EW_TEMP with a hybrid / field pressure and compute 1..3 (no saturation table in the kernel),
  // EW_HUM for the two kinds that need no table inverse (q <-> RH)
  EW_TEMP_PLAIN = 8,
  EW_HUM_DIRECT = 9
};
enum PressureSource { PS_SCALAR = 0, PS_HYBRID = 1, PS_FIELD = 2 };
enum HumKind { HUM_Q_RH = 0, HUM_RH_Q = 1, HUM_Q_TD = 2, HUM_RH_TD = 3 };
// which extra undefined test the pressure field gets (hlevelhum :1187, alevelhum :1429)
enum PTest { PT_NONE = 0, PT_FULL = 1 /* is_defined(p) */, PT_NEQ = 2 /* p != undef only */ };

struct EwiseParams
{
  int op;
  int n;          // cells per field
  int all_defined; // input flag == ALL_DEFINED: no per-cell tests (FieldCalculations.h:47-50)
  int count;      // 0: operator does not count / touch the flag (pleveltemp 1..3)
  int psrc;       // PressureSource
  int ptest;      // PTest
  int compute;    // remapped compute (temp: 1..5, others see kernel)
  int kind;       // HumKind
  int from_theta; // humidity: t is potential temperature
  float p;        // PS_SCALAR: pressure
  float pidcp;    // PS_SCALAR: powf(p*p0inv,kappa) evaluated on the host like the reference (:347)
  float pi;       // PS_SCALAR: host-side pi (pidcp*cp for temp, cp*pidcp for hum)
  float tconv;    // plevelhum :436 / cvhum :1753
  float tdconv;   // :437, :1181, :1423, :1754
  float alevel, blevel;
  float unit_scale; // cvhum :1746-1750
  int nx;           // momentum coordinates: row length (cell index -> column / row)
  int cell0;        // index of in0[0] inside the field (non-zero only for the scalar tail launch)
  float fcormin;    // momentum coordinates: |fcoriolisMin| (:2366)
  float undef;
  const float* in0; // u | t
  const float* in1; // v | hum
  const float* in2; // ps | p field
  float* out;
  u64* n_undefined; // device counter (may be null when count == 0)
  // big launches: the workgroups leave their counts in partials[blockIdx.x] (plain stores) and a one-workgroup kernel
  // behind the launch adds them up -- no queue of same-address atomics (mifc_device.h: undefined-cell counting)
  unsigned int* partials;
  int partials_cap;
};

hipError_t launch_ewise(const EwiseParams& prm, hipStream_t stream);

// recommended distance (in floats) between the levels of a device-resident batch of fields of n cells
size_t padded_level_stride(size_t n);

// Fused derived variables over hybrid levels (mifc_derived.hip), BASELINE.json config 2 x nlev.
struct DerivedParams
{
  int n;    // cells per level
  int nlev;
  const float *u, *v, *t, *h, *ps; // h: humidity input (q or RH); ps shared by all levels
  const float *alevel, *blevel;    // device float[nlev]
  float *ff, *temp, *hum, *td;     // outputs, any may be null: vectorabs | hleveltemp | hlevelhum | a second hlevelhum variant
  float* dd;                       // EXTENSION output (may be null): wind direction from u, v, see wind_direction() in mifc_device.h
  int temp_compute;                // hleveltemp compute after the unit remap, 1..5
  int hum_code, td_code;           // 1 + HumKind + 4 * from_theta (0 = none)
  float hum_tdconv, td_tdconv;     // :1181
  const unsigned char* wind_all_defined;   // device u8[nlev]
  const unsigned char* thermo_all_defined; // device u8[nlev]
  int every_level_all_defined;             // host hint: skip all tests
  float undef;
  u64 *cnt_ff, *cnt_temp, *cnt_hum, *cnt_td, *cnt_dd; // device u64[nlev] each (level 0 of this launch first)
  // small batches (nlev <= 8, e.g. the single level of BASELINE.json config 2)
  // carry the per-level scalars in the kernel arguments: no upload before the launch
  int n_inline; // != 0: use the arrays below instead of the device arrays above
  float a_inline[8], b_inline[8];
  unsigned char wind_inline[8], thermo_inline[8];
};
hipError_t launch_derived_levels(const DerivedParams& prm, hipStream_t stream);

// ------------------------------------------- the rest of the pointwise catalogue
// (FieldCalculations.cc line of each operator in the comment)
enum PwOp {
  PW_PLEVELTHE = 0,   // plevelthe :369: in = t, rh
  PW_XLEVELTHE,       // hlevelthe :1100 (hybrid) / alevelthe :1355: in = t, q, ps|p
  PW_PDUCT,           // plevelducting :597: in = t, h
  PW_XDUCT,           // hlevelducting :1219 (hybrid) / alevelducting :1460: in = t, h, ps|p
  PW_HPRESSURE,       // hlevelpressure :1276
  PW_DZ2TMEAN,        // pleveldz2tmean :466
  PW_KINDEX,          // :745
  PW_DUCTINDEX,       // :816
  PW_SHOWALTER,       // :872
  PW_BOYDEN,          // :973
  PW_SWEAT,           // :1016
  PW_SOUNDSPEED,      // seaSoundSpeed :1555
  PW_ADDCONST,        // cvtemp :1608 (the conversion pass)
  PW_ABSHUM,          // :1676
  PW_WINDCOOLING,     // :2181
  PW_UNDERCOOLED,     // underCooledRain :2231
  PW_FLIGHTLEVEL,     // pressure2FlightLevel :2311
  PW_SNOWCM,          // snow_in_cm :3063
  PW_CLASSES,         // values2classes :2462
  PW_MINMAX_FIELDS,   // minvalueFields :2501 (compute 1), maxvalueFields :2516 (2)
  PW_MINMAX_CONST,    // minvalueFieldConst :2507 (1), maxvalueFieldConst :2522 (2)
  PW_MATH,            // abs 1, log10 2, pow10 3, log 4, exp 5, power 6 (:2531-2563)
  PW_REPLACE,         // replaceUndefined :2565 (1), replaceDefined :2587 (2), copy (3)
  PW_FILL,            // fillUndef :76 and the std::fill branches of replace*
  PW_FIELD_OP_FIELD,  // fieldOPERfield :2611
  PW_FIELD_OP_CONST,  // fieldOPERconstant :2627
  PW_CONST_OP_FIELD,  // constantOPERfield :2647
  // FieldCalculationsVesselIcing.cc: vesselIcingOverland :77 (compute 1), vesselIcingMertins :114 (2);
  // in = airtemp, seatemp, u, v, sal, aice
  PW_VESSEL_ICING,
  // EXTENSION, no reference function (BASELINE.json names "wind direction from u/v"):
  // meteorological direction the wind blows FROM, degrees clockwise from north; in = u, v
  PW_WINDDIR
};

struct PwParams
{
  int op;
  int n;
  int all_defined;          // input flag == ALL_DEFINED
  int count;                // operator classifies its output (the "Undef" helper templates :142-179 and the hand-written loops)
  int compute;
  int hybrid;               // p = s[0] + s[1] * ps (h-level) instead of the p field (a-level)
  int may_keep;             // some cells may stay unwritten: the kernel starts from the output's content
  int no_input_test;        // replace*: no is_defined test on the input
  int skip_undefined_input; // showalterIndex: an undefined input is counted but the cell is not written
  float undef;
  float s[8];  // operator scalars, evaluated on the host like the reference does
  double d[2];
  const float* in[8];
  float* out;
  u64* n_undefined;
  const float* values; // values2classes: device copy of the class limits
  int nvalues;
  unsigned int* partials; // see EwiseParams
  int partials_cap;
};
hipError_t launch_pointwise(const PwParams& prm, hipStream_t stream);
// sum and number of the defined cells (cvtemp compute 3, 4)
hipError_t launch_count_partials(const unsigned int* partials, int n, u64* counter, hipStream_t stream);
// partials[level][unit]: one workgroup per level adds its `per_level` entries to counters[level]
hipError_t launch_count_partials_levels(const unsigned int* partials, int per_level, int nlev, u64* counters, hipStream_t stream);
hipError_t launch_mean_defined(const float* f, int n, int all_defined, float undef, double* sum, unsigned long long* count, hipStream_t stream);

// ------------------------------------ reductions over ensemble members
enum EnsembleOp {
  ENS_SUM = 0,        // sumFields :2671
  ENS_MEAN = 1,       // meanValue :2696
  ENS_STDDEV = 2,     // stddevValue :2726
  ENS_EXTREME = 3,    // extremeValue :2759 (compute 1 max, 2 min, 3 index of max, 4 index of min)
  ENS_PROBABILITY = 4 // probability :2807 (compute 1..3 percent, 4..6 count)
};

struct EnsembleParams
{
  int op;
  int n;       // cells per member field
  int first;   // scalar tail launch: first cell
  int nfields; // members
  int compute;
  int all_defined;                    // sumFields / extremeValue: the one input flag
  const unsigned char* member_flags;  // device u8[nfields] (ValuesDefined of each member) or null
  int check_above, check_below;       // probability :2821-2823
  float value_above, value_below;     // :2824-2825
  int vector_ok;                      // every member field and the output are 16-byte aligned
  float undef;
  const float* const* fields; // device table of nfields device pointers
  float* out;
  // The caller's output IS a member's array (fres == fields[j], callers reduce in place): the device copy of that
  // member, else null.  The reference accumulates in fres[i] (:2681, :2707, :2776, :2838), so it reads its own running
  // result where that member was; the kernel does the same (ens_aliased).  stddevValue writes fres[i] last and is not affected.
  const float* out_member;
  u64* n_undefined;
  // up to 64 members (an ensemble: 51) travel in the kernel arguments: no table upload before the launch
  int n_inline;         // != 0: use the arrays below instead of `fields` / `member_flags`
  int has_member_flags; // with n_inline: flags_inline is meaningful
  const float* fields_inline[64];
  unsigned char flags_inline[64];
};
// the 16-byte launch (four cells per lane), which a scalar launch for the last n % 4 cells follows; else one scalar launch
inline bool ensemble_vec4(const EnsembleParams& P)
{
  return P.vector_ok && P.n >= 4;
}
hipError_t launch_ensemble(const EnsembleParams& prm, hipStream_t stream);

// ------------------------------------ percentiles across ensemble members (mifc_quantile.hip), EXTENSION
// One launch covers `nlev` levels of `n` cells each; member j's level l is mem(j) + l * stride, output q's likewise.
// Members, percentiles, outputs and the per-level ALL_DEFINED member bits travel in the kernel arguments when they fit
// (nmem <= 64, nq <= QUANTILE_KARG_Q, every level of the call < QUANTILE_KARG_LEVELS), in the device table otherwise.
// The host has validated every percentile (0 <= p <= 100) and keeps the outputs apart from the members.
const int QUANTILE_KARG_MEM = 64, QUANTILE_KARG_Q = 16, QUANTILE_KARG_LEVELS = 64;
struct QuantileTable // device memory, used when inline_args == 0
{
  const float* const* mem; // [nmem]
  float* const* out;       // [nq]
  const float* p;          // [nq]
  const u64* all_bits;     // [level][words]: bit j % 64 of word j / 64 set = member j's flag is ALL_DEFINED at that level
};
struct QuantileParams
{
  int nlev;    // levels of this launch
  int lev0;    // the call's level of the launch's level 0 (member bits, counters)
  int n;       // cells per level
  long stride; // floats between consecutive levels of every member and output of the launch
  int nmem, nq;
  int method;  // MIFC_QUANTILE_LOWER / MIFC_QUANTILE_LINEAR
  int words;   // (nmem + 63) / 64
  float undef;
  u64* n_undefined;       // [call levels]: cells without a defined member, at lev0 + l (zeroed by the caller)
  unsigned int* partials; // per-workgroup counts of big launches (see EwiseParams), or null
  int partials_cap;
  int inline_args;
  QuantileTable tab;
  const float* mem_inline[QUANTILE_KARG_MEM];
  float* out_inline[QUANTILE_KARG_Q];
  float p_inline[QUANTILE_KARG_Q];
  u64 all_inline[QUANTILE_KARG_LEVELS]; // nmem <= 64: one word per level
};
// the sorting-network capacity that holds nmem members (8, 16, 32, 64), or 0: the bisection path (nmem > 64)
inline int quantile_tier(int nmem)
{
  return nmem <= 8 ? 8 : nmem <= 16 ? 16 : nmem <= 32 ? 32 : nmem <= 64 ? 64 : 0;
}
// workgroups per level of a launch over n cells (the host sizes the partial-count buffer with it)
inline int quantile_blocks(int n)
{
  const long want = ((long)n + 255) / 256;
  return (int)(want < 1 ? 1 : (want > 65535 ? 65535 : want));
}
// big levels: the counts of a launch go through the partial-count table
inline bool quantile_partials(const QuantileParams& P)
{
  const int gx = quantile_blocks(P.n);
  return P.partials && gx >= 2048 && (long)gx * P.nlev <= (long)P.partials_cap;
}
hipError_t launch_quantiles(const QuantileParams& prm, hipStream_t stream);

// ------------------------------------ several ensemble reductions in one pass over the members (mifc_ensemble_levels.hip)
// One launch covers `nlev` levels of `n` cells each, laid out as for launch_quantiles.  The products of a call sit in
// fixed slots: 0 sumFields, 1 meanValue, 2 stddevValue, 2 + c extremeValue compute c (1..4), 7..14 probability; slot k is
// live when bit k of `live` is set, its result goes to out[k] and its undefined count to n_undefined[k * call_nlev + level].
// The product parameters are of fixed size and always travel in the kernel arguments; what grows with the call (member
// pointers, per-level member bits, per-level defined-member counts and input flags) does so up to 64 members and 64 levels
// and sits in the device table beyond.
const int ENSLV_SLOTS = 15, ENSLV_EXT0 = 2, ENSLV_PROB0 = 7, ENSLV_NPROB = 8, ENSLV_KARG_MEM = 64, ENSLV_KARG_LEVELS = 64;
struct EnsLevelsTable // device memory, used when inline_args == 0
{
  const float* const* mem;     // [nmem]
  const u64* all_bits;         // [level][words]: member j's flag is ALL_DEFINED at that level
  const u64* none_bits;        // [level][words]: member j's flag is NONE_DEFINED (probability leaves it out)
  const int* ndef;             // [level]: members not flagged NONE_DEFINED (probability's nfields_defined)
  const unsigned char* in_all; // [level]: bit 0 sumFields', bit c extremeValue compute c's input flag is ALL_DEFINED
};
struct EnsLevelsParams
{
  int nlev;      // levels of this launch
  int lev0;      // the call's level of the launch's level 0 (bits, counters)
  int call_nlev; // levels of the whole call: the distance between the counters of two slots
  int n;         // cells per level
  long stride;   // floats between consecutive levels of every member and output of the launch
  int nmem;
  int words;     // (nmem + 63) / 64
  int vector_ok; // every member and output is 16-byte aligned, and so is every level inside them
  unsigned int live;
  float undef;
  float* out[ENSLV_SLOTS];
  // probability slot i (:2821-2825) in bit i; percent: compute < 4
  unsigned int check_above, check_below, percent;
  float value_above[ENSLV_NPROB], value_below[ENSLV_NPROB];
  u64* n_undefined;       // [ENSLV_SLOTS][call_nlev], zeroed by the caller
  unsigned int* partials; // [slot][launch level][workgroup] counts of big launches (see EwiseParams), or null
  int partials_cap;
  int inline_args;
  EnsLevelsTable tab;
  const float* mem_inline[ENSLV_KARG_MEM];
  u64 all_inline[ENSLV_KARG_LEVELS], none_inline[ENSLV_KARG_LEVELS]; // nmem <= 64: one word per level
  unsigned char ndef_inline[ENSLV_KARG_LEVELS], in_all_inline[ENSLV_KARG_LEVELS];
};
// workgroups per level of a launch over n cells (the host sizes the partial-count buffer with it)
inline int ensemble_levels_blocks(int n, bool vec4)
{
  const long lanes = vec4 ? (long)(n >> 2) : (long)n, want = (lanes + 255) / 256;
  return (int)(want < 1 ? 1 : (want > 65535 ? 65535 : want));
}
inline bool ensemble_levels_vec4(const EnsLevelsParams& P)
{
  return P.vector_ok && P.n >= 4 && (P.n & 3) == 0;
}
// The kernel instance a launch takes and whether its counts go through the partial-count table: the launcher dispatches
// on it and mifc_last_ensemble_form reports it.  c == 1 is the one scalar shape with everything in it; with c == 4 `np` is
// the room for probability slots (0, 3 or 8), and a list with Welford, one to three probabilities and no flagged product
// runs on the flagged shape (see launch_ensemble_levels).
struct EnsLevelsShape
{
  int c;
  bool welford, flagged;
  int np;
  bool partials;
};
inline EnsLevelsShape ensemble_levels_shape(const EnsLevelsParams& P)
{
  EnsLevelsShape s;
  const bool vec4 = ensemble_levels_vec4(P);
  const int gx = ensemble_levels_blocks(P.n, vec4);
  const int np = __builtin_popcount(P.live >> ENSLV_PROB0); // the host fills the probability slots from the first
  s.c = vec4 ? 4 : 1;
  s.welford = !vec4 || ((P.live >> 2) & 1u);
  s.np = !vec4 ? ENSLV_NPROB : np == 0 ? 0 : np <= 3 ? 3 : 8;
  s.flagged = !vec4 || (P.live & 0x79u) != 0 || (s.welford && s.np == 3); // slots 0, 3..6
  s.partials = P.partials && gx >= 2048 && (long)ENSLV_SLOTS * gx * P.nlev <= (long)P.partials_cap;
  return s;
}
hipError_t launch_ensemble_levels(const EnsLevelsParams& prm, hipStream_t stream);

// ------------------------------------ level batches to constant surfaces (mifc_vinterp.hip), EXTENSION
// One launch walks the `nlev` levels of `n` columns once and serves up to VINTERP_PASS targets; the host launches a second
// pass for targets beyond that.  Field f's level k is fields[f] + k * in_stride, its result for call target t
// out[f] + t * out_stride; `coord` is ps (hybrid: n floats) or the coordinate batch (field: laid out like a field).
// The per-level scalars sit in a device table (`ab`: alevel[nlev] then blevel[nlev]; `lev_bits[k]`: bit f = field f is
// flagged ALL_DEFINED at level k, bit VINTERP_COORD_BIT = the coordinate is), the targets of the pass in the kernel
// arguments.  vec4: four cells per lane through 16-byte loads -- every pointer 16-byte aligned, both strides multiples
// of 4, and the four floats of a lane's group readable even where the group straddles n (the staged band is padded; a
// device batch qualifies when n is a multiple of 4).  Otherwise one cell per lane.
const int VINTERP_MAX_FIELDS = 8, VINTERP_PASS = 32, VINTERP_MAX_TARGETS = 64, VINTERP_COORD_BIT = 8;
struct VinterpParams
{
  int hybrid;     // coordinate kind: 1 = alevel + blevel * ps, 0 = field
  int method;     // MIFC_VINTERP_LINEAR / MIFC_VINTERP_LOG
  int nfields;    // 1 .. VINTERP_MAX_FIELDS
  int n;          // columns of this launch
  int nlev;       // >= 2
  int nt;         // targets of this pass, 1 .. VINTERP_PASS
  int t0;         // the call's target of the pass' target 0 (outputs, counters)
  int nt_call;    // targets of the whole call: the distance between the counters of two fields
  int vec4;
  int ps_all;     // hybrid: fdef_ps == ALL_DEFINED
  float undef;
  long in_stride, out_stride;
  const float* fields[VINTERP_MAX_FIELDS];
  float* out[VINTERP_MAX_FIELDS];
  const float* coord;
  const float* ab;
  const unsigned int* lev_bits;
  u64* n_undefined;                // [nfields][nt_call], zeroed by the caller
  float target[VINTERP_PASS];      // ct
  int target_key[VINTERP_PASS];    // ct + 0.f as an order-preserving int (vinterp_key): the wave-uniform pre-filter compares integers
  double target_log[VINTERP_PASS]; // LOG: log((double)ct), from the host
};
// float bits -> int with the same order as the floats (no NaN among the operands; -0 must have been turned into +0)
__host__ __device__ inline int vinterp_key(int bits)
{
  return bits ^ ((bits >> 31) & 0x7fffffff);
}
hipError_t launch_vinterp(const VinterpParams& prm, hipStream_t stream);

// ------------------------------------ level batches to per-cell target surfaces (mifc_vregrid.hip), EXTENSION
// One launch walks the `nlev` levels of `n` columns once, in index order (from = 0) or against it (from = 1), and serves
// the `nt` target planes tcoord + (t0 + t) * in_stride of one pass, nt <= tb <= VREGRID_MAX_TB; the host launches again
// for the targets beyond.  A lane keeps the targets of its own cells in LDS (nt * 256 * V floats of dynamic LDS, with nt = tb at most
// VREGRID_MAX_LDS bytes, which with the counting table stays within 64 KiB: tb * V <= 63).  Fields, outputs, `coord`, `ab`, `lev_bits`, the counters and vec4 as in
// VinterpParams; hybrid with no_ps: nothing is read per cell, ps counts as 0 (the `levels` form: ab = levels[nlev] then
// nlev zeros).  Bit t of tc_all: target plane t0 + t is flagged ALL_DEFINED.
const int VREGRID_MAX_FIELDS = 8, VREGRID_MAX_TARGETS = 256, VREGRID_MAX_TB = 32, VREGRID_TB = 24, VREGRID_MAX_LDS = 65536 - 1024;
struct VregridParams
{
  int hybrid;  // coordinate kind: 1 = alevel + blevel * ps, 0 = field
  int no_ps;   // hybrid only: 1 = the `levels` form
  int method;  // MIFC_VINTERP_LINEAR / MIFC_VINTERP_LOG
  int from;    // MIFC_VREGRID_FROM_FIRST / _FROM_LAST
  int outside; // MIFC_VREGRID_OUTSIDE_UNDEF / _OUTSIDE_CLAMP
  int nfields; // 1 .. VREGRID_MAX_FIELDS
  int n;       // columns of this launch
  int nlev;    // >= 2
  int tb;      // targets a pass has room for
  int nt;      // targets of this pass, 1 .. tb
  int t0;      // the call's target of the pass' target 0 (target planes, outputs, counters)
  int nt_call; // targets of the whole call: the distance between the counters of two fields
  int ps_all;  // hybrid: ps is flagged ALL_DEFINED
  int vec4;
  unsigned int tc_all;
  float undef;
  long in_stride, out_stride;
  const float* fields[VREGRID_MAX_FIELDS];
  float* out[VREGRID_MAX_FIELDS];
  const float* coord;
  const float* tcoord;
  const float* ab;
  const unsigned int* lev_bits;
  u64* n_undefined; // [nfields][nt_call], zeroed by the caller
};
hipError_t launch_vregrid(const VregridParams& prm, hipStream_t stream);

// ------------------------------------ layer integrals, means and extremes of level batches (mifc_vlayer.hip), EXTENSION
// One launch walks the `nlev` levels of `n` columns once for up to VLAYER_PASS fields and stores, per field, the products
// whose `slot` is not negative: product code p (MIFC_VLAYER_*, 1..6) goes to out[f] + slot[p - 1] * out_stride.  The host
// launches again for the fields beyond VLAYER_PASS (the coordinate and the bounds are read again, every field level once).
// VLAYER_PASS is the most a launch takes; carrying the sums AND the extremes it takes two (vlayer_pass_fields: the field
// counts at which every instance keeps two waves per SIMD without a spill).
// Inputs, `coord`, the level table (`ab`, `lev_bits`: bit f0 + f = field f of the launch is flagged ALL_DEFINED at level
// k, bit VINTERP_COORD_BIT = the coordinate is) and vec4 as in VinterpParams; lo_field / hi_field: per-cell bounds (n
// floats each, on the 16-byte grid for vec4) or null = the scalar.  `group`: what the walk carries -- VLAYER_SUMS
// (INTEGRAL, MEAN), VLAYER_EXTREMES (the other four) or both.
const int VLAYER_MAX_FIELDS = 8, VLAYER_PASS = 4, VLAYER_PRODUCTS = 6, VLAYER_SUMS = 1, VLAYER_EXTREMES = 2;
constexpr int vlayer_pass_fields(int group)
{
  return group == (VLAYER_SUMS | VLAYER_EXTREMES) ? 2 : VLAYER_PASS;
}
struct VlayerParams
{
  int hybrid;  // coordinate kind: 1 = alevel + blevel * ps, 0 = field
  int group;   // VLAYER_SUMS | VLAYER_EXTREMES
  int nfields; // of this launch, 1 .. VLAYER_PASS
  int f0;      // the call's field of the launch's field 0 (level bits, counters)
  int n;       // columns of this launch
  int nlev;    // >= 2
  int vec4;
  int ps_all;  // hybrid: fdef_ps == ALL_DEFINED
  float undef, lo, hi;
  long in_stride, out_stride;
  const float* fields[VLAYER_PASS];
  float* out[VLAYER_PASS];
  const float* coord;
  const float *lo_field, *hi_field;
  const float* ab;
  const unsigned int* lev_bits;
  u64* n_undefined; // [the call's nfields], zeroed by the caller
  int slot[VLAYER_PRODUCTS];
};
hipError_t launch_vlayer(const VlayerParams& prm, hipStream_t stream);

// ------------------------------------ vertical derivatives of level batches (mifc_vderiv.hip), EXTENSION
// One launch walks the `nlev` levels of `n` columns once for up to VDERIV_PASS fields and stores, per field and level, the
// derivative along the coordinate (what & VDERIV_DERIV: out[f] + k * out_stride) and, per pair of fields (2j, 2j + 1)
// and level, the magnitude of the two derivatives (what & VDERIV_MAG: mag[j] + k * out_stride; nfields is even then).
// The host launches again for the fields beyond vderiv_pass_fields(what): VDERIV_PASS, or two where both the derivatives
// and the magnitudes are written (the field counts at which every instance keeps two waves per SIMD without a spill,
// DESIGN.md 4.17).  Inputs, `coord`, `ab`, `lev_bits` (bit f0 + f = field f of
// the launch is flagged ALL_DEFINED at level k, bit VINTERP_COORD_BIT = the coordinate is) and vec4 as in VinterpParams.
// kind VDERIV_LEVELS: the coordinate is one constant per level, nothing is read per cell; the host has put what depends
// on it into the table: lev_bits bit VDERIV_LOWER_BIT / VDERIV_UPPER_BIT = c_k-1 / c_k+1 exists and differs from c_k,
// VDERIV_FOLD_BIT = the two-sided denominator is zero; lev_w[4 * k ..] = 1 / (c_k - c_k-1), 1 / (c_k+1 - c_k) and the
// two-sided weights (CENTRED: w, unused; WEIGHTED: w1, w2).
// Counters: n_undefined[(f0 + f) * nlev + k], n_undefined_mag[(f0 / 2 + j) * nlev + k], zeroed by the caller; a workgroup
// gathers its counts in (VDERIV_PASS + VDERIV_PASS / 2) * nlev words of dynamic LDS when lds_counts is set (the launcher
// sets it where that fits), otherwise a wave adds to the global counters itself.
const int VDERIV_MAX_FIELDS = 8, VDERIV_PASS = 4, VDERIV_DERIV = 1, VDERIV_MAG = 2;
const int VDERIV_HYBRID = 0, VDERIV_FIELD = 1, VDERIV_LEVELS = 2;
const int VDERIV_LOWER_BIT = 9, VDERIV_UPPER_BIT = 10, VDERIV_FOLD_BIT = 11;
constexpr int vderiv_pass_fields(int what)
{
  return what == (VDERIV_DERIV | VDERIV_MAG) ? 2 : VDERIV_PASS;
}
struct VderivParams
{
  int kind;    // VDERIV_HYBRID / VDERIV_FIELD / VDERIV_LEVELS
  int what;    // VDERIV_DERIV | VDERIV_MAG
  int method;  // MIFC_VDERIV_CENTRED / MIFC_VDERIV_WEIGHTED
  int nfields; // of this launch, 1 .. vderiv_pass_fields(what)
  int f0;      // the call's field of the launch's field 0 (level bits, counters): even
  int n;       // columns of this launch
  int nlev;    // >= 2
  int vec4;
  int ps_all;  // hybrid: fdef_ps == ALL_DEFINED
  int lds_counts; // set by launch_vderiv
  float undef;
  long in_stride, out_stride;
  const float* fields[VDERIV_PASS];
  float* out[VDERIV_PASS];
  float* mag[VDERIV_PASS / 2];
  const float* coord;
  const float* ab;
  const unsigned int* lev_bits;
  const double* lev_w;
  u64 *n_undefined, *n_undefined_mag;
};
hipError_t launch_vderiv(const VderivParams& prm, hipStream_t stream);

// ------------------------------------ running vertical integrals of level batches (mifc_vcumul.hip), EXTENSION
// One launch walks the `nlev` levels of `n` columns once, from level 0 upward in index (from = 0) or from level nlev - 1
// downward (from = 1), for up to VCUMUL_PASS fields and stores, per field and level, the trapezoid integral of the field
// over the coordinate (method 0) or over its logarithm (method 1) from the start of the walk to that level:
// out[f] + k * out_stride.  The host launches again for the fields beyond VCUMUL_PASS.  Inputs, `coord`, `ab`, `lev_bits`
// (bit f0 + f = field f of the launch is flagged ALL_DEFINED at level k, bit VINTERP_COORD_BIT = the coordinate is), vec4
// and kind (VDERIV_HYBRID / _FIELD / _LEVELS) as in VderivParams.  kind VDERIV_LEVELS: lev_g[k] = g(levels[k]), from the
// host.  start: n floats or null (start_all: flagged ALL_DEFINED); base[f]: n floats or null (bit f of base_all: flagged
// ALL_DEFINED); scale[f]: the factor of the sum.  Counters: n_undefined[(f0 + f) * nlev + k], zeroed by the caller; a
// workgroup gathers its counts in VCUMUL_PASS * nlev words of dynamic LDS when lds_counts is set (the launcher sets it
// where that fits), otherwise a wave adds to the global counters itself.
const int VCUMUL_MAX_FIELDS = 8, VCUMUL_PASS = 4;
struct VcumulParams
{
  int kind;    // VDERIV_HYBRID / VDERIV_FIELD / VDERIV_LEVELS
  int method;  // MIFC_VCUMUL_LINEAR / MIFC_VCUMUL_LOG
  int from;    // MIFC_VCUMUL_FROM_FIRST / MIFC_VCUMUL_FROM_LAST
  int nfields; // of this launch, 1 .. VCUMUL_PASS
  int f0;      // the call's field of the launch's field 0 (level bits, counters)
  int n;       // columns of this launch
  int nlev;    // >= 2
  int vec4;
  int ps_all;  // hybrid: fdef_ps == ALL_DEFINED
  int start_all, base_all;
  int lds_counts; // set by launch_vcumul
  float undef;
  long in_stride, out_stride;
  const float* fields[VCUMUL_PASS];
  float* out[VCUMUL_PASS];
  const float* base[VCUMUL_PASS];
  double scale[VCUMUL_PASS];
  const float* coord;
  const float* start;
  const float* ab;
  const unsigned int* lev_bits;
  const double* lev_g;
  u64* n_undefined;
};
hipError_t launch_vcumul(const VcumulParams& prm, hipStream_t stream);

// ------------------------------------ parcel ascent over level batches (mifc_vparcel.hip), EXTENSION
// One launch walks `n` columns once, from level 0 upward in index (from = 0) or from level nlev - 1 downward (from = 1),
// lifts the parcel of rules 1 to 9 of mifc_vparcel_* (include/mifc.h) from level to level and stores what is asked for:
// planes[0 .. 4] = cape, cin, plcl, plfc, pel (n floats each) and tparcel (a batch: level k at tparcel + k * out_stride);
// each may be null.  `t`, `coord`, `ab`, `lev_bits` (bit 0 = t is flagged ALL_DEFINED at level k, bit VINTERP_COORD_BIT =
// the pressure batch is), vec4 and kind (VDERIV_HYBRID / _FIELD / _LEVELS) as in VcumulParams.  kind VDERIV_LEVELS:
// lev_p[k] = levels[k] and lev_p[nlev + k] = pi_from_p(levels[k]), from the host.  src_level >= 0: the source is that
// level with the humidity q_src; -1: the planes t_src, q_src, p_src (n floats each; *_all: flagged ALL_DEFINED).
// Counters: n_undefined[0 .. 4] the planes, n_undefined[VPARCEL_PLANES + k] tparcel's level k, zeroed by the caller; a
// workgroup gathers its counts in VPARCEL_PLANES + nlev words of dynamic LDS when lds_counts is set (the launcher sets it
// where that fits), otherwise a wave adds to the global counters itself.
const int VPARCEL_PLANES = 5;
struct VparcelParams
{
  int kind; // VDERIV_HYBRID / VDERIV_FIELD / VDERIV_LEVELS
  int from; // MIFC_VPARCEL_FROM_FIRST / MIFC_VPARCEL_FROM_LAST
  int src_level;
  int n;    // columns of this launch
  int nlev; // >= 2
  int vec4;
  int ps_all; // hybrid: fdef_ps == ALL_DEFINED
  int tsrc_all, qsrc_all, psrc_all;
  int lds_counts; // set by launch_vparcel
  float undef;
  long in_stride, out_stride;
  const float* t;
  const float* coord;
  const float *t_src, *q_src, *p_src;
  float* planes[VPARCEL_PLANES];
  float* tparcel;
  const float* ab;
  const unsigned int* lev_bits;
  const float* lev_p;
  u64* n_undefined;
};
hipError_t launch_vparcel(const VparcelParams& prm, hipStream_t stream);

// ------------------------------------ Ertel potential vorticity of level batches (mifc_pvort.hip), EXTENSION
// One launch walks the `nlev` levels of a block of rows once.  The planes of the launch hold `rows` rows of nx cells: row
// 0 of them is row g0 of the call's grid of ny rows (device memory: g0 = 0, rows = ny; a staged band: the rows it owns
// and the neighbour rows they need).  The workgroup tiles cover the columns 0 .. nx - 1 and the rows c0 .. c1 (grid
// rows, all of them interior: 1 <= c0, c1 <= ny - 2, and c0 - 1 .. c1 + 1 lie in the planes); a computed row y is stored
// to y where own0 <= y < own1, to row 0 where y == 1 and own0 == 0, and to row ny - 1 where y == ny - 2 and own1 == ny.
// Level k of a batch lies k * stride floats behind its pointer (inputs and output alike).  kind, ab, lev_bits (bits 0, 1,
// 2: u, v, th flagged ALL_DEFINED at level k), lev_w and vec4 as in VderivParams; vec4 needs nx % 4 == 0 too.
// Counters: n_undefined[k], zeroed by the caller, one atomic per workgroup and level with something to count.
const int PVORT_LANES_X = 32, PVORT_TILE_ROWS = 8;
struct PvortParams
{
  int kind;   // VDERIV_HYBRID / VDERIV_FIELD / VDERIV_LEVELS
  int method; // MIFC_VDERIV_CENTRED / MIFC_VDERIV_WEIGHTED
  int nx, ny, nlev;
  int g0, rows;
  int c0, c1;
  int own0, own1;
  int vec4;
  int ps_all; // hybrid: fdef_ps == ALL_DEFINED
  float undef;
  double scale;
  long stride;
  const float *u, *v, *th;
  const float* coord; // ps [rows][nx], the coordinate batch, or null (levels)
  const float *xmapr, *ymapr, *fcoriolis; // [rows][nx]; fcoriolis may be null
  float* out;
  const float* ab;
  const unsigned int* lev_bits;
  const double* lev_w;
  u64* n_undefined;
};
hipError_t launch_pvort(const PvortParams& prm, hipStream_t stream);

// ------------------------------------ level batches sampled at arbitrary points (mifc_hinterp.hip), EXTENSION
// One launch samples `nlev` levels of up to hinterp_pass_fields(method) fields at `npos` points: a gather.  A lane owns
// one point, a workgroup 256 consecutive points and the levels [blockIdx.y * chunk, + chunk) of the launch; level k of
// field f lies at fields[f] + k * in_stride ([ny][nx]) and is written to out[f] + k * out_stride ([npos]).  The launch's
// level 0 is level lev0 of the call: lev_bits[lev0 + k] bit f0 + f = field f of the launch is flagged ALL_DEFINED there
// (read only by the tested instances), the counters are n_undefined[(f0 + f) * call_nlev + lev0 + k], zeroed by the
// caller.  Points whose position is unusable (rule 1 of include/mifc.h) are written as undef at every level and counted
// ONCE, into *n_unusable, by the workgroups of level chunk 0 of a launch with count_unusable set; the caller adds that
// number to every counter.  xpos, ypos: [npos].  Every access is a single dword: any alignment of any pointer.
const int HINTERP_MAX_FIELDS = 8, HINTERP_PASS = 4, HINTERP_PASS_BICUBIC = 2, HINTERP_UNROLL = 2;
const int HINTERP_NEAREST = 0, HINTERP_BILINEAR = 1, HINTERP_BICUBIC = 2;
constexpr int hinterp_pass_fields(int method)
{
  return method == HINTERP_BICUBIC ? HINTERP_PASS_BICUBIC : HINTERP_PASS;
}
struct HinterpParams
{
  int method;  // HINTERP_*
  int nfields; // of this launch, 1 .. hinterp_pass_fields(method)
  int f0;      // the call's field of the launch's field 0 (level bits, counters)
  int nx, ny;
  int npos;
  int nlev;      // levels of this launch
  int lev0;      // the call's level of the launch's level 0
  int call_nlev; // levels of the call: the row length of the counters
  int chunk;     // levels per workgroup: grid.y = ceil(nlev / chunk) (set by launch_hinterp from hinterp_plan)
  int tested;    // 0: every level of every field of the call is ALL_DEFINED, no value is tested
  int count_unusable;
  float undef;
  long in_stride, out_stride;
  const float* fields[HINTERP_PASS];
  float* out[HINTERP_PASS];
  const float *xpos, *ypos;
  const unsigned int* lev_bits;
  u64 *n_undefined, *n_unusable;
};
// The launch shape, the one rule for it: ceil(npos / 256) workgroups per level chunk, and the levels cut into as many
// chunks as it takes to give every CU eight workgroups where nlev allows -- but chunks of HINTERP_UNROLL levels at least,
// so that the loads of two levels are in flight.  Large npos: one chunk.  (MIFC_HINTERP_LEVEL_CHUNK overrides the chunk.)
struct HinterpPlan
{
  int blocks, chunk, level_chunks;
};
HinterpPlan hinterp_plan(int npos, int nlev);
hipError_t launch_hinterp(const HinterpParams& prm, hipStream_t stream);
// The ROTATE form (mifc_hinterp_vector_levels): the fields of the launch are pairs (u0, v0, u1, v1: nfields 2 or 4, 2 with
// the bicubic method, f0 even); every component is sampled as above and rounded to float, then the pair is rotated by rule R
// of include/mifc.h with the point's coefficients cosa[p], sina[p] (rot_all: fdef_rot == ALL_DEFINED).  A point whose
// coefficients are undefined counts as an unusable position.  A hole of either component is a hole of the pair: both
// outputs are undef there, and it is counted once, into n_undefined[(f0 / 2 + q) * call_nlev + lev0 + k].
struct HinterpRotateParams : HinterpParams
{
  const float *cosa, *sina;
  int rot_all;
};
hipError_t launch_hinterp_rotate(const HinterpRotateParams& prm, hipStream_t stream);

// ------------------------------------ level batches regridded by a weight table (mifc_hremap.hip), EXTENSION
// One launch applies a plan's table (the sliced-ELL layout of mifc_hremap_plan.h, on the device) to `nlev` levels of up to
// hremap_pass_fields(tested) fields: a sparse gather with a variable number of terms per output.  A lane owns one destination, a wave one
// slice of 64, a workgroup four slices and the levels [blockIdx.y * chunk, + chunk) of the launch, a register block of
// them (hremap_levels()) at a time with the sums in registers: a lane reads its (col, w) pair once per trip and uses it for those levels and every
// field of the launch.  Level k of field f lies at fields[f] + k * in_stride ([nsrc]) and is written to
// out[f] + k * out_stride ([ndst]).  The launch's level k is the call's level lev0 + k, its field f the call's f0 + f:
// lev_bits[lev0 + k] bit f0 + f says the input is ALL_DEFINED there, destinations with a row that are left undef are
// counted in n_undefined[(f0 + f) * call_nlev + lev0 + k]; empty rows are the plan's and are added by the caller.
// A tested launch takes HREMAP_PASS_TESTED fields: with Wdef, nbad and the lane masks of the tests three or four fields
// by four levels do not fit the scalar registers (the register table).  The register block is
// hremap_levels() levels: eight where eight levels of every field of the launch fit, else four.
const int HREMAP_MAX_FIELDS = 8, HREMAP_PASS = 4, HREMAP_PASS_TESTED = 2, HREMAP_LEVELS = 4, HREMAP_LEVELS_FEW = 8;
const int HREMAP_STRICT = 0, HREMAP_RENORM = 1;
constexpr int hremap_pass_fields(bool tested)
{
  return tested ? HREMAP_PASS_TESTED : HREMAP_PASS;
}
constexpr int hremap_levels(int nfields, bool tested) // nfields: of a launch
{
  return nfields * HREMAP_LEVELS_FEW <= (tested ? 8 : 16) ? HREMAP_LEVELS_FEW : HREMAP_LEVELS;
}
struct HremapParams
{
  int mode;    // HREMAP_*
  int nfields; // of this launch, 1 .. hremap_pass_fields(tested)
  int f0;
  int ndst, nslices;
  int nlev, lev0, call_nlev;
  int chunk;  // levels per workgroup: grid.y = ceil(nlev / chunk) (the caller's, from hremap_shape)
  int tested; // 0: every level of every field of the call is ALL_DEFINED, no value is tested
  float undef;
  double min_frac;
  long in_stride, out_stride;
  const float* fields[HREMAP_PASS];
  float* out[HREMAP_PASS];
  const u64* slice_off;   // [nslices]
  const int* slice_width; // [nslices]
  const int* len;         // [nslices * 64]
  const double* wall;     // [nslices * 64]
  const void* entries;    // 8-byte (col, w) pairs, slice_off[s] + r * 64 + lane
  const unsigned int* lev_bits;
  u64* n_undefined;
};
// The launch shape: ceil(nslices / 4) workgroups per level chunk, and the levels cut into chunks of ONE register block
// (hremap_levels(nfields, tested), nfields the fields per launch of the call), so that the tables are read once per chunk
// -- but shorter chunks, down to one level, where it takes that to give every CU eight workgroups, the target of
// hinterp_plan (few destinations: DESIGN.md 4.23, the measurement).  (MIFC_HREMAP_LEVEL_CHUNK overrides the chunk; a
// longer one walks several register blocks and reads the tables once per block.)
struct HremapShape
{
  int blocks, chunk, level_chunks;
};
HremapShape hremap_shape(int nslices, int nlev, int nfields, bool tested);
hipError_t launch_hremap(const HremapParams& prm, hipStream_t stream);

// ------------------------------------ vector pairs of level batches rotated on the grid (mifc_vrotate.hip), EXTENSION
// One launch rotates `nlev` levels of `npairs` pairs (u_q = fields[2q], v_q = fields[2q + 1]) at `n` cells by rule R of
// include/mifc.h: a streaming kernel.  A lane owns V consecutive cells (vec4: four through 16-byte accesses, as in
// VinterpParams; else one), a workgroup 256 lanes and the levels [blockIdx.y * chunk, + chunk); it reads its coefficients
// cosa, sina (n floats each) once.  Level k of a field lies at fields[f] + k * in_stride and is written to
// out[f] + k * out_stride.  lev_bits[k] bit f = field f is flagged ALL_DEFINED at level k (read only by the tested
// instances); rot_all: fdef_rot == ALL_DEFINED.  tested == 0: every flag of the call and fdef_rot are ALL_DEFINED.
// Counters: n_undefined[q * nlev + k], zeroed by the caller.
const int VROTATE_MAX_PAIRS = 4, VROTATE_UNROLL = 2, VROTATE_CHUNK = 4;
struct VrotateParams
{
  int npairs; // 1 .. VROTATE_MAX_PAIRS
  int n;      // cells of this launch
  int nlev;
  int chunk; // levels per workgroup: grid.y = ceil(nlev / chunk) (set by launch_vrotate from vrotate_plan)
  int tested;
  int rot_all;
  int vec4;
  float undef;
  long in_stride, out_stride;
  const float* fields[2 * VROTATE_MAX_PAIRS];
  float* out[2 * VROTATE_MAX_PAIRS];
  const float *cosa, *sina;
  const unsigned int* lev_bits;
  u64* n_undefined;
};
// The launch shape, the one rule for it: ceil(cells / (V * 256)) workgroups per level chunk, V = 4 or 1, and the levels cut
// into chunks of VROTATE_CHUNK, the last one shorter: the length measured fastest on small and on large fields alike
// (the coefficients are read once per chunk, 8 B per cell against the chunk's 64 * npairs).
// (MIFC_HINTERP_LEVEL_CHUNK overrides the chunk of this walk too.)
struct VrotatePlan
{
  int blocks, chunk, level_chunks;
};
VrotatePlan vrotate_plan(int cells, int nlev, int vec4 = 1);
hipError_t launch_vrotate(const VrotateParams& prm, hipStream_t stream);

// ------------------------------------ field expressions over level batches (mifc_fexpr.hip), EXTENSION
// One launch per problem evaluates the register program of mifc_fexpr_levels (include/mifc.h, rules 1-5) in every cell:
// grid.y is the level, a lane owns four consecutive cells (16-byte accesses) or one.  The program, its constants and the
// pointers travel in the kernel arguments; `code` is the program as mifc_fexpr_prog.h normalised it (op | dst << 8 |
// a << 16 | b << 24, then c), so the instruction words are scalar loads.  Input i < nfields is a batch (level k at
// in[i] + k * stride), the next nplanes are planes; out[o] receives register (out_regs >> 8 o) & 255.  The launch covers
// the cells cell0 .. cell0 + n - 1 of the levels lev0 .. lev0 + grid.y - 1; level_scalars is float[..][nlev_all] on the
// device, the counters n_undefined[o * nlev_all + k] are zeroed by the caller.
const int FEXPR_MAX_IN = 12, FEXPR_MAX_OUT = 4, FEXPR_MAX_CODE = 64, FEXPR_MAX_CONSTS = 16;
struct FexprParams
{
  int n, lev0, nlev_all;
  int ncode, nfields, nplanes, nout;
  unsigned int out_regs;
  float undef;
  long stride, cell0;
  const float* in[FEXPR_MAX_IN];
  float* out[FEXPR_MAX_OUT];
  const float* level_scalars;
  u64* n_undefined;
  unsigned int code[2 * FEXPR_MAX_CODE];
  float consts[FEXPR_MAX_CONSTS];
};
// The launch shape, the one rule for it: the vector form where every pointer of the call is on the 16-byte grid and a level
// has four cells or more -- ceil(n / 4 / 256) workgroups per level, and the n % 4 cells a level has left go to one
// 64-lane workgroup per level of the scalar kernel --, else the scalar form, ceil(n / 256) workgroups per level.
struct FexprShape
{
  int vector, grid, tail;
};
FexprShape fexpr_shape(const FexprParams& prm);
hipError_t launch_fexpr(const FexprParams& prm, int nlev, int tables, hipStream_t stream);

// ------------------------------------ horizontal statistics of level batches (mifc_hstats.hip), EXTENSION
// Two kernels (rules 1-7 of mifc_hstats_levels, include/mifc.h).  The segment kernel: a wave owns one (row, segment) of up
// to HSTATS_PASS fields -- the columns [4096 s, 4096 s + 4096) of one grid row, cut to the box -- and walks the levels
// blockIdx.y, + gridDim.y, ...; lane l owns the cells with (i / 4) mod 64 == l, 16 trips of four consecutive cells at most,
// loaded as one 16-byte access (vec4: every row of every plane on the 16-byte grid) or as four dwords.  The planes hold
// the rows [.., ..) of the grid that the caller staged: row r of the launch is row plane_row0 + r of the planes, grid row
// grid_row0 + r, row part_row0 + r of the box.  Level k of a field lies at fields[f] + k * stride, of minus[f] alike;
// weight is one plane.  lev_bits[k] bit f0 + f: field f of the launch is flagged ALL_DEFINED there, bit
// HSTATS_MINUS_BIT + f0 + f: its minus batch is; weight_all: fdef_weight == ALL_DEFINED; tested == 0: every flag of the
// call is ALL_DEFINED and no value is tested.  pivot: double[call fields][nlev] on the device.  The wave's eight numbers
// N, W, S1, S2, MIN, MAX, IMIN, IMAX of every field go to
//   part[((((f0 + f) * nlev + k) * box_rows + part_row0 + r) * segs + (s - seg0)) * 8 ..]   (the requested groups only).
// The combine kernel: a lane owns one (field, level, result row, slot) and walks its partials in the order of rule 4; it
// writes stats, and with mean[] given the float mean and, per row left undef, one count into n_undefined[f * nlev + k].
const int HSTATS_MAX_FIELDS = 8, HSTATS_PASS = 4, HSTATS_SEGMENT = 4096, HSTATS_TRIP = 256, HSTATS_MINUS_BIT = 8;
const int HSTATS_AREA = 0, HSTATS_ROWS = 1, HSTATS_MOMENTS = 1, HSTATS_EXTREMES = 2;
struct HstatsParams
{
  int nfields; // of this launch, 1 .. HSTATS_PASS
  int f0;      // the call's field of the launch's field 0
  int nx, nlev;
  int i0, i1;                                         // the box's columns
  int rows, plane_row0, grid_row0, part_row0, box_rows; // see above
  int seg0, segs;                                     // the first segment that the box touches, how many it touches
  int products;                                       // HSTATS_MOMENTS | HSTATS_EXTREMES
  int tested, weight_all, vec4;
  int level_blocks; // grid.y, the stride of a workgroup's walk over the levels (set by launch_hstats_segments from hstats_plan)
  float undef;
  long stride;
  const float* fields[HSTATS_PASS];
  const float* minus[HSTATS_PASS]; // all null: none
  const float* weight;             // null: none
  const unsigned int* lev_bits;
  const double* pivot;
  double* part;
};
struct HstatsPlan
{
  int blocks, level_blocks; // grid.x: four (row, segment) units per workgroup; grid.y
};
HstatsPlan hstats_plan(int rows, int segs, int nlev);
hipError_t launch_hstats_segments(const HstatsParams& prm, hipStream_t stream);
struct HstatsCombineParams
{
  int nfields, nlev, box_rows, segs; // of the call
  int mode, products;
  float undef;
  const double* part;
  const double* pivot;
  double* stats;                  // [nfields][nlev][nrows][8], nrows = 1 (AREA) or box_rows
  float* mean[HSTATS_MAX_FIELDS]; // [nlev][nrows] each, or all null
  u64* n_undefined;
};
hipError_t launch_hstats_combine(const HstatsCombineParams& prm, hipStream_t stream);

// ------------------------------------ area histograms and exact percentiles of level batches (mifc_hdist.hip), EXTENSION
// One walk over the included cells of (field, level) -- the rules of mifc_hdist_* (include/mifc.h), their arithmetic in
// mifc_hdist_rules.h -- serves three purposes (HdistParams::what): HDIST_COUNT bins every cell against the field's edges,
// HDIST_EXTENT finds n and the smallest and largest key, HDIST_DIGIT counts one digit of the selection.  A workgroup owns
// rows_per_group rows of the box of one field (grid.z) and walks the levels blockIdx.y, + gridDim.y, ...; its 256 lanes
// take four consecutive cells each, 1024 columns a trip, one 16-byte load where every row is on the 16-byte grid (vec4)
// or four dwords.  The planes hold the rows that the caller staged: row r of the launch is row plane_row0 + r of the
// planes and result row out_row0 + r of a ROWS histogram.  Level k of the launch is level lev0 + k of the call (the
// level table and the results are indexed by that, the units of the selection by k).
const int HDIST_COUNT = 0, HDIST_EXTENT = 1, HDIST_DIGIT = 2;
const int HDIST_GROUP_SLOTS = 4; // prefixes whose digit counters a workgroup keeps in LDS at a time
// the selection's state of one (field, level), device memory; written by the extent walk, the plan and the scan kernels
struct HdistUnit
{
  unsigned int n, kmin, kmax; // pass 0 (the init kernel: 0, 0xffffffff, 0)
  int passes, pass_shift[3], pass_width[3];
  int nranks;               // distinct ranks wanted, ascending
  unsigned int rank_left[32]; // the rank inside the prefix found so far
  unsigned int rank_key[32];  // the bits of the key found so far, the others zero
  int rank_slot[32];          // which of the prefixes below is this rank's
  int nslots;                 // distinct prefixes of the coming pass, ascending
  unsigned int slot_prefix[32];
  int qk[16], qk1[16]; // per percentile: which ranks are x[k] and x[k1]
  double qt[16];
};
struct HdistParams
{
  int what;
  int nx, nlev, lev0, unit_levels; // nlev: levels of this launch, lev0: the call's level of its level 0
  int nfields;
  int i0, i1;                          // the box's columns
  int rows, plane_row0, out_row0;      // the box's rows in the planes
  int rows_per_group;
  int tested, mask_all, vec4;
  int plain;        // the LDS counters without the wave's ballot (A/B: MIFC_HDIST_AGGREGATE=0)
  int level_blocks; // grid.y (set by launch_hdist_walk)
  float undef;
  long stride;
  const float* fields[8];
  const float* mask; // null: none
  const unsigned int* lev_bits;
  // HDIST_COUNT
  int nedges, out_rows, per_row;      // per_row: a result per row (ROWS), else one (AREA)
  const unsigned int* edge_keys;      // [call fields][nedges]
  int* hist;                          // [nfields][call nlev][out_rows][nedges + 2]
  int call_nlev;
  // HDIST_EXTENT, HDIST_DIGIT
  int pass, slot_stride;
  HdistUnit* units;         // [nfields][unit_levels]
  unsigned int* digit_hist; // [unit][slot_stride][HDIST_DIGIT_BINS]
};
struct HdistWalkShape
{
  int groups, level_blocks; // grid.x, grid.y
};
HdistWalkShape hdist_walk_shape(const HdistParams& prm);
hipError_t launch_hdist_walk(const HdistParams& prm, hipStream_t stream);
struct HdistSelectParams
{
  int nunits, unit_levels, lev0, call_nlev; // units = [nfields][unit_levels]
  int nq, method, pass, slot_stride;
  float undef;
  const float* percentiles; // [nq], device memory
  HdistUnit* units;
  const unsigned int* digit_hist;
  float* quant[8]; // [call nlev][nq] each
  u64* n_undefined; // [nfields][call nlev]
};
hipError_t launch_hdist_init(const HdistSelectParams& prm, hipStream_t stream);  // the units before the extent walk
hipError_t launch_hdist_plan(const HdistSelectParams& prm, hipStream_t stream);  // behind the extent walk: ranks, digits
hipError_t launch_hdist_scan(const HdistSelectParams& prm, hipStream_t stream);  // behind the digit walk of `pass`
hipError_t launch_hdist_final(const HdistSelectParams& prm, hipStream_t stream); // the percentiles, the counters

// ------------------------------------ trajectories through a series of wind level batches (mifc_htraj.hip), EXTENSION
// One launch carries the particles of `nlev` levels through ONE interval, from slice A to slice B, by the rules of
// mifc_htraj_levels (include/mifc.h), their arithmetic in mifc_htraj_rules.h: an iterated gather.  A lane owns particle p
// of one level for all nsub * (1 + niter) evaluations, a workgroup 256 consecutive particles and the levels
// [blockIdx.y * chunk, + chunk) of the launch, one after the other.  Every pointer is the caller's for level 0 of the
// launch and the slot the interval starts from: level k of a plane lies at its pointer + k * in_stride (the map planes
// are [ny][nx]); a slot is [levels][npos], level k at + k * npos: the one the interval starts from at x, y, t[f], the
// one it ends in slot_stride further.  The interval starts from the positions that the launch before left at x, y -- an
// undef there is a lost particle --, the launch with `first` set from xpos0, ypos0, shared by all levels, and it writes
// the slot it starts from too (the starts bit for bit, the trace of slice A).  bits[k] is the HTRAJ_*_BIT word
// of level k in this interval (read only by the tested instances).  The counters, zeroed by the caller, are rows of
// call_nlev, one per (g, slot): counts[(g * nslots + e) * call_nlev + k], e = 0 the starting slot and 1 the ending one;
// g = 0 the lost particles, g = 1 + f the trace holes of field f under live particles.  Every access is a single dword:
// any alignment.
struct HtrajParams
{
  int nx, ny, npos;
  int nlev;      // levels of this launch
  int call_nlev; // levels of the call: the row length of the counters
  int chunk;     // levels per workgroup: grid.y = ceil(nlev / chunk) (set by launch_htraj from htraj_level_chunk)
  int nslots;
  int nsub, niter, ntrace;
  int tested; // 0: every plane of the call is ALL_DEFINED, no value is tested
  int first;
  float undef;
  double tau; // times[B] - times[A]
  long in_stride, slot_stride;
  const float *uA, *uB, *vA, *vB, *xmapr, *ymapr;
  const float* trace[8]; // [0 .. 3] of slice A (read by the first launch only), [4 .. 7] of slice B
  const float *xpos0, *ypos0; // the start positions [npos] (read by the first launch only)
  float *x, *y, *t[4];
  const unsigned int* bits;
  u64* counts;
};
hipError_t launch_htraj(const HtrajParams& prm, hipStream_t stream);

// -------------------------------------------------------------------- stencils
enum StencilOp {
  ST_RELVORT = 0,    // :1843
  ST_ABSVORT = 1,    // :1875
  ST_DIVERGENCE = 2, // :1910
  ST_VORTDIV = 3,    // relvort + divergence fused, two outputs
  ST_GRAD_X = 4,     // gradient compute 1 :2013
  ST_GRAD_Y = 5,     // 2 :2025
  ST_GRAD_ABS = 6,   // 3 :2037
  ST_GRAD_LAP = 7,   // 4 :2051
  ST_GWIND_X = 8,    // plevelgwind_xcomp :638
  ST_GWIND_Y = 9,    // plevelgwind_ycomp :674
  ST_GVORT = 10,     // plevelgvort :708
  ST_IGWIND = 11,    // ilevelgwind :1511, two outputs
  // SURVEY.md 8f-1 (one-lane-per-cell kernel only, so far)
  ST_ADVECTION = 12, // advection :1942: f0 = f, f1 = u, f2 = v, scale = -3600*hours
  ST_JACOBIAN = 13,  // jacobian :2424: f0 = field1, f1 = field2
  ST_TFP = 14,       // second pass of thermalFrontParameter :2289-2302: f0 = tx, f1 = |grad tx|
  // last pass of plevelqvector :564-593: f0 = ug, f1 = vg, f2 = t, scale = tscale, scale2 = c
  ST_QVEC_X = 15, // compute 1, 2
  ST_QVEC_Y = 16  // compute 3, 4
};

struct StencilParams
{
  int op;
  int nx;
  int ny_global; // rows of the whole field
  int j0;        // global row of the first owned row (0 unless row-slab decomposed)
  int ny_local;  // owned rows in this buffer
  int nlev;      // fields in the batch (maps are shared)
  // f0/f1 point at OWNED row 0; for a slab the halo rows sit directly before and after
  const float* f0; // u | z | field | mpot
  const float* f1; // v (uv family only)
  const float* f2; // third input (advection: v)
  float scale;     // advection: -3600 * hours, rounded to float like the reference (:1963); Q-vector: tscale
  float scale2;    // Q-vector: c = -r / (p * 100) (:564)
  const float* scale_lev;  // Q-vector over a level batch: tscale / c per level of the launch (device), or null: scale / scale2
  const float* scale2_lev;
  const float* xmapr;
  const float* ymapr;
  const float* fcoriolis;
  float* out0;
  float* out1;   // second output (ST_VORTDIV diverg, ST_IGWIND vg); may be null
  // ST_VORTDIV over whole fields only, optional: the wind speed sqrt(u*u + v*v) of every cell as a third output and its
  // per-level undefined counts (vectorabs :1819, count domain nx*ny).  launch_vortdiv_rows leaves *handled false when the
  // launch is not one the split-role kernel takes; launch_stencil then returns hipErrorNotSupported
  float* out_ff;
  u64* n_undefined_ff;
  long in_level_stride;  // elements between consecutive levels of f0/f1
  long out_level_stride; // same for out0/out1
  const unsigned char* all_defined; // device u8[nlev] or null
  int every_level_all_defined;
  float undef;
  u64* n_undefined; // device u64[nlev]
  // row slabs of the wind operators only: restrict the launch to the owned output rows
  // [row_begin, row_end) (0, 0 = all).  Lets a caller compute the rows that need no halo while
  // the halo exchange is in flight.  A range must not separate a global edge row from the row
  // it is filled from (rows 0 / 1 and ny-2 / ny-1 of the whole field stay together).
  int row_begin, row_end;
  // Big levels (>= 2 048 workgroups per level), tested: the workgroups leave their counts in partials[level][unit] (plain
  // stores) and launch_count_partials_levels adds them up behind the kernel -- thousands of atomics on ONE counter address
  // (or on neighbouring counters: one cache line) take ~5 ns each, one after the other (4000 x 4000: 7 800 workgroups, 44 us
  // on top of a 65-us kernel; 8 levels on the level-walking kernel: 196 us on top of 390).  nullptr / 0: atomics.
  unsigned int* partials = nullptr;
  int partials_cap = 0;
};

hipError_t launch_stencil(const StencilParams& prm, hipStream_t stream);

// What a level-batch launch needs in place beforehand, as ONE small kernel instead of a host-to-device copy plus a fill
// (two stream operations on two engines: ~10 us of a 0.2 ms launch): the per-level input flags travel bit-packed in the
// kernel arguments and are expanded into d_flags (u8[nlev], null: none needed), d_counts[0 .. n_counts) is zeroed
// (null: nothing to zero).  Returns hipErrorInvalidValue beyond kPrepMaxLevels levels (the caller then copies and fills).
constexpr int kPrepMaxLevels = 2048;
// Which kernel form the calling thread's last stencil launch took ("wind_split", "scalar_oneshot", "flat4" ...): a
// diagnostic for tests and bug reports (mifc_last_stencil_form), nothing reads it on the data path.
void note_form(const char* form);
const char* last_form();
// The launch shape of the calling thread's last elementwise (mifc_ewise.hip), catalogue (mifc_pointwise.hip) or fused
// derived (mifc_derived.hip) launch: the same kind of diagnostic (mifc_last_pointwise_form).  The launchers store this
// small struct, host side, once per call; the text is only formatted when somebody asks for it.
struct PointwiseForm
{
  const char* family = ""; // "ewise" | "pointwise" | "derived"; "" before the first launch
  int op = 0;              // kernel instantiation: the EwiseOp / PwOp template argument (0 for derived)
  int vec = 0;             // 1: four cells per lane (16-byte accesses), 0: one cell per lane
  int grid = 0;            // workgroups of the main launch (derived: gx, workgroups per level)
  int nlev = 0;            // derived: levels (grid.y), else 0
  int partials = 0;        // 1: the counts went by the partials buffer and count_partials_kernel
  int tail = 0;            // cells of the 64-lane tail launch (n % 4 in the vector form, else 0)
  int n = 0;               // cells per field (derived: per level)
  const char* inst = "";   // derived: "ff+rh+theta", "ff+rh+theta+td", "rh+theta", "rh+theta+td", "ff" or "generic"
  int check = 0;           // derived: the CHECK instantiation (some level is not ALL_DEFINED)
  int pipe = 0;            // derived: the two-trip software pipeline
};
void note_pointwise_form(const PointwiseForm& form);
const char* last_pointwise_form();
hipError_t launch_prep_levels(const unsigned char* host_flags, int nlev, unsigned char* d_flags, u64* d_counts, int n_counts, hipStream_t stream);

// second-order Shapiro filter, FieldCalculations.cc:2076 (mifc_shapiro.hip)
struct ShapiroParams
{
  int nx, ny;
  int all_defined;       // input flag == ALL_DEFINED
  float undef;
  float* f1;             // in: the field, out: the smoothed field
  float* f2;             // scratch, nx*ny floats
  unsigned char* mask_x; // scratch, nx*ny bytes each (unused when all_defined)
  unsigned char* mask_y;
};
hipError_t launch_shapiro2(const ShapiroParams& prm, hipStream_t stream);
hipError_t launch_shapiro2_levels(const ShapiroParams& prm, int n_launch_levels, const int* levels, hipStream_t stream); // batches, see mifc_shapiro.hip
// The four sweeps in one launch, src -> dst (two different arrays); nx % 4 == 0, 16-byte aligned.
bool shapiro2_fused_supported(int nx, int ny, const float* src, const float* dst);
hipError_t launch_shapiro2_fused(int nx, int ny, int all_defined, float undef, const float* src, float* dst, hipStream_t stream);
// the same over n_launch_levels fields level_stride floats apart; entry k of the launch is level levels[k] (k if null)
hipError_t launch_shapiro2_fused_levels(int nx, int ny, int all_defined, float undef, const float* src, float* dst, int n_launch_levels,
                                        long level_stride, const int* levels, hipStream_t stream);

// Stencil-of-a-stencil operators in one launch (mifc_fused2.hip): the
// intermediate field(s) of thermalFrontParameter (:2266) and plevelqvector
// (:505) live in LDS row rings instead of going through HBM.
enum Fused2Op
{
  F2_TFP = 0,    // a = tx
  F2_QVEC_X = 1, // a = z, t = temperature; compute 1, 2
  F2_QVEC_Y = 2  // compute 3, 4
};
struct Fused2Params
{
  int op;
  int nx, ny;
  int check; // input flag != ALL_DEFINED
  const float* a;
  const float* t;
  const float* xmapr;
  const float* ymapr;
  const float* fcoriolis; // Q-vector only
  float* out;
  float undef;
  float scale;  // Q-vector: tscale
  float scale2; // Q-vector: c (:564)
  // [0] cells the first pass left undefined (TFP, tested input only)
  // [1] cells the last pass left undefined (what the returned flag is made from)
  // [2] TFP, tested input only: cells of the last pass that only the defined-test rejected
  u64* counts;
  // level batches (0 / null: one field): grid.y walks n_launch_levels entries; entry k is level
  // levels[k] (or k when levels is null) -- the levels of a batch are launched in two groups, the ones
  // whose input flag is ALL_DEFINED (no tests) and the others.  a, t, out are level_stride floats
  // apart, the map / Coriolis fields are shared, counts holds three counters per level, and the
  // Q-vector's scalars (they depend on the level's pressure) come from scale_lev / scale2_lev.
  int n_launch_levels;
  long level_stride;
  const int* levels;
  const float* scale_lev;
  const float* scale2_lev;
};
bool fused2_supported(const Fused2Params& prm);
hipError_t launch_fused2(const Fused2Params& prm, hipStream_t stream);

// ---------------------------------------------------------------- neighbourhood statistics
// neighbourProbFunctions :2862 / neighbourFunctions :2955 (mifc_neighbour.hip).  [nlev][ny][nx] batches, level_stride
// floats apart; the host has validated every scalar (range >= 1 except the range-0 threshold, step / 2 <= range,
// 0 <= ii < N), so every write lands inside the level.
struct NeighbourParams
{
  int nx, ny, nlev;
  long level_stride;
  int compute;  // 1 mean, 2 max, 3 min, 4 percentile, 5 count >, 6 count <; anything else writes +0 into its blocks
  int range, step;
  float limit;  // (float)(int)constant, as the reference compares float field against int limit
  float nf;     // (float)(2r+1)^2
  int ii;       // percentile index, 0 <= ii < N
  float undef;
  const float* in;
  float* out;
  u64* bits; // box counts: [nlev][ny][nwords] threshold bit rows (nwords = ceil(nx / 64))
};
__host__ __device__ inline int neighbour_words(int nx)
{
  return (nx + 63) / 64;
}
// compute 5/6 per cell as 0/1 (neighbourProbFunctions with range 0)
hipError_t launch_neighbour_threshold(const NeighbourParams& P, hipStream_t stream);
// compute 5/6 box count of every cell / (float)N, border undef: neighbourProbFunctions, and neighbourFunctions with step 1
hipError_t launch_neighbour_box(const NeighbourParams& P, hipStream_t stream);
// neighbourFunctions: undef border, then every centre's step x step block
hipError_t launch_neighbour_functions(const NeighbourParams& P, hipStream_t stream);

// ---------------------------------------------------------------- iterative vessel icing
// vesselIcingModStall (FieldCalculationsVesselIcing.cc:182) / vesselIcingMincog (:677) (mifc_icing.hip), one lane per
// cell over [nlev][ny][nx] batches.  The per-call constants come from mifc_icing::icing_consts (mifc_icing_cell.h).
const int ICING_KARG_LEVELS = 64; // level factors up to this many travel in the kernel arguments, more in lev_buf
struct IcingParams
{
  int nlev;
  int n;       // cells of one level
  long level_stride;
  const float* in[11];  // sal, wave, x_wind, y_wind, airtemp, rh, sst, p, Pw, aice, depth
  long in_stride[11];   // level_stride, or 0 for an input shared by every level
  float* out;
  const unsigned char* all_defined; // [nlev]: the level's input flag was ALL_DEFINED
  u64* n_undefined;                 // [nlev], zeroed by the caller
  float undef;
  const double* lev_buf;            // [number] level factors when number > ICING_KARG_LEVELS
  double lev[ICING_KARG_LEVELS];    // exp(-0.55 * (zmin + 0.5 k)) otherwise
  // mifc_icing::IcingConsts, flattened so that this header needs no other
  int model, alt, number, bisect_iter;
  float vs, cos_alpha, sin_beta, drag, Swdown;
  double vs_cos_d, cos_d;
  float br_sin2[2], br_cos[2], br_cos2[2];
};
hipError_t launch_vessel_icing(const IcingParams& P, hipStream_t stream);

#ifdef MIFC_MEASUREMENT_BUILD // libmifc_measure.so only
// diagnostic: (0.5*a*b*g0)/g through the shared-reciprocal quotient of mifc_device.h and through a plain f64 division
hipError_t launch_division_check(const float* a, const float* b, const float* g, float* shared, float* plain, size_t n, hipStream_t stream);

// diagnostic: two-in / two-out streaming copy (bandwidth yardstick)
hipError_t launch_stream2(int variant, int blocks, float* d0, float* d1, const float* s0, const float* s1, size_t n_floats, hipStream_t stream);
#endif

} // namespace mifc

#endif // MIFC_KERNELS_H
