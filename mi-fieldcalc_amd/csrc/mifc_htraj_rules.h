// mifc_htraj_rules.h -- the rules of mifc_htraj_levels (include/mifc.h), stated once for the kernel of mifc_htraj.hip, the
// host code of mifc_capi_htraj.hip and the tests: the inside test, the cell of a position and its safe offsets, the value
// of a plane at a double position (rules 2, 3 and 5 of mifc_hinterp_levels without the final rounding), the index velocity
// G, one interval of the Petterssen scheme, the trace sample, and the host side's argument check and interval / slot /
// chunk plan.  Plain C++ without any device header: tests/test_htraj_cpu.py compiles it with the host compiler
// (tests/htraj_rules_shim.cc, tests/host/htraj_rules_main.cc under the address and undefined-behaviour sanitizers).  The
// kernel file defines MIFC_HTRAJ_FN as the host-and-device qualifiers before it includes this text.  Every operation is a
// double operation rounded on its own: whoever compiles this text switches contraction off.
//
// Offsets are made safe instead of loads conditional (as in the hinterp kernel): a position that does not need column
// i0 + 1 (a == 0) or row j0 + 1 (b == 0) reads column i0 / row j0 again, a particle that is lost reads cell 0, and the
// integer cell is clamped into the grid AFTER the inside test, so that no offset outside [0, nx * ny) can be formed from
// any position, a NaN included.  The 24 loads of an evaluation are then straight-line code.
#ifndef MIFC_HTRAJ_RULES_H
#define MIFC_HTRAJ_RULES_H

#ifndef MIFC_HTRAJ_FN
#define MIFC_HTRAJ_FN inline
#endif

namespace mifc {

const int HTRAJ_MAX_NSUB = 64, HTRAJ_MAX_NITER = 8, HTRAJ_MAX_TRACE = 4, HTRAJ_MAX_EDGE = 1 << 24;
// the word of an (interval, level): which planes are flagged ALL_DEFINED there
const int HTRAJ_UA_BIT = 0, HTRAJ_UB_BIT = 1, HTRAJ_VA_BIT = 2, HTRAJ_VB_BIT = 3, HTRAJ_MAP_BIT = 4, HTRAJ_TRACE_B_BIT = 8, HTRAJ_TRACE_A_BIT = 12;

MIFC_HTRAJ_FN bool htraj_is_def(float x, float undef)
{
  return !(x != x) && x != undef;
}

// the inside test of rule 1, in double; a NaN fails it
MIFC_HTRAJ_FN bool htraj_inside(double xd, double yd, int nx, int ny)
{
  return xd >= 0.0 && xd <= (double)(nx - 1) && yd >= 0.0 && yd <= (double)(ny - 1);
}

// rule 1: a start (or the position of a slot) that a particle can leave from
MIFC_HTRAJ_FN bool htraj_usable(float x, float y, float undef, int nx, int ny)
{
  return htraj_is_def(x, undef) && htraj_is_def(y, undef) && htraj_inside((double)x, (double)y, nx, ny);
}

// rule 2: the cell of a position that passed the inside test (live), the fractions and the offsets of the four corners
// from the plane's base; a position that did not (live == false) is cell 0 with a == b == 0
struct HtrajCell
{
  int o00, o10, o01, o11;
  double a, b;
  bool a0, b0;
};
MIFC_HTRAJ_FN HtrajCell htraj_cell(double xd, double yd, int nx, int ny, bool live)
{
  const double xs = live ? xd : 0.0, ys = live ? yd : 0.0;
  int i0 = (int)xs, j0 = (int)ys;
  i0 = i0 < 0 ? 0 : (i0 > nx - 1 ? nx - 1 : i0); // (no change for a position inside: the offsets do not rest on the test)
  j0 = j0 < 0 ? 0 : (j0 > ny - 1 ? ny - 1 : j0);
  HtrajCell c;
  c.a = xs - (double)i0;
  c.b = ys - (double)j0;
  c.a0 = c.a == 0.0;
  c.b0 = c.b == 0.0;
  const int dx = (c.a0 || i0 >= nx - 1) ? 0 : 1, dy = (c.b0 || j0 >= ny - 1) ? 0 : nx;
  c.o00 = j0 * nx + i0;
  c.o10 = c.o00 + dx;
  c.o01 = c.o00 + dy;
  c.o11 = c.o00 + dy + dx;
  return c;
}

struct HtrajCorners
{
  float v00, v10, v01, v11;
};
MIFC_HTRAJ_FN HtrajCorners htraj_load(const float* plane, const HtrajCell& c)
{
  HtrajCorners v;
  v.v00 = plane[c.o00];
  v.v10 = plane[c.o10];
  v.v01 = plane[c.o01];
  v.v11 = plane[c.o11];
  return v;
}

// rule 5 of mifc_hinterp_levels without the final rounding; ok: every needed corner passes is_defined -- which counts
// only where the plane is not flagged ALL_DEFINED (rule 3): the caller knows the flag
template <bool TESTED>
MIFC_HTRAJ_FN double htraj_value(const HtrajCell& c, const HtrajCorners& v, float undef, bool& ok)
{
  const bool d00 = !TESTED || htraj_is_def(v.v00, undef), d10 = !TESTED || htraj_is_def(v.v10, undef);
  const bool d01 = !TESTED || htraj_is_def(v.v01, undef), d11 = !TESTED || htraj_is_def(v.v11, undef);
  ok = d00 & (c.a0 | d10) & (c.b0 | d01) & (c.a0 | c.b0 | d11);
  const double x00 = (double)v.v00, x10 = (double)v.v10, x01 = (double)v.v01, x11 = (double)v.v11;
  const double e0 = x10 - x00, e1 = x11 - x01;
  const double g0 = c.a * e0, g1 = c.a * e1;
  const double s0 = x00 + g0, s1 = x01 + g1;
  const double r0 = c.a0 ? x00 : s0, r1 = c.a0 ? x01 : s1;
  const double er = r1 - r0;
  const double gr = c.b * er;
  const double sr = r0 + gr;
  return c.b0 ? r0 : sr;
}

// the planes of one level in one interval, slice A to slice B; all: the HTRAJ_*_BIT word of the level
struct HtrajWind
{
  const float *uA, *uB, *vA, *vB, *mx, *my;
  unsigned int all;
  int nx, ny;
  float undef;
};

// rule 3: the index velocity at (xd, yd) and the weight w of slice B; false: the particle is lost (it was already, it is
// outside, or a needed corner of one of the six planes is undefined)
template <bool TESTED>
MIFC_HTRAJ_FN bool htraj_velocity(const HtrajWind& W, double xd, double yd, double w, bool live, double& gx, double& gy)
{
  live = live && htraj_inside(xd, yd, W.nx, W.ny);
  const HtrajCell c = htraj_cell(xd, yd, W.nx, W.ny, live);
  const HtrajCorners cuA = htraj_load(W.uA, c), cuB = htraj_load(W.uB, c), cvA = htraj_load(W.vA, c), cvB = htraj_load(W.vB, c);
  const HtrajCorners cmx = htraj_load(W.mx, c), cmy = htraj_load(W.my, c);
  bool ok_uA, ok_uB, ok_vA, ok_vB, ok_mx, ok_my;
  const double uA = htraj_value<TESTED>(c, cuA, W.undef, ok_uA), uB = htraj_value<TESTED>(c, cuB, W.undef, ok_uB);
  const double vA = htraj_value<TESTED>(c, cvA, W.undef, ok_vA), vB = htraj_value<TESTED>(c, cvB, W.undef, ok_vB);
  const double mx = htraj_value<TESTED>(c, cmx, W.undef, ok_mx), my = htraj_value<TESTED>(c, cmy, W.undef, ok_my);
  // rule 3: the planes with a hole under this position as a word like W.all; a hole counts where the plane's bit is not set
  const unsigned int holes = (ok_uA ? 0u : 1u << HTRAJ_UA_BIT) | (ok_uB ? 0u : 1u << HTRAJ_UB_BIT) | (ok_vA ? 0u : 1u << HTRAJ_VA_BIT) |
                             (ok_vB ? 0u : 1u << HTRAJ_VB_BIT) | ((ok_mx && ok_my) ? 0u : 1u << HTRAJ_MAP_BIT);
  const double du = uB - uA, dv = vB - vA;
  const double pu = w * du, pv = w * dv;
  const double su = uA + pu, sv = vA + pv;
  const double uu = w == 0.0 ? uA : (w == 1.0 ? uB : su), vv = w == 0.0 ? vA : (w == 1.0 ? vB : sv);
  gx = uu * mx;
  gy = vv * my;
  return live && (holes & ~W.all) == 0u;
}

// rule 4: the nsub substeps of one interval, tau = times[B] - times[A]; (x, y) goes in at slice A and comes out at slice
// B; false: the particle is lost (then x and y mean nothing)
template <bool TESTED>
MIFC_HTRAJ_FN bool htraj_interval(const HtrajWind& W, double tau, int nsub, int niter, double& x, double& y, bool live)
{
  const double dn = (double)nsub;
  const double h = tau / dn;
  const double hh = 0.5 * h;
  for (int s = 0; s < nsub; ++s) {
    const double w0 = (double)s / dn, w1 = (double)(s + 1) / dn;
    double g0x, g0y;
    live = htraj_velocity<TESTED>(W, x, y, w0, live, g0x, g0y);
    const double px = h * g0x, py = h * g0y;
    double xs = x + px, ys = y + py;
    for (int it = 0; it < niter; ++it) {
      double g1x, g1y;
      live = htraj_velocity<TESTED>(W, xs, ys, w1, live, g1x, g1y);
      const double sx = g0x + g1x, sy = g0y + g1y;
      const double cx = hh * sx, cy = hh * sy;
      xs = x + cx;
      ys = y + cy;
    }
    x = xs;
    y = ys;
  }
  return live && htraj_inside(x, y, W.nx, W.ny);
}

// rule 7: rules 2-5 of mifc_hinterp_levels, BILINEAR, at the float position of a slot; hole: the particle is alive and a
// needed corner is undefined.  A lost particle gives undef and no hole.
template <bool TESTED>
MIFC_HTRAJ_FN float htraj_trace(const float* plane, float x, float y, bool live, bool all, float undef, int nx, int ny, bool& hole)
{
  const HtrajCell c = htraj_cell((double)x, (double)y, nx, ny, live);
  bool ok;
  const float r = (float)htraj_value<TESTED>(c, htraj_load(plane, c), undef, ok);
  ok = ok || all;
  hole = live && !ok;
  return (live && ok) ? r : undef;
}

// ---------------------------------------------------------------------------------------------------- the host side
// The refusals that read only the scalars and `times`, in the order of include/mifc.h: null where the call is fine, else
// the reason.
MIFC_HTRAJ_FN const char* htraj_check(int nx, int ny, int nlev, int nt, int npos, int j_start, int j_end, int nsub, int niter, int ntrace,
                                      const double* times, float undef)
{
  if (nt < 2)
    return "nt < 2";
  if (nlev < 1)
    return "nlev < 1";
  if (npos < 1)
    return "npos < 1";
  if (nx < 1 || ny < 1)
    return "nx < 1 or ny < 1";
  if (nx > HTRAJ_MAX_EDGE || ny > HTRAJ_MAX_EDGE)
    return "nx or ny above 2^24";
  if ((long long)nx * (long long)ny > 0x7fffffffLL)
    return "more than 2^31 - 1 cells per level";
  if (j_start < 0 || j_start > nt - 1 || j_end < 0 || j_end > nt - 1)
    return "j_start or j_end outside 0..nt-1";
  if (j_start == j_end)
    return "j_start == j_end";
  if (nsub < 1 || nsub > HTRAJ_MAX_NSUB)
    return "nsub outside 1..64";
  if (niter < 0 || niter > HTRAJ_MAX_NITER)
    return "niter outside 0..8";
  if (ntrace < 0 || ntrace > HTRAJ_MAX_TRACE)
    return "ntrace outside 0..4";
  if (!times)
    return "a null pointer (times)";
  const int lo = j_start < j_end ? j_start : j_end, hi = j_start < j_end ? j_end : j_start;
  for (int j = lo; j <= hi; ++j)
    if (!(times[j] - times[j] == 0.0))
      return "a time of the used slices is not finite";
  for (int j = lo; j < hi; ++j)
    if (!(times[j] < times[j + 1]))
      return "the times of the used slices are not strictly increasing";
  const int edge = nx > ny ? nx : ny;
  if (undef >= 0.0f && (double)undef <= (double)(edge - 1))
    return "undef is a position inside the grid";
  return nullptr;
}

// slot n belongs to slice j_start + n * dir; interval n runs from slot n to slot n + 1
struct HtrajPlan
{
  int dir, nslots, intervals;
};
MIFC_HTRAJ_FN HtrajPlan htraj_plan(int j_start, int j_end)
{
  HtrajPlan p;
  p.dir = j_end > j_start ? 1 : -1;
  p.intervals = (j_end - j_start) * p.dir;
  p.nslots = p.intervals + 1;
  return p;
}
MIFC_HTRAJ_FN int htraj_slice(const HtrajPlan& p, int j_start, int slot)
{
  return j_start + slot * p.dir;
}

// Host memory: the levels of a staged chunk -- two slice buffers of u, v and the trace fields, and every slot of x, y and
// the traces -- within `budget` bytes, but never less than one level.
MIFC_HTRAJ_FN unsigned long long htraj_bytes_per_level(unsigned long long cells, unsigned long long npos, int nslots, int ntrace)
{
  const unsigned long long planes = 2ull + (unsigned long long)ntrace;
  return (2ull * planes * cells + planes * (unsigned long long)nslots * npos) * sizeof(float);
}
MIFC_HTRAJ_FN int htraj_levels_per_chunk(unsigned long long budget, unsigned long long per_level, int nlev)
{
  const unsigned long long fit = budget / per_level;
  return fit < 1 ? 1 : (fit > (unsigned long long)nlev ? nlev : (int)fit);
}

// The levels a workgroup walks (grid.y = ceil(nlev / chunk)): one, so that every (level, 256 particles) is a workgroup of
// its own and the device has as many dependent chains in flight as the call has -- unless `forced` > 0 says otherwise or
// grid.y would pass its limit.
MIFC_HTRAJ_FN int htraj_level_chunk(int nlev, int forced)
{
  const int max_grid_y = 65535, least = (nlev + max_grid_y - 1) / max_grid_y;
  int chunk = forced > 0 ? (forced < nlev ? forced : nlev) : 1;
  return chunk > least ? chunk : least;
}

} // namespace mifc

#endif // MIFC_HTRAJ_RULES_H
