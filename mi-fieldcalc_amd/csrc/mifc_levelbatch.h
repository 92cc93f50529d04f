// mifc_levelbatch.h -- the host driver of the entries that walk level batches column by column (mifc_capi_vinterp.hip,
// mifc_capi_vlayer.hip, mifc_capi_vderiv.hip, mifc_capi_vcumul.hip, mifc_capi_vparcel.hip; the head, the refusals and the level table also serve
// mifc_capi_hinterp.hip, which samples the levels instead of walking them, and mifc_capi_hremap.hip, which regrids them by a weight table; mifc_capi_pvort.hip differences along the rows too, its bands carry neighbour rows): the head of such a call and the refusals
// that read only it, the overlap rule, the device table of the per-level scalars (for the `levels` form of the vertical
// derivative its weights too), and where the planes of the call are on the device -- the caller's own for device memory, a
// band of rows at a time for host memory (columns are independent, so a band of every level is a complete problem; where
// rows are not, a band is staged with the neighbour rows it needs).  Implemented in mifc_levelbatch.hip.
#ifndef MIFC_LEVELBATCH_H
#define MIFC_LEVELBATCH_H

#include "mifc_ctx.h"

#include <algorithm>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

namespace mifc_host {

// the coordinate: alevel + blevel * ps, a batch like the fields, or one HOST number per level (nothing per cell)
enum { COORD_HYBRID = 0, COORD_FIELD = 1, COORD_LEVELS = 2 };

struct LevelBatchCall
{
  const char* name;
  int kind; // COORD_*
  int nx, ny, nlev;
  const float* const* fields;
  const int* fdefined_in;
  int nfields;
  const float* coord; // ps [ny][nx], the coordinate batch [nlev][ny][nx] or levels[nlev]
  int fdef_ps;
  const int* fdef_coord;
  const float *alevel, *blevel;
  float undef;
  int memkind;

  bool hybrid() const { return kind == COORD_HYBRID; }
  size_t coord_planes() const { return kind == COORD_HYBRID ? 1 : (kind == COORD_FIELD ? (size_t)nlev : 0); }
  size_t cells() const { return (size_t)nx * (size_t)ny; }
};

int refuse(mifc_ctx* c, const LevelBatchCall& a, const std::string& why);

// The shared refusals, 0 with the context's error set.  An entry puts its own between them, in this order:
// an open capture, nlev, nfields | negative nx or ny, memkind | fields[f], fres[f] (where fres is given) | the hybrid
// levels, the cell limit
int check_counts(mifc_ctx* c, const LevelBatchCall& a, int max_fields);
int check_grid(mifc_ctx* c, const LevelBatchCall& a);
int check_field_pointers(mifc_ctx* c, const LevelBatchCall& a, float* const* fres);
int check_levels(mifc_ctx* c, const LevelBatchCall& a);

// In-place is not offered: every output (name[i] = p[i], i < n, of `bytes` each) against the coordinate, `more_inputs` (the
// ones that are not null), every field and every other output, by byte range; "<out> overlaps <in>".
struct Outputs
{
  float* const* p;
  int n;
  size_t bytes;
  const char* name;
};
struct Input
{
  const void* p;
  size_t bytes;
  const char* name;
};
int check_overlaps(mifc_ctx* c, const LevelBatchCall& a, std::initializer_list<Outputs> outs, std::initializer_list<Input> more_inputs = {});

// One device block, uploaded once: n_counts counters (zero) | alevel, blevel | a word per level (bit f: field f is
// flagged ALL_DEFINED there, VINTERP_COORD_BIT: the coordinate is) | `tail_bytes` of the caller's.
class LevelTable
{
public:
  int build(mifc_ctx* c, const LevelBatchCall& a, size_t n_counts, size_t tail_bytes = 0);
  unsigned int* bits() { return reinterpret_cast<unsigned int*>(host_.data() + o_bits_); } // the caller may add its own, and fill
  void* tail() { return host_.data() + o_tail_; }                                           // the tail, before upload()
  int upload(mifc_ctx* c, Staging& st);
  u64* n_undefined() const { return reinterpret_cast<u64*>(dev_); }
  const float* ab() const { return reinterpret_cast<const float*>(dev_ + o_ab_); }
  const unsigned int* lev_bits() const { return reinterpret_cast<const unsigned int*>(dev_ + o_bits_); }
  const void* dev_tail() const { return dev_ + o_tail_; }
  int read_counts(mifc_ctx* c); // behind the last launch, in front of Staging::finish()
  int classify(size_t counter, size_t cells) const { return mifc_classify(counts_[counter], (u64)cells); }
  u64 count(size_t counter) const { return counts_[counter]; } // (an entry that adds a common counter to the others classifies itself)

private:
  std::vector<unsigned char> host_;
  std::vector<u64> counts_;
  size_t o_ab_ = 0, o_bits_ = 0, o_tail_ = 0;
  unsigned char* dev_ = nullptr;
};

// Rules 3 to 5 of mifc_vderiv_* (include/mifc.h) for a coordinate that is the same in every cell of a level (COORD_LEVELS,
// a.coord = levels[nlev], none of them NaN: the caller has refused that): the sides that exist and the weights, divided
// once per level in double, every operation rounded on its own (mifc_levelbatch.hip is compiled without contraction like
// the kernels).  Into the tail of `tab`, built with 4 * nlev doubles of it: 1 / (c_k - c_k-1), 1 / (c_k+1 - c_k) and the
// two-sided weights of `method` per level; VDERIV_LOWER_BIT / _UPPER_BIT / _FOLD_BIT are added to the level's word.
void vderiv_level_weights(LevelTable& tab, const LevelBatchCall& a, int method);

// The rows of a staged band such that `planes` planes of them, each padded to a multiple of 64 floats (every plane on the
// 16-byte grid), fit `budget` bytes -- but never less than one row.
inline size_t plan_band(size_t budget, size_t planes, size_t nx, size_t ny)
{
  size_t rows = std::max<size_t>(1, std::min<size_t>(ny, budget / (planes * nx * sizeof(float))));
  while (rows > 1 && planes * align_up(rows * nx, 64) * sizeof(float) > budget)
    rows -= 1;
  return rows;
}

// The planes of a call, in groups that lie [planes][ny][nx] at `host`: uploaded (in) or downloaded (out) per band in the
// order they were added.  A group without planes or without a pointer takes no room and stays null.
struct PlaneGroup
{
  float* host;
  float* dev;
  size_t planes;
  bool out;
};
// The rows of one problem of BandPlan::run(): the planes on the device hold the grid rows first .. first + staged - 1, the
// rows own0 .. own1 - 1 of them are this problem's to write (device memory: all ny rows, staged and owned).
struct BandRows
{
  int nx, first, staged, own0, own1;
  int n() const { return staged * nx; } // the cells of a plane
};
class BandPlan
{
public:
  PlaneGroup* in(const float* host, size_t planes) { return add(const_cast<float*>(host), planes, false); }
  PlaneGroup* out(float* host, size_t planes) { return add(host, planes, true); }
  // device memory: dev = host, the stride a level, vec4 where every pointer and the level size allow 16-byte accesses;
  // host memory: the groups one behind the other in one block of `budget` bytes at most, the stride S, vec4 (a lane's four
  // floats may straddle the end of the band: they stay inside the padded plane).
  // halo_rows = 0: columns are independent, a band of rows is a complete problem.  halo_rows = h > 0 (ny >= 2 h + 1): a
  // row needs its h neighbours on each side, the rows 0 .. h - 1 and ny - h .. ny - 1 are written from the rows next to
  // them; a band is staged with the rows its own rows need -- at least 2 h + 1 rows whatever the budget says, the stride
  // is their padded size -- and owns what is left of them, or everything where all ny rows fit.
  int place(mifc_ctx* c, Staging& st, const LevelBatchCall& a, size_t budget, int halo_rows = 0);
  long stride = 0;
  int vec4 = 0;
  // launch(rows): the launches of one problem (BandRows), 0 where one failed.  Host memory: per band the in-groups up over
  // the staged rows, launch, the owned rows of the out-groups down.
  template <class Launch>
  int run(mifc_ctx* c, const LevelBatchCall& a, Launch launch)
  {
    const int nx = a.nx, ny = a.ny, h = halo_;
    if (a.memkind != MIFC_MEM_HOST)
      return launch(BandRows{nx, 0, ny, 0, ny});
    const size_t pitch = a.cells() * sizeof(float), dpitch = (size_t)stride * sizeof(float);
    for (int r0 = 0; r0 < ny; r0 += own_) {
      // the band's own rows, clamped to the rows that have all their neighbours, and the h rows around those
      const int r1 = std::min(r0 + own_, ny), lo = std::min(std::max(r0, h), ny - 1 - h), hi = std::min(std::max(r1 - 1, h), ny - 1 - h);
      const BandRows b = {nx, lo - h, hi - lo + 1 + 2 * h, r0, r1};
      const size_t off = (size_t)b.first * (size_t)nx, mine = (size_t)r0 * (size_t)nx;
      for (int i = 0; i < n_; ++i)
        if (g_[i].dev && !g_[i].out)
          MIFC_HIP(c, hipMemcpy2DAsync(g_[i].dev, dpitch, g_[i].host + off, pitch, (size_t)b.n() * sizeof(float), g_[i].planes, hipMemcpyHostToDevice, c->stream));
      if (!launch(b))
        return 0;
      for (int i = 0; i < n_; ++i)
        if (g_[i].dev && g_[i].out)
          MIFC_HIP(c, hipMemcpy2DAsync(g_[i].host + mine, pitch, g_[i].dev + (mine - off), dpitch, (size_t)(r1 - r0) * (size_t)nx * sizeof(float), g_[i].planes,
                                       hipMemcpyDeviceToHost, c->stream));
    }
    return 1;
  }

private:
  PlaneGroup* add(float* host, size_t planes, bool out)
  {
    g_[n_] = {planes ? host : nullptr, nullptr, host ? planes : 0, out};
    return &g_[n_++];
  }
  static const int MAX_GROUPS = 28; // 8 fields, the coordinate, two bounds, 8 + 4 outputs; or a start, 8 bases and 8 outputs
  PlaneGroup g_[MAX_GROUPS];
  int n_ = 0;
  int own_ = 0, halo_ = 0; // host memory: the rows a band owns, the neighbour rows on each side
};

// What VinterpParams, VlayerParams, VderivParams and VcumulParams have alike, everything else zero.
template <class Params>
void fill_params(Params& P, const LevelBatchCall& a, const LevelTable& tab, const BandPlan& plan, const PlaneGroup* coord)
{
  std::memset(&P, 0, sizeof P);
  P.nlev = a.nlev;
  P.ps_all = a.fdef_ps == MIFC_ALL_DEFINED ? 1 : 0;
  P.undef = a.undef;
  P.n_undefined = tab.n_undefined();
  P.ab = tab.ab();
  P.lev_bits = tab.lev_bits();
  P.coord = coord->dev;
  P.in_stride = P.out_stride = plan.stride;
  P.vec4 = plan.vec4;
}

} // namespace mifc_host

#endif // MIFC_LEVELBATCH_H
