// mifc_memberbatch.h -- the host driver of the entries that take `nmem` members of `nlev` levels and write a few outputs
// of the same shape, in host or device memory (mifc_capi_quantile.hip, mifc_capi_ensemble.hip).  What each piece does
// is in DESIGN.md 4.19.  Implemented in mifc_memberbatch.hip.
#ifndef MIFC_MEMBERBATCH_H
#define MIFC_MEMBERBATCH_H

#include "mifc_ctx.h"

#include <algorithm>
#include <initializer_list>
#include <string>
#include <vector>

namespace mifc_host {

struct MemberBatchCall
{
  const char* name;
  int nx, ny, nlev, nmem;
  const float* const* fields;
  const int* fdefined_in; // [nmem][nlev], or null: SOME_DEFINED
  float undef;
  int memkind;
  size_t cells() const { return (size_t)nx * (size_t)ny; }
  size_t bytes() const { return cells() * (size_t)nlev * sizeof(float); } // of one member or output
};

int refuse(mifc_ctx* c, const MemberBatchCall& a, const std::string& why);

// Nothing may be thrown across the C ABI: host allocations run in here, before the call enqueues its first operation.
template <class Allocate>
int host_memory(mifc_ctx* c, Allocate allocate)
{
  try {
    allocate();
    return 1;
  } catch (...) {
    c->err = "out of host memory";
    return 0;
  }
}

// The shared refusals, 0 with the context's error set; an entry puts its own in front, between and behind them:
// nlev, a negative size, memkind, a null pointer (`other_null`: one of the entry's own, `names` it and `fields`), fields[j]
int check_head(mifc_ctx* c, const MemberBatchCall& a, bool other_null, const char* names);
// the cell limit, two outputs (of bytes() each) that share a byte
int check_outputs(mifc_ctx* c, const MemberBatchCall& a, float* const* out, int nout);

// Bounded staging of a host-memory ensemble batch (mifc_ensembleQuantiles, mifc_ensemble_levels): `per_cell` bytes of
// device memory per staged cell, `budget` bytes in all.  Whole levels while they fit, else a range of cells of one level.
inline void plan_level_chunks(size_t budget, size_t cells, size_t per_cell, size_t nlev, size_t* lev_chunk, size_t* cell_chunk)
{
  *lev_chunk = nlev;
  *cell_chunk = cells;
  if (cells * per_cell <= budget) {
    *lev_chunk = nlev < budget / (cells * per_cell) ? nlev : budget / (cells * per_cell);
  } else {
    *lev_chunk = 1;
    *cell_chunk = budget / per_cell > 1 ? budget / per_cell : 1;
  }
}

// One call's tables and placement.  build() allocates every host buffer; place() says where the arrays of a launch are.
struct MemberBatch
{
  int words = 1;                 // per level: bit j % 64 of word j / 64 = member j is flagged ALL_DEFINED / NONE_DEFINED
  std::vector<u64> all, none;    // (`none`, and `ndef`, the members of a level that are not, only with_none)
  std::vector<int> ndef;
  std::vector<const float*> mem; // on the device: the caller's, or the staged chunk's
  std::vector<float*> out;       // (an entry may point one elsewhere before run())
  size_t lev_chunk = 0, cell_chunk = 0;
  bool aligned = true;           // every mem[] and out[] is on the 16-byte grid
  int launches = 0;              // of run(): one per staged chunk
  int build(mifc_ctx* c, const MemberBatchCall& a, bool with_none, float* const* out_host, int nout, size_t n_counts);
  // device memory: one chunk of everything; host memory: two scratch blocks of `budget` bytes at most, the arrays a
  // multiple of 64 floats apart; cells_by_4: a range of cells that is not a level's last is a multiple of 4
  int place(mifc_ctx* c, Staging& st, const MemberBatchCall& a, size_t budget, bool cells_by_4);
  // The first n_counts counters of the context (of ensure_levels(count_levels)) to zero and into P.n_undefined; then per
  // chunk P.nlev, P.lev0, P.n and P.stride, the members up (host memory), launch() -- 0 where it failed --, the outputs down.
  template <class Params, class Launch>
  int run(mifc_ctx* c, const MemberBatchCall& a, Params& P, size_t count_levels, Launch launch)
  {
    if (!ensure_levels(c, count_levels))
      return 0;
    P.n_undefined = c->d_counts;
    MIFC_HIP(c, hipMemsetAsync(c->d_counts, 0, counts_.size() * sizeof(u64), c->stream));
    const bool host = a.memkind == MIFC_MEM_HOST;
    const size_t nlev = (size_t)a.nlev, cells = a.cells();
    for (size_t l0 = 0; l0 < nlev; l0 += lev_chunk)
      for (size_t c0 = 0; c0 < cells; c0 += cell_chunk) {
        const size_t nl = std::min(lev_chunk, nlev - l0), nc = std::min(cell_chunk, cells - c0);
        const size_t off = l0 * cells + c0, bytes = nl * nc * sizeof(float); // more than one level only where nc == cells
        for (size_t j = 0; host && j < mem.size(); ++j)
          MIFC_HIP(c, hipMemcpyAsync(const_cast<float*>(mem[j]), a.fields[j] + off, bytes, hipMemcpyHostToDevice, c->stream));
        P.nlev = (int)nl;
        P.lev0 = (int)l0;
        P.n = (int)nc;
        P.stride = (long)nc;
        if (!launch())
          return 0;
        launches += 1;
        for (size_t k = 0; host && k < out.size(); ++k)
          MIFC_HIP(c, hipMemcpyAsync(out_host_[k] + off, out[k], bytes, hipMemcpyDeviceToHost, c->stream));
      }
    return 1;
  }
  int finish(mifc_ctx* c, Staging& st); // the counters back, then the call's one synchronisation
  int classify(size_t counter, size_t cells) const { return mifc_classify(counts_[counter], (u64)cells); }

private:
  std::vector<u64> counts_;
  float* const* out_host_ = nullptr;
};

// mifc_last_ensemble_form (include/mifc.h): what the calling thread's last member-batch call launched.  An entry fills
// one in as it decides and notes it once, when the call has succeeded; it is formatted only when asked for.
struct EnsembleForm
{
  enum { NONE = -1, SINGLE, LEVELS, QUANTILES };
  int entry = NONE;
  int c = 0, tail = 0;                  // SINGLE, LEVELS
  int welford = 0, flagged = 0, np = 0; // LEVELS: the template arguments of the instance
  int tier = 0;                         // QUANTILES
  int inline_args = 0, launches = 0, partials = 0;
  size_t lev_chunk = 0, cell_chunk = 0;
};
void note_ensemble_form(const EnsembleForm& form);

// What does not fit the kernel arguments: sections (where from, bytes), each on the 16-byte grid of one device block that
// is uploaded once from `host`, which has to live until the stream is synchronised.  dev[i]: where section i is.
typedef std::pair<const void*, size_t> Section;
int upload_table(mifc_ctx* c, Staging& st, std::vector<unsigned char>& host, std::initializer_list<Section> sections,
                 const unsigned char** dev);

} // namespace mifc_host

#endif // MIFC_MEMBERBATCH_H
