// mifc_capi_hdist.hip -- C ABI of mifc_hdist_histogram_levels and mifc_hdist_quantile_levels (include/mifc.h; EXTENSION,
// no reference function): their refusals (the head of the call, the overlap rule and the level table are the ones of
// mifc_levelbatch.h, without a coordinate; the edge check is mifc_hdist_rules.h), the launches of mifc_hdist.hip and, for
// host memory, the staging.  Counts add, so a histogram of host memory runs band of rows by band of rows
// (mifc_levelbatch.h's BandPlan) into one device result: exactly the counts of a device call.  An order statistic needs
// every cell of its level, so the percentiles of host memory run chunk of whole levels by chunk, all passes of the
// selection while the chunk is resident; device memory is walked in blocks of levels too, so that the digit counters
// (fields * levels * prefixes * 2048 words) stay within MIFC_HDIST_CHUNK_MIB.
#include "mifc_hdist_rules.h"
#include "mifc_levelbatch.h"

#include <cstdint>
#include <cstdio>

using namespace mifc_host;

static_assert(MIFC_QUANTILE_LOWER == mifc::HDIST_LOWER && MIFC_QUANTILE_LINEAR == mifc::HDIST_LINEAR, "HdistSelectParams::method");

namespace {

// mifc_last_hdist_form: the shape of the calling thread's last call
struct HdistForm
{
  int entry = -1, mode = 0, v = 0, nf = 0, nbins = 0, mask = 0, tested = 0, prefix = 0, passes = 0, launches = 0, bands = 0, chunks = 0;
};
thread_local HdistForm t_form;
thread_local char t_form_text[224];

struct Box
{
  int i0, i1, j0, j1;
};

// the refusals that the two entries share behind their own counts; 0 with the context's error set
int check_head(mifc_ctx* c, const LevelBatchCall& a, const int* box, Box& b)
{
  if (a.nlev < 1)
    return refuse(c, a, "nlev < 1");
  if (a.nfields < 1 || a.nfields > mifc::HDIST_MAX_FIELDS)
    return refuse(c, a, "nfields " + std::to_string(a.nfields) + " outside 1.." + std::to_string(mifc::HDIST_MAX_FIELDS));
  if (a.nx < 1 || a.ny < 1)
    return refuse(c, a, "nx < 1 or ny < 1");
  if (!check_grid(c, a) || !check_levels(c, a)) // memkind; the cell limit
    return 0;
  b = {box ? box[0] : 0, box ? box[1] : a.nx, box ? box[2] : 0, box ? box[3] : a.ny};
  if (b.i0 < 0 || b.i1 > a.nx || b.i0 >= b.i1 || b.j0 < 0 || b.j1 > a.ny || b.j0 >= b.j1)
    return refuse(c, a, "the box {" + std::to_string(b.i0) + ", " + std::to_string(b.i1) + ", " + std::to_string(b.j0) + ", " + std::to_string(b.j1) +
                            "} is empty or outside the grid");
  return 1;
}

bool any_tested(const LevelBatchCall& a, const float* mask, int fdef_mask)
{
  bool tested = mask && fdef_mask != MIFC_ALL_DEFINED;
  for (size_t j = 0; j < (size_t)a.nfields * (size_t)a.nlev; ++j)
    tested |= !a.fdefined_in || a.fdefined_in[j] != MIFC_ALL_DEFINED;
  return tested;
}

bool on_16(const void* p)
{
  return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

size_t budget_bytes()
{
  return (size_t)(mifc::env().hdist_chunk_mib > 0 ? mifc::env().hdist_chunk_mib : 256) << 20;
}

} // namespace

extern "C" {

int mifc_hdist_histogram_levels(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields,
                                const float* edges, int nedges, const float* mask, int fdef_mask, const int* box, int mode, int* hist, float undef,
                                int memkind)
{
  CTX_OR_FAIL(c);
  // (the head of a level-batch call without a coordinate: what the shared checks and the level table read)
  const LevelBatchCall a = {"mifc_hdist_histogram_levels", COORD_LEVELS, nx, ny, nlev, fields, fdefined_in, nfields, nullptr, MIFC_SOME_DEFINED, nullptr,
                            nullptr, nullptr, undef, memkind};
  if (c->capturing)
    return refuse(c, a, "not available while a mifc_graph capture is open");
  Box b;
  if (!check_head(c, a, box, b))
    return 0;
  if (mode != MIFC_HSTATS_AREA && mode != MIFC_HSTATS_ROWS)
    return refuse(c, a, "unknown mode " + std::to_string(mode));
  if (nedges < 1 || nedges > mifc::HDIST_MAX_EDGES)
    return refuse(c, a, "nedges " + std::to_string(nedges) + " outside 1.." + std::to_string(mifc::HDIST_MAX_EDGES));
  if (!fields || !edges || !hist)
    return refuse(c, a, "a null pointer (fields, edges or hist)");
  const int nf = nfields;
  for (int f = 0; f < nf; ++f) {
    if (!fields[f])
      return refuse(c, a, "a null pointer (fields[" + std::to_string(f) + "])");
    const int bad = mifc::hdist_check_edges(edges + (size_t)f * nedges, nedges);
    if (bad >= 0)
      return refuse(c, a, "field " + std::to_string(f) + ": edge " + std::to_string(bad) + " is NaN or not above the edge before it");
  }
  const size_t cells = a.cells(), levels = (size_t)nlev, box_rows = (size_t)(b.j1 - b.j0), nrows = mode == MIFC_HSTATS_AREA ? 1 : box_rows;
  const size_t nslots = (size_t)nedges + 2, n_hist = (size_t)nf * levels * nrows * nslots;
  {
    float* const hist_as_floats = reinterpret_cast<float*>(hist); // (the overlap rule goes by byte range)
    if (!check_overlaps(c, a, {{&hist_as_floats, 1, n_hist * sizeof(int), "hist"}}, {{mask, cells * sizeof(float), "mask"}}))
      return 0;
  }

  // the level table: the bits of the fields' flags, the edges as bin keys behind it
  LevelTable tab;
  Staging st(c, memkind);
  if (!tab.build(c, a, 0, (size_t)nf * nedges * sizeof(unsigned int)))
    return 0;
  for (size_t e = 0; e < (size_t)nf * nedges; ++e)
    static_cast<unsigned int*>(tab.tail())[e] = mifc::hdist_bin_key(mifc::hdist_float_bits(edges[e]));
  if (!tab.upload(c, st))
    return 0;
  const bool tested = any_tested(a, mask, fdef_mask);
  const float* const mask_used = (mask && fdef_mask != MIFC_ALL_DEFINED) ? mask : nullptr; // (a mask that is all defined excludes nothing)

  const bool host = memkind == MIFC_MEM_HOST;
  int* d_hist = host ? static_cast<int*>(st.scratch(n_hist * sizeof(int))) : hist;
  if (!st.ok())
    return 0;
  MIFC_LAUNCH(c, hipMemsetAsync(d_hist, 0, n_hist * sizeof(int), c->stream));

  // where the planes are: the caller's, or a band of rows of every level at a time
  BandPlan plan;
  PlaneGroup* gx[mifc::HDIST_MAX_FIELDS];
  for (int f = 0; f < nf; ++f)
    gx[f] = plan.in(fields[f], levels);
  PlaneGroup* gm = plan.in(mask_used, 1);
  if (!plan.place(c, st, a, budget_bytes()))
    return 0;

  mifc::HdistParams P;
  std::memset(&P, 0, sizeof P);
  P.what = mifc::HDIST_COUNT;
  P.nx = nx;
  P.nlev = nlev;
  P.call_nlev = nlev;
  P.nfields = nf;
  P.i0 = b.i0;
  P.i1 = b.i1;
  P.tested = tested ? 1 : 0;
  P.mask_all = 0;
  P.plain = mifc::env().hdist_aggregate ? 0 : 1;
  P.vec4 = (plan.vec4 && (nx & 3) == 0) ? 1 : 0; // every ROW on the 16-byte grid, not only every plane
  P.undef = undef;
  P.stride = plan.stride;
  for (int f = 0; f < nf; ++f)
    P.fields[f] = gx[f]->dev;
  P.mask = gm->dev;
  P.lev_bits = tab.lev_bits();
  P.nedges = nedges;
  P.out_rows = (int)nrows;
  P.per_row = mode == MIFC_HSTATS_ROWS ? 1 : 0;
  P.edge_keys = static_cast<const unsigned int*>(tab.dev_tail());
  P.hist = d_hist;

  HdistForm form;
  form.entry = 0;
  form.mode = mode;
  form.v = P.vec4 ? 4 : 1;
  form.nf = nf;
  form.nbins = nedges + 1;
  form.mask = mask_used ? 1 : 0;
  form.tested = P.tested;
  form.passes = 1;
  const int ran = plan.run(c, a, [&](const BandRows& band) {
    const int band_row0 = band.first, lo = std::max(band_row0, b.j0), hi = std::min(band_row0 + band.staged, b.j1); // the box's rows in this band
    form.bands += 1;
    if (lo < hi) {
      P.rows = hi - lo;
      P.plane_row0 = lo - band_row0;
      P.out_row0 = lo - b.j0;
      MIFC_LAUNCH(c, mifc::launch_hdist_walk(P, c->stream));
      form.launches += 1;
    }
    return 1;
  });
  if (!ran)
    return 0;
  if (host)
    MIFC_HIP(c, hipMemcpyAsync(hist, d_hist, n_hist * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (!st.finish()) // the one synchronisation of the call
    return 0;
  t_form = form;
  return 1;
}

int mifc_hdist_quantile_levels(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields,
                               const float* percentiles, int nq, int method, const float* mask, int fdef_mask, const int* box, float* quant,
                               int* fdefined_q, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  const LevelBatchCall a = {"mifc_hdist_quantile_levels", COORD_LEVELS, nx, ny, nlev, fields, fdefined_in, nfields, nullptr, MIFC_SOME_DEFINED, nullptr,
                            nullptr, nullptr, undef, memkind};
  if (c->capturing)
    return refuse(c, a, "not available while a mifc_graph capture is open");
  Box b;
  if (!check_head(c, a, box, b))
    return 0;
  if (method != MIFC_QUANTILE_LOWER && method != MIFC_QUANTILE_LINEAR)
    return refuse(c, a, "unknown method " + std::to_string(method));
  if (nq < 1 || nq > mifc::HDIST_MAX_Q)
    return refuse(c, a, "nq " + std::to_string(nq) + " outside 1.." + std::to_string(mifc::HDIST_MAX_Q));
  if (!fields || !percentiles || !quant || !fdefined_q)
    return refuse(c, a, "a null pointer (fields, percentiles, quant or fdefined_q)");
  const int nf = nfields;
  for (int f = 0; f < nf; ++f)
    if (!fields[f])
      return refuse(c, a, "a null pointer (fields[" + std::to_string(f) + "])");
  for (int q = 0; q < nq; ++q)
    if (!(percentiles[q] >= 0.0f && percentiles[q] <= 100.0f))
      return refuse(c, a, "percentile " + std::to_string(q) + " is NaN or outside [0, 100]");
  const size_t cells = a.cells(), levels = (size_t)nlev, n_quant = (size_t)nf * levels * (size_t)nq;
  if (!check_overlaps(c, a, {{&quant, 1, n_quant * sizeof(float), "quant"}}, {{mask, cells * sizeof(float), "mask"}}))
    return 0;

  // the level table: one counter per field and level (percentiles left undef), the bits of the flags, the percentiles
  const size_t n_counts = (size_t)nf * levels;
  LevelTable tab;
  Staging st(c, memkind);
  if (!tab.build(c, a, n_counts, (size_t)nq * sizeof(float)))
    return 0;
  std::memcpy(tab.tail(), percentiles, (size_t)nq * sizeof(float));
  if (!tab.upload(c, st))
    return 0;
  const bool tested = any_tested(a, mask, fdef_mask), host = memkind == MIFC_MEM_HOST;
  const float* const mask_used = (mask && fdef_mask != MIFC_ALL_DEFINED) ? mask : nullptr;
  const float* const d_mask = mask_used ? st.in(mask_used, cells) : nullptr;

  // A block of L levels: the units and the digit counters of its (field, level)s and, for host memory, its cells; never
  // less than a level.
  const size_t slots = std::min<size_t>(mifc::HDIST_MAX_RANKS, (size_t)nq * (method == MIFC_QUANTILE_LINEAR ? 2 : 1));
  const size_t hist_words = slots * mifc::HDIST_DIGIT_BINS;
  const size_t per_level = (size_t)nf * (hist_words * sizeof(unsigned int) + sizeof(mifc::HdistUnit) + (host ? cells * sizeof(float) : 0));
  const size_t L = std::max<size_t>(1, std::min<size_t>(levels, budget_bytes() / per_level));
  const size_t units = (size_t)nf * L;
  mifc::HdistUnit* d_units = static_cast<mifc::HdistUnit*>(st.scratch(units * sizeof(mifc::HdistUnit)));
  unsigned int* d_digits = static_cast<unsigned int*>(st.scratch(units * hist_words * sizeof(unsigned int)));
  float* staged = host ? static_cast<float*>(st.scratch(units * cells * sizeof(float))) : nullptr;
  float* d_quant = st.out(quant, n_quant);
  if (!st.ok())
    return 0;
  std::vector<unsigned int> extents; // n, kmin, kmax and a pad of every unit of every block, for the form
  try {                              // nothing may be thrown across the C ABI
    extents.assign(4 * (size_t)nf * ((levels + L - 1) / L) * L, 0u);
  } catch (...) {
    c->err = "out of host memory";
    return 0;
  }

  mifc::HdistParams P;
  std::memset(&P, 0, sizeof P);
  P.nx = nx;
  P.nfields = nf;
  P.i0 = b.i0;
  P.i1 = b.i1;
  P.rows = b.j1 - b.j0;
  P.plane_row0 = b.j0;
  P.tested = tested ? 1 : 0;
  P.undef = undef;
  P.stride = (long)cells;
  P.mask = d_mask;
  P.lev_bits = tab.lev_bits();
  P.units = d_units;
  P.digit_hist = d_digits;
  P.slot_stride = (int)slots;
  P.plain = mifc::env().hdist_aggregate ? 0 : 1;
  mifc::HdistSelectParams Q;
  std::memset(&Q, 0, sizeof Q);
  Q.call_nlev = nlev;
  Q.nq = nq;
  Q.method = method;
  Q.slot_stride = (int)slots;
  Q.undef = undef;
  Q.percentiles = static_cast<const float*>(tab.dev_tail());
  Q.units = d_units;
  Q.digit_hist = d_digits;
  for (int f = 0; f < nf; ++f)
    Q.quant[f] = d_quant + (size_t)f * levels * (size_t)nq;
  Q.n_undefined = tab.n_undefined();

  HdistForm form;
  form.entry = 1;
  form.mode = method;
  form.nf = nf;
  form.nbins = mifc::HDIST_DIGIT_BINS;
  form.mask = mask_used ? 1 : 0;
  form.tested = P.tested;
  size_t block = 0;
  for (size_t k0 = 0; k0 < levels; k0 += L, ++block) {
    const size_t n = std::min(L, levels - k0);
    bool grid16 = (nx & 3) == 0 && on_16(d_mask);
    for (int f = 0; f < nf; ++f) {
      if (host) {
        float* d = staged + (size_t)f * L * cells;
        MIFC_HIP(c, hipMemcpyAsync(d, fields[f] + k0 * cells, n * cells * sizeof(float), hipMemcpyHostToDevice, c->stream));
        P.fields[f] = d;
      } else {
        P.fields[f] = fields[f] + k0 * cells;
      }
      grid16 = grid16 && on_16(P.fields[f]);
    }
    P.vec4 = grid16 ? 1 : 0;
    P.nlev = (int)n;
    P.lev0 = (int)k0;
    P.unit_levels = (int)L;
    Q.nunits = (int)units;
    Q.unit_levels = (int)L;
    Q.lev0 = (int)k0;
    form.v = P.vec4 ? 4 : 1;
    form.chunks += 1;
    MIFC_LAUNCH(c, mifc::launch_hdist_init(Q, c->stream));
    P.what = mifc::HDIST_EXTENT;
    MIFC_LAUNCH(c, mifc::launch_hdist_walk(P, c->stream));
    MIFC_LAUNCH(c, mifc::launch_hdist_plan(Q, c->stream));
    form.launches += 1;
    P.what = mifc::HDIST_DIGIT;
    for (int pass = 0; pass < mifc::HDIST_MAX_PASSES; ++pass) { // (a unit that has its keys leaves the later passes at once)
      P.pass = Q.pass = pass;
      MIFC_LAUNCH(c, hipMemsetAsync(d_digits, 0, units * hist_words * sizeof(unsigned int), c->stream));
      MIFC_LAUNCH(c, mifc::launch_hdist_walk(P, c->stream));
      MIFC_LAUNCH(c, mifc::launch_hdist_scan(Q, c->stream));
      form.launches += 1;
    }
    // (the last block may hold fewer levels than units: the units beyond them stay as the init kernel left them, n == 0,
    // and the final kernel is given only the levels that exist)
    mifc::HdistSelectParams F = Q;
    if (n < L) { // units are [field][L]: the final kernel walks them as they lie, so it takes each field on its own
      for (int f = 0; f < nf; ++f) {
        F = Q;
        F.units = d_units + (size_t)f * L;
        F.nunits = (int)n;
        F.unit_levels = (int)n;
        F.quant[0] = Q.quant[f];
        F.n_undefined = Q.n_undefined + (size_t)f * levels;
        MIFC_LAUNCH(c, mifc::launch_hdist_final(F, c->stream));
      }
    } else {
      MIFC_LAUNCH(c, mifc::launch_hdist_final(F, c->stream));
    }
    MIFC_HIP(c, hipMemcpy2DAsync(extents.data() + 4 * block * units, 16, d_units, sizeof(mifc::HdistUnit), 16, units, hipMemcpyDeviceToHost, c->stream));
  }
  if (!tab.read_counts(c) || !st.finish()) // finish(): the one synchronisation of the call
    return 0;
  form.prefix = 32;
  for (size_t u = 0; u < extents.size() / 4; ++u)
    if (extents[4 * u] != 0u) {
      const mifc::HdistPlan plan = mifc::hdist_digit_plan(extents[4 * u + 1], extents[4 * u + 2]);
      form.prefix = std::min(form.prefix, plan.prefix_bits);
      form.passes = std::max(form.passes, plan.passes);
    }
  t_form = form;
  for (size_t j = 0; j < n_counts; ++j)
    fdefined_q[j] = tab.classify(j, (size_t)nq);
  return 1;
}

const char* mifc_last_hdist_form(void)
{
  const HdistForm& f = t_form;
  if (f.entry < 0)
    return "";
  const char* const mode = f.entry == 0 ? (f.mode == MIFC_HSTATS_AREA ? "area" : "rows") : (f.mode == MIFC_QUANTILE_LOWER ? "lower" : "linear");
  std::snprintf(t_form_text, sizeof t_form_text, "entry=%s mode=%s v=%d nf=%d nbins=%d mask=%d tested=%d prefix=%d passes=%d launches=%d bands=%d chunks=%d",
                f.entry == 0 ? "hist" : "quant", mode, f.v, f.nf, f.nbins, f.mask, f.tested, f.prefix, f.passes, f.launches, f.bands, f.chunks);
  return t_form_text;
}

} // extern "C"
