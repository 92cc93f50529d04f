// mifc_capi_hstats.hip -- C ABI of mifc_hstats_levels (include/mifc.h; EXTENSION, no reference function): its refusals
// (the head of the call, the overlap rule and the level table are the ones of mifc_levelbatch.h), the passes over the
// fields -- four per launch of the segment kernel of mifc_hstats.hip -- and, for host memory, the bands of rows.  Rows
// are independent up to rule 4, so a band of rows of every level (mifc_levelbatch.h's BandPlan) is a complete problem
// for the segment kernel; the partials of all bands lie in one block in box order, and ONE combine launch behind the
// last band adds them exactly as it does behind the single launch of a device call: the same bits whatever the staging.
#include "mifc_levelbatch.h"

#include <cstdio>

using namespace mifc_host;

static_assert(MIFC_HSTATS_AREA == mifc::HSTATS_AREA && MIFC_HSTATS_ROWS == mifc::HSTATS_ROWS && MIFC_HSTATS_MOMENTS == mifc::HSTATS_MOMENTS &&
                  MIFC_HSTATS_EXTREMES == mifc::HSTATS_EXTREMES,
              "HstatsParams::products, HstatsCombineParams::mode");

namespace {

// mifc_last_hstats_form: the shape of the calling thread's last segment launch and the launches of its call
struct HstatsForm
{
  int mode = -1, v = 0, nf = 0, w = 0, minus = 0, tested = 0, products = 0, segs = 0, blocks = 0, launches = 0, bands = 0;
};
thread_local HstatsForm t_form;
thread_local char t_form_text[192];

const char* const MINUS_NAMES[mifc::HSTATS_MAX_FIELDS] = {"minus[0]", "minus[1]", "minus[2]", "minus[3]", "minus[4]", "minus[5]", "minus[6]", "minus[7]"};

} // namespace

extern "C" {

int mifc_hstats_levels(mifc_ctx* c, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields,
                       const float* const* minus, const int* fdefined_minus, const double* pivot, const float* weight, int fdef_weight,
                       const int* box, int mode, int products, double* stats, float* const* mean, int* fdefined_mean, float undef, int memkind)
{
  CTX_OR_FAIL(c);
  // (the head of a level-batch call without a coordinate: what the shared checks and the level table read)
  const LevelBatchCall a = {"mifc_hstats_levels", COORD_LEVELS, nx, ny, nlev, fields, fdefined_in, nfields, nullptr, MIFC_SOME_DEFINED, nullptr,
                            nullptr, nullptr, undef, memkind};
  if (c->capturing)
    return refuse(c, a, "not available while a mifc_graph capture is open");
  if (nlev < 1)
    return refuse(c, a, "nlev < 1");
  if (nfields < 1 || nfields > mifc::HSTATS_MAX_FIELDS)
    return refuse(c, a, "nfields " + std::to_string(nfields) + " outside 1.." + std::to_string(mifc::HSTATS_MAX_FIELDS));
  if (nx < 1 || ny < 1)
    return refuse(c, a, "nx < 1 or ny < 1");
  if (!check_grid(c, a) || !check_levels(c, a)) // memkind; the cell limit
    return 0;
  if (mode != MIFC_HSTATS_AREA && mode != MIFC_HSTATS_ROWS)
    return refuse(c, a, "unknown mode " + std::to_string(mode));
  if (products == 0 || (products & ~(MIFC_HSTATS_MOMENTS | MIFC_HSTATS_EXTREMES)) != 0)
    return refuse(c, a, "products " + std::to_string(products) + ": no product or unknown bits");
  if (mean && (products & MIFC_HSTATS_MOMENTS) == 0)
    return refuse(c, a, "mean without MIFC_HSTATS_MOMENTS");
  if (!fields || !stats || (mean && !fdefined_mean))
    return refuse(c, a, "a null pointer (fields, stats or fdefined_mean)");
  const int nf = nfields;
  for (int f = 0; f < nf; ++f) {
    if (!fields[f] || (mean && !mean[f]))
      return refuse(c, a, "a null pointer (fields[" + std::to_string(f) + "] or mean[" + std::to_string(f) + "])");
    if (minus && !minus[f])
      return refuse(c, a, "a null pointer (minus[" + std::to_string(f) + "]): minus is given for every field or for none");
  }
  const int i0 = box ? box[0] : 0, i1 = box ? box[1] : nx, j0 = box ? box[2] : 0, j1 = box ? box[3] : ny;
  if (i0 < 0 || i1 > nx || i0 >= i1 || j0 < 0 || j1 > ny || j0 >= j1)
    return refuse(c, a, "the box {" + std::to_string(i0) + ", " + std::to_string(i1) + ", " + std::to_string(j0) + ", " + std::to_string(j1) +
                            "} is empty or outside the grid");
  const size_t cells = a.cells(), levels = (size_t)nlev, box_rows = (size_t)(j1 - j0), nrows = mode == MIFC_HSTATS_AREA ? 1 : box_rows;
  const size_t n_stats = (size_t)nf * levels * nrows * 8;
  {
    float* const stats_as_floats = reinterpret_cast<float*>(stats); // (the overlap rule goes by byte range)
    const float* const* m = minus;
    if (!check_overlaps(c, a, {{&stats_as_floats, 1, n_stats * sizeof(double), "stats"}, {mean, mean ? nf : 0, levels * nrows * sizeof(float), "mean"}},
                        {{weight, cells * sizeof(float), "weight"},
                         {m && nf > 0 ? m[0] : nullptr, cells * levels * sizeof(float), MINUS_NAMES[0]},
                         {m && nf > 1 ? m[1] : nullptr, cells * levels * sizeof(float), MINUS_NAMES[1]},
                         {m && nf > 2 ? m[2] : nullptr, cells * levels * sizeof(float), MINUS_NAMES[2]},
                         {m && nf > 3 ? m[3] : nullptr, cells * levels * sizeof(float), MINUS_NAMES[3]},
                         {m && nf > 4 ? m[4] : nullptr, cells * levels * sizeof(float), MINUS_NAMES[4]},
                         {m && nf > 5 ? m[5] : nullptr, cells * levels * sizeof(float), MINUS_NAMES[5]},
                         {m && nf > 6 ? m[6] : nullptr, cells * levels * sizeof(float), MINUS_NAMES[6]},
                         {m && nf > 7 ? m[7] : nullptr, cells * levels * sizeof(float), MINUS_NAMES[7]}}))
      return 0;
  }

  // the level table: one counter per field and level (rows whose mean is undef), the bits of the fields' flags, the bits
  // of the minus batches' flags next to them, the pivots behind it
  const size_t n_counts = (size_t)nf * levels;
  LevelTable tab;
  Staging st(c, memkind);
  if (!tab.build(c, a, n_counts, n_counts * sizeof(double)))
    return 0;
  bool tested = weight && fdef_weight != MIFC_ALL_DEFINED;
  for (size_t j = 0; j < n_counts; ++j) {
    tested |= !fdefined_in || fdefined_in[j] != MIFC_ALL_DEFINED;
    tested |= minus && (!fdefined_minus || fdefined_minus[j] != MIFC_ALL_DEFINED);
    static_cast<double*>(tab.tail())[j] = pivot ? pivot[j] : 0.0;
  }
  if (minus && fdefined_minus)
    for (size_t k = 0; k < levels; ++k)
      for (int f = 0; f < nf; ++f)
        if (fdefined_minus[(size_t)f * levels + k] == MIFC_ALL_DEFINED)
          tab.bits()[k] |= 1u << (mifc::HSTATS_MINUS_BIT + f);
  if (!tab.upload(c, st))
    return 0;

  const int seg0 = i0 / mifc::HSTATS_SEGMENT, segs = (i1 - 1) / mifc::HSTATS_SEGMENT - seg0 + 1;
  const size_t n_part = n_counts * box_rows * (size_t)segs * 8;
  double* part = static_cast<double*>(st.scratch(n_part * sizeof(double)));
  const bool host = memkind == MIFC_MEM_HOST;
  double* d_stats = host ? static_cast<double*>(st.scratch(n_stats * sizeof(double))) : stats;
  if (!st.ok())
    return 0;
  const bool partial = products != (MIFC_HSTATS_MOMENTS | MIFC_HSTATS_EXTREMES);
  if (host && partial) // (the slots of the group that is not requested keep the caller's content)
    MIFC_HIP(c, hipMemcpyAsync(d_stats, stats, n_stats * sizeof(double), hipMemcpyHostToDevice, c->stream));

  // where the planes are: the caller's, or a band of rows of every level at a time
  BandPlan plan;
  PlaneGroup *gx[mifc::HSTATS_MAX_FIELDS], *gy[mifc::HSTATS_MAX_FIELDS];
  for (int f = 0; f < nf; ++f)
    gx[f] = plan.in(fields[f], levels);
  for (int f = 0; f < nf; ++f)
    gy[f] = plan.in(minus ? minus[f] : nullptr, levels);
  PlaneGroup* gw = plan.in(weight, 1);
  if (!plan.place(c, st, a, (size_t)(mifc::env().hstats_chunk_mib > 0 ? mifc::env().hstats_chunk_mib : 256) << 20))
    return 0;

  mifc::HstatsParams P;
  std::memset(&P, 0, sizeof P);
  P.nx = nx;
  P.nlev = nlev;
  P.i0 = i0;
  P.i1 = i1;
  P.box_rows = (int)box_rows;
  P.seg0 = seg0;
  P.segs = segs;
  P.products = products;
  P.tested = tested ? 1 : 0;
  P.weight_all = fdef_weight == MIFC_ALL_DEFINED ? 1 : 0;
  P.vec4 = (plan.vec4 && (nx & 3) == 0) ? 1 : 0; // every ROW on the 16-byte grid, not only every plane
  P.undef = undef;
  P.stride = plan.stride;
  P.weight = gw->dev;
  P.lev_bits = tab.lev_bits();
  P.pivot = static_cast<const double*>(tab.dev_tail());
  P.part = part;

  HstatsForm form;
  form.mode = mode;
  form.v = P.vec4 ? 4 : 1;
  form.nf = std::min(mifc::HSTATS_PASS, nf);
  form.w = weight ? 1 : 0;
  form.minus = minus ? 1 : 0;
  form.tested = P.tested;
  form.products = products;
  form.segs = segs;
  const int ran = plan.run(c, a, [&](const BandRows& band) {
    const size_t band_row0 = (size_t)band.first, band_rows = (size_t)band.staged; // the grid row of the planes' row 0, their rows
    const size_t lo = std::max(band_row0, (size_t)j0), hi = std::min(band_row0 + band_rows, (size_t)j1); // the box's rows in this band
    form.bands += 1;
    if (lo < hi) {
      P.rows = (int)(hi - lo);
      P.plane_row0 = (int)(lo - band_row0);
      P.grid_row0 = (int)lo;
      P.part_row0 = (int)(lo - (size_t)j0);
      for (int f0 = 0; f0 < nf; f0 += mifc::HSTATS_PASS) {
        P.f0 = f0;
        P.nfields = std::min(mifc::HSTATS_PASS, nf - f0);
        for (int f = 0; f < mifc::HSTATS_PASS; ++f) {
          P.fields[f] = f < P.nfields ? gx[f0 + f]->dev : nullptr;
          P.minus[f] = f < P.nfields ? gy[f0 + f]->dev : nullptr;
        }
        MIFC_LAUNCH(c, mifc::launch_hstats_segments(P, c->stream));
        form.launches += 1;
      }
      form.blocks = mifc::hstats_plan(P.rows, segs, nlev).blocks;
    }
    return 1;
  });
  if (!ran)
    return 0;

  mifc::HstatsCombineParams Q;
  std::memset(&Q, 0, sizeof Q);
  Q.nfields = nf;
  Q.nlev = nlev;
  Q.box_rows = (int)box_rows;
  Q.segs = segs;
  Q.mode = mode;
  Q.products = products;
  Q.undef = undef;
  Q.part = part;
  Q.pivot = P.pivot;
  Q.stats = d_stats;
  Q.n_undefined = tab.n_undefined();
  if (mean)
    for (int f = 0; f < nf; ++f)
      Q.mean[f] = st.out(mean[f], levels * nrows);
  if (!st.ok())
    return 0;
  MIFC_LAUNCH(c, mifc::launch_hstats_combine(Q, c->stream));
  if (host)
    MIFC_HIP(c, hipMemcpyAsync(stats, d_stats, n_stats * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  if (!tab.read_counts(c) || !st.finish()) // finish(): the one synchronisation of the call
    return 0;
  t_form = form;
  if (mean)
    for (size_t j = 0; j < n_counts; ++j)
      fdefined_mean[j] = tab.classify(j, nrows);
  return 1;
}

const char* mifc_last_hstats_form(void)
{
  const HstatsForm& f = t_form;
  if (f.mode < 0)
    return "";
  std::snprintf(t_form_text, sizeof t_form_text, "mode=%s v=%d nf=%d w=%d minus=%d tested=%d products=%d segs=%d blocks=%d launches=%d bands=%d",
                f.mode == MIFC_HSTATS_AREA ? "area" : "rows", f.v, f.nf, f.w, f.minus, f.tested, f.products, f.segs, f.blocks, f.launches, f.bands);
  return t_form_text;
}

} // extern "C"
