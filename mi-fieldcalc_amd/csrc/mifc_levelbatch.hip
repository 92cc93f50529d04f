// mifc_levelbatch.hip -- the host driver of the level-batch entries (mifc_levelbatch.h).
#include "mifc_levelbatch.h"

#include <cstdint>

namespace mifc_host {

int refuse(mifc_ctx* c, const LevelBatchCall& a, const std::string& why)
{
  c->err = std::string(a.name) + ": " + why;
  return 0;
}

int check_counts(mifc_ctx* c, const LevelBatchCall& a, int max_fields)
{
  if (c->capturing)
    return refuse(c, a, "not available while a mifc_graph capture is open");
  if (a.nlev < 2)
    return refuse(c, a, "nlev < 2");
  if (a.nfields < 1 || a.nfields > max_fields)
    return refuse(c, a, "nfields " + std::to_string(a.nfields) + " outside 1.." + std::to_string(max_fields));
  return 1;
}

int check_grid(mifc_ctx* c, const LevelBatchCall& a)
{
  if (a.nx < 0 || a.ny < 0)
    return refuse(c, a, "a negative nx or ny");
  if (a.memkind != MIFC_MEM_HOST && a.memkind != MIFC_MEM_DEVICE)
    return refuse(c, a, "unknown memkind " + std::to_string(a.memkind));
  return 1;
}

int check_field_pointers(mifc_ctx* c, const LevelBatchCall& a, float* const* fres)
{
  for (int f = 0; f < a.nfields; ++f)
    if (!a.fields[f] || (fres && !fres[f]))
      return refuse(c, a, "a null pointer (fields[" + std::to_string(f) + "] or fres[" + std::to_string(f) + "])");
  return 1;
}

int check_levels(mifc_ctx* c, const LevelBatchCall& a)
{
  if (a.hybrid())
    for (int k = 0; k < a.nlev; ++k)
      if (bad_hlevel(a.alevel[k], a.blevel[k]))
        return refuse(c, a, "level " + std::to_string(k) + ": alevel / blevel are no hybrid level (FieldCalculations.cc:298)");
  if ((long)a.nx * (long)a.ny > 0x7fffffffL)
    return refuse(c, a, "more than 2^31 - 1 cells per level");
  return 1;
}

int check_overlaps(mifc_ctx* c, const LevelBatchCall& a, std::initializer_list<Outputs> out_lists, std::initializer_list<Input> more_inputs)
{
  struct NamedRange
  {
    const void* p;
    size_t bytes;
    std::string name;
  };
  try { // nothing may be thrown across the C ABI
    std::vector<NamedRange> ins, outs;
    if (a.coord_planes() != 0)
      ins.push_back({a.coord, a.cells() * a.coord_planes() * sizeof(float), a.hybrid() ? "ps" : "coord"});
    for (const Input& i : more_inputs)
      if (i.p)
        ins.push_back({i.p, i.bytes, i.name});
    for (int g = 0; g < a.nfields; ++g)
      ins.push_back({a.fields[g], a.cells() * (size_t)a.nlev * sizeof(float), "fields[" + std::to_string(g) + "]"});
    for (const Outputs& l : out_lists)
      for (int i = 0; i < l.n; ++i)
        outs.push_back({l.p[i], l.bytes, l.name + ("[" + std::to_string(i) + "]")});
    for (const NamedRange& o : outs) {
      for (const NamedRange& i : ins)
        if (overlaps(o.p, o.bytes, i.p, i.bytes))
          return refuse(c, a, o.name + " overlaps " + i.name);
      for (const NamedRange& q : outs)
        if (&q != &o && overlaps(o.p, o.bytes, q.p, q.bytes))
          return refuse(c, a, o.name + " overlaps " + q.name);
    }
  } catch (...) {
    c->err = "out of host memory";
    return 0;
  }
  return 1;
}

int LevelTable::build(mifc_ctx* c, const LevelBatchCall& a, size_t n_counts, size_t tail_bytes)
{
  const size_t nlev = (size_t)a.nlev;
  o_ab_ = align_up(n_counts * sizeof(u64), 16);
  o_bits_ = o_ab_ + align_up(2 * nlev * sizeof(float), 16);
  o_tail_ = o_bits_ + align_up(nlev * sizeof(unsigned int), 16);
  try { // nothing may be thrown across the C ABI
    host_.assign(o_tail_ + tail_bytes, 0);
    counts_.assign(n_counts, 0);
  } catch (...) {
    c->err = "out of host memory";
    return 0;
  }
  if (a.hybrid()) {
    std::memcpy(host_.data() + o_ab_, a.alevel, nlev * sizeof(float));
    std::memcpy(host_.data() + o_ab_ + nlev * sizeof(float), a.blevel, nlev * sizeof(float));
  }
  for (size_t k = 0; k < nlev; ++k) {
    unsigned int b = 0;
    if (a.fdefined_in)
      for (int f = 0; f < a.nfields; ++f)
        if (a.fdefined_in[(size_t)f * nlev + k] == MIFC_ALL_DEFINED)
          b |= 1u << f;
    if (a.kind == COORD_FIELD && a.fdef_coord && a.fdef_coord[k] == MIFC_ALL_DEFINED)
      b |= 1u << mifc::VINTERP_COORD_BIT;
    bits()[k] = b;
  }
  return 1;
}

int LevelTable::upload(mifc_ctx* c, Staging& st)
{
  dev_ = static_cast<unsigned char*>(st.scratch(host_.size()));
  if (!st.ok())
    return 0;
  MIFC_HIP(c, hipMemcpyAsync(dev_, host_.data(), host_.size(), hipMemcpyHostToDevice, c->stream));
  return 1;
}

int LevelTable::read_counts(mifc_ctx* c)
{
  MIFC_HIP(c, hipMemcpyAsync(counts_.data(), dev_, counts_.size() * sizeof(u64), hipMemcpyDeviceToHost, c->stream));
  return 1;
}

void vderiv_level_weights(LevelTable& tab, const LevelBatchCall& a, int method)
{
  const int nlev = a.nlev;
  const float* lv = a.coord;
  double* w = static_cast<double*>(tab.tail());
  for (int k = 0; k < nlev; ++k) {
    const bool lower = k > 0 && lv[k - 1] != lv[k], upper = k < nlev - 1 && lv[k + 1] != lv[k];
    const double d0 = (double)lv[k], dm = k > 0 ? (double)lv[k - 1] : 0.0, dp = k < nlev - 1 ? (double)lv[k + 1] : 0.0;
    const double h1 = d0 - dm, h2 = dp - d0;
    if (lower)
      w[4 * k] = 1.0 / h1;
    if (upper)
      w[4 * k + 1] = 1.0 / h2;
    bool fold = false;
    if (lower && upper) {
      if (method == MIFC_VDERIV_WEIGHTED) {
        const double s = h1 + h2;
        fold = s == 0.0;
        if (!fold) {
          const double p1 = h1 * s, p2 = h2 * s;
          w[4 * k + 2] = h2 / p1;
          w[4 * k + 3] = h1 / p2;
        }
      } else {
        const double dc = dp - dm;
        fold = dc == 0.0;
        if (!fold)
          w[4 * k + 2] = 1.0 / dc;
      }
    }
    tab.bits()[k] |= (lower ? 1u << mifc::VDERIV_LOWER_BIT : 0u) | (upper ? 1u << mifc::VDERIV_UPPER_BIT : 0u) | (fold ? 1u << mifc::VDERIV_FOLD_BIT : 0u);
  }
}

int BandPlan::place(mifc_ctx* c, Staging& st, const LevelBatchCall& a, size_t budget, int halo_rows)
{
  if (a.memkind != MIFC_MEM_HOST) {
    uintptr_t all = 0;
    for (int i = 0; i < n_; ++i) {
      g_[i].dev = g_[i].host;
      all |= reinterpret_cast<uintptr_t>(g_[i].host);
    }
    stride = (long)a.cells();
    vec4 = ((a.cells() & 3) == 0 && (all & 15) == 0) ? 1 : 0;
    return 1;
  }
  size_t planes = 0;
  for (int i = 0; i < n_; ++i)
    planes += g_[i].planes;
  const size_t nx = (size_t)a.nx, ny = (size_t)a.ny, around = 2 * (size_t)halo_rows;
  size_t staged = plan_band(budget, planes, nx, ny);
  if (around != 0)
    staged = std::min(ny, std::max(around + 1, staged));
  const size_t S = align_up(staged * nx, 64);
  float* d = static_cast<float*>(st.scratch(planes * S * sizeof(float)));
  if (!st.ok())
    return 0;
  for (int i = 0; i < n_; ++i) {
    g_[i].dev = g_[i].planes ? d : nullptr;
    d += g_[i].planes * S;
  }
  own_ = (int)(staged >= ny ? ny : staged - around);
  halo_ = halo_rows;
  stride = (long)S;
  vec4 = 1;
  return 1;
}

} // namespace mifc_host
