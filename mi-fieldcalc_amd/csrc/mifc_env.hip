// mifc_env.hip -- see mifc_env.h (host code only).
#include "mifc_env.h"

#include <cstdlib>
#include <cstring>
#include <mutex>

namespace mifc {

namespace {
Env g_env;
std::mutex g_env_mutex;

int positive_int(const char* name)
{
  const char* e = std::getenv(name);
  if (!e)
    return 0;
  const int v = std::atoi(e);
  return v > 0 ? v : 0;
}

bool not_zero(const char* name)
{
  const char* e = std::getenv(name);
  return !(e && e[0] == '0');
}
} // namespace

const Env& env()
{
  return g_env;
}

void env_reload()
{
  Env e;
  e.force_cell_kernel = std::getenv("MIFC_FORCE_CELL_KERNEL") != nullptr;
  e.host_pipeline = not_zero("MIFC_HOST_PIPELINE");
  e.fused2 = not_zero("MIFC_FUSED2");
  e.shapiro_fused = not_zero("MIFC_SHAPIRO_FUSED");
  e.shapiro_regs = not_zero("MIFC_SHAPIRO_REGS");
  e.ewise_max_blocks = positive_int("MIFC_EWISE_MAX_BLOCKS");
  if (const char* s = std::getenv("MIFC_SCALAR_ROWS_R")) {
    const int v = std::atoi(s);
    e.scalar_rows_r = v > 0 ? v : 0;
  }
  e.fused2_band = positive_int("MIFC_FUSED2_BAND");
  e.host_threads = positive_int("MIFC_HOST_THREADS");
  e.host_chunk_mib = positive_int("MIFC_HOST_CHUNK_MIB");
  e.host_pipe_min_kib = positive_int("MIFC_HOST_PIPE_MIN_KIB");
  e.host_chunk_levels = positive_int("MIFC_HOST_CHUNK_LEVELS");
  e.quantile_chunk_mib = positive_int("MIFC_QUANTILE_CHUNK_MIB");
  e.ensemble_chunk_mib = positive_int("MIFC_ENSEMBLE_CHUNK_MIB");
  e.vinterp_chunk_mib = positive_int("MIFC_VINTERP_CHUNK_MIB");
  e.vlayer_chunk_mib = positive_int("MIFC_VLAYER_CHUNK_MIB");
  e.vderiv_chunk_mib = positive_int("MIFC_VDERIV_CHUNK_MIB");
  e.vcumul_chunk_mib = positive_int("MIFC_VCUMUL_CHUNK_MIB");
  e.vregrid_chunk_mib = positive_int("MIFC_VREGRID_CHUNK_MIB");
  e.vregrid_tb = positive_int("MIFC_VREGRID_TB");
  e.vregrid_v = positive_int("MIFC_VREGRID_V");
  e.vparcel_chunk_mib = positive_int("MIFC_VPARCEL_CHUNK_MIB");
  e.pvort_chunk_mib = positive_int("MIFC_PVORT_CHUNK_MIB");
  e.hinterp_chunk_mib = positive_int("MIFC_HINTERP_CHUNK_MIB");
  e.hstats_chunk_mib = positive_int("MIFC_HSTATS_CHUNK_MIB");
  e.hdist_chunk_mib = positive_int("MIFC_HDIST_CHUNK_MIB");
  e.hdist_aggregate = not_zero("MIFC_HDIST_AGGREGATE");
  e.htraj_chunk_mib = positive_int("MIFC_HTRAJ_CHUNK_MIB");
  e.htraj_level_chunk = positive_int("MIFC_HTRAJ_LEVEL_CHUNK");
  e.hremap_chunk_mib = positive_int("MIFC_HREMAP_CHUNK_MIB");
  e.hremap_level_chunk = positive_int("MIFC_HREMAP_LEVEL_CHUNK");
  e.fexpr_chunk_mib = positive_int("MIFC_FEXPR_CHUNK_MIB");
  e.hinterp_level_chunk = positive_int("MIFC_HINTERP_LEVEL_CHUNK");
  e.derived_blocks = positive_int("MIFC_DERIVED_BLOCKS");
  e.derived_pipe = not_zero("MIFC_DERIVED_PIPE") ? 1 : 0;
  e.levelwalk = not_zero("MIFC_VORTDIV_LEVELWALK");
  e.split_roles = not_zero("MIFC_VORTDIV_SPLIT");
  e.levelwalk_min_units = positive_int("MIFC_LEVELWALK_MIN_UNITS");
  e.slab_graph = not_zero("MIFC_SLAB_GRAPH");
  e.ragged_split = not_zero("MIFC_RAGGED_SPLIT");
  if (const char* s = std::getenv("MIFC_VORTDIV_TUNE")) {
    e.has_vortdiv_tune = true;
    std::strncpy(e.vortdiv_tune, s, sizeof e.vortdiv_tune - 1);
  }
  if (const char* s = std::getenv("MIFC_SCALAR_SPLIT_TUNE"))
    std::strncpy(e.scalar_split_tune, s, sizeof e.scalar_split_tune - 1);
  std::lock_guard<std::mutex> lock(g_env_mutex);
  g_env = e;
}

} // namespace mifc
