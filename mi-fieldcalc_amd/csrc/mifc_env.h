// mifc_env.h -- the tuning / diagnostic environment variables of the library,
// read ONCE (mifc_create, mifc_reload_env) into a process-wide snapshot.  No
// launch path calls getenv: the launchers read this struct.  The variables
// select between code paths that all give the reference's results (A/B
// measurements, tests of every fallback); none of them changes what is computed.
#ifndef MIFC_ENV_H
#define MIFC_ENV_H

namespace mifc {

struct Env
{
  bool force_cell_kernel = false; // MIFC_FORCE_CELL_KERNEL: one-lane-per-cell stencil kernels everywhere
  bool host_pipeline = true;      // MIFC_HOST_PIPELINE=0: stage host-resident level batches whole
  bool fused2 = true;             // MIFC_FUSED2=0: multi-pass thermalFrontParameter / plevelqvector
  bool shapiro_fused = true;      // MIFC_SHAPIRO_FUSED=0: four-launch shapiro2_filter
  bool shapiro_regs = true;       // MIFC_SHAPIRO_REGS=0: the one-launch form with its rows in LDS rings instead of registers
  int ewise_max_blocks = 0;       // MIFC_EWISE_MAX_BLOCKS (> 0 overrides the grid cap of the table kernels)
  int scalar_rows_r = -1;         // MIFC_SCALAR_ROWS_R: -1 unset, 0 = "set, keep the default height", > 0 band height
  int fused2_band = 0;            // MIFC_FUSED2_BAND (> 0 overrides the band height of the fused two-stage kernels)
  int host_threads = 0;           // MIFC_HOST_THREADS (> 0)
  int host_chunk_mib = 0;         // MIFC_HOST_CHUNK_MIB (> 0)
  int host_pipe_min_kib = 0;      // MIFC_HOST_PIPE_MIN_KIB (> 0 replaces the 64 MiB per field from which a host-memory level batch is pipelined; tests)
  int host_chunk_levels = 0;      // MIFC_HOST_CHUNK_LEVELS (> 0: levels per chunk of the host pipeline, before MIFC_HOST_CHUNK_MIB and without the nlev / 4 cap; tests)
  int quantile_chunk_mib = 0;     // MIFC_QUANTILE_CHUNK_MIB (> 0): device staging of a host-memory mifc_ensembleQuantiles call (default 256)
  int ensemble_chunk_mib = 0;     // MIFC_ENSEMBLE_CHUNK_MIB (> 0): device staging of a host-memory mifc_ensemble_levels call (default 256)
  int vinterp_chunk_mib = 0;      // MIFC_VINTERP_CHUNK_MIB (> 0): device staging of a host-memory mifc_vinterp_* call, a band of rows at a time (default 256)
  int vlayer_chunk_mib = 0;       // MIFC_VLAYER_CHUNK_MIB (> 0): device staging of a host-memory mifc_vlayer_* call, a band of rows at a time (default 256)
  int vderiv_chunk_mib = 0;       // MIFC_VDERIV_CHUNK_MIB (> 0): device staging of a host-memory mifc_vderiv_* call, a band of rows at a time (default 256); mifc_vrotate_levels too
  int vcumul_chunk_mib = 0;       // MIFC_VCUMUL_CHUNK_MIB (> 0): device staging of a host-memory mifc_vcumul_* call, a band of rows at a time (default 256)
  int vregrid_chunk_mib = 0;      // MIFC_VREGRID_CHUNK_MIB (> 0): device staging of a host-memory mifc_vregrid_* call, a band of rows at a time (default 256)
  int vregrid_tb = 0;             // MIFC_VREGRID_TB (> 0): target planes per pass of the mifc_vregrid_* kernel, capped at what the form allows (A/B, tools/bench_vregrid.py; the results are the same)
  int vregrid_v = 0;              // MIFC_VREGRID_V=4: the mifc_vregrid_* kernel takes four cells per lane where the batch is on the 16-byte grid (default: one cell per lane everywhere, the faster form; A/B, tools/bench_vregrid.py, tests; the results are the same)
  int vparcel_chunk_mib = 0;      // MIFC_VPARCEL_CHUNK_MIB (> 0): device staging of a host-memory mifc_vparcel_* call, a band of rows at a time (default 256)
  int pvort_chunk_mib = 0;        // MIFC_PVORT_CHUNK_MIB (> 0): device staging of a host-memory mifc_pvort_* call, a band of rows and its neighbour rows at a time (default 256)
  int hinterp_chunk_mib = 0;      // MIFC_HINTERP_CHUNK_MIB (> 0): device staging of a host-memory mifc_hinterp_levels call, whole levels at a time (default 256); mifc_hinterp_vector_levels too
  int hstats_chunk_mib = 0;       // MIFC_HSTATS_CHUNK_MIB (> 0): device staging of a host-memory mifc_hstats_levels call, a band of rows at a time (default 256)
  int hdist_chunk_mib = 0;        // MIFC_HDIST_CHUNK_MIB (> 0): device staging of a host-memory mifc_hdist_* call (bands of rows, chunks of levels) and the digit counters of the selection, a block of levels at a time (default 256)
  bool hdist_aggregate = true;    // MIFC_HDIST_AGGREGATE=0: the counters of the mifc_hdist_* kernels take every lane's runs one by one, without the wave's ballot (A/B, tests; the counts are the same)
  int htraj_chunk_mib = 0;        // MIFC_HTRAJ_CHUNK_MIB (> 0): device staging of a host-memory mifc_htraj_levels call, a chunk of whole levels with two slice buffers and every slot (default 256)
  int htraj_level_chunk = 0;      // MIFC_HTRAJ_LEVEL_CHUNK (> 0 overrides the levels a workgroup of the htraj kernel walks; A/B, tests)
  int hremap_chunk_mib = 0;       // MIFC_HREMAP_CHUNK_MIB (> 0): device staging of a host-memory mifc_hremap_levels call, whole levels at a time (default 256)
  int fexpr_chunk_mib = 0;        // MIFC_FEXPR_CHUNK_MIB (> 0): device staging of a host-memory mifc_fexpr_levels call, a band of rows at a time (default 256)
  int hremap_level_chunk = 0;     // MIFC_HREMAP_LEVEL_CHUNK (> 0 overrides the levels a workgroup of the hremap kernel takes; A/B, tests)
  int hinterp_level_chunk = 0;    // MIFC_HINTERP_LEVEL_CHUNK (> 0 overrides the levels a workgroup of the hinterp and vrotate kernels walks; A/B, tests)
  int derived_blocks = 0;         // MIFC_DERIVED_BLOCKS (> 0 overrides the persistent grid of the fused derived kernel)
  int derived_pipe = 1;           // MIFC_DERIVED_PIPE=0: the fused derived kernel without the two-trip software pipeline (A/B)
  bool levelwalk = true;          // MIFC_VORTDIV_LEVELWALK=0: deep wind batches on the row-walking kernel (A/B)
  bool split_roles = true;        // MIFC_VORTDIV_SPLIT=0: deep batches of the stencil operators on the level-walking kernels whose waves load AND store (A/B)
  int levelwalk_min_units = 0;    // MIFC_LEVELWALK_MIN_UNITS (> 0 overrides the launch size from which the level-walking forms are chosen; tests)
  bool ragged_split = true;       // MIFC_RAGGED_SPLIT=0: widths that are not a multiple of 4 keep the flat four-cells-per-lane kernel for deep batches too (A/B)
  bool slab_graph = true;         // MIFC_SLAB_GRAPH=0: the row-slab step (mifc_slab_plan_step) enqueues its sequence directly instead of replaying a HIP graph
  bool has_vortdiv_tune = false;  // MIFC_VORTDIV_TUNE="R=8,D=1,..."
  char vortdiv_tune[256] = {0};
  char scalar_split_tune[64] = {0}; // MIFC_SCALAR_SPLIT_TUNE="TR=12,NL=2,PF=2,LG=6": shape of the split-role form of the one-input stencil operators (A/B, tests)
};

// the current snapshot (defaults until the first reload)
const Env& env();
// re-reads the process environment into the snapshot
void env_reload();

} // namespace mifc

#endif // MIFC_ENV_H
