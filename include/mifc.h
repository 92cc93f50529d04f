/*
 * mifc.h -- C ABI of the MI355X (gfx950) implementation of the mi-fieldcalc
 * hot path: the elementwise derived-variable operators and the horizontal
 * 5-point-stencil operators of miutil::fieldcalc.
 *
 * This is the drop-in boundary.  The reference has no FFI layer of its own:
 * its operator API is the set of C++ free functions declared in
 * src/mi_fieldcalc/FieldCalculations.h.  Each entry point below replaces one
 * of them (file:line cited per function) with the same argument order
 *   nx, ny, input fields, scalars ("compute" last), output field(s),
 *   fDefined (in/out), undef                      (FieldCalculations.h:102-107)
 * plus a leading context and a trailing `memkind`.  The source-compatible C++
 * header mi-fieldcalc_amd/include/mi_fieldcalc/FieldCalculations.h forwards
 * the original signatures to these; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - fields are row-major float32, index = j*nx + i, x fastest
 *     (FieldCalculations.cc:65-73); batched calls take [nlev][ny][nx]
 *     contiguous, level-major.
 *   - `int* fdefined` carries miutil::ValuesDefined (FieldDefined.h:41) and is
 *     IN/OUT exactly as in the reference: in = state of the inputs
 *     (MIFC_ALL_DEFINED enables the no-test fast path, FieldCalculations.h:47-50),
 *     out = state of the result (FieldDefined.cc:62-70).  Always host memory.
 *   - return value: 1 = success, 0 = the reference's `return false`
 *     (bad sizes / compute / pressure) or a HIP failure; in the latter case
 *     mifc_last_error() is non-empty.  Nothing throws across this boundary.
 *   - memkind says where the FIELD pointers live: MIFC_MEM_HOST (legacy
 *     callers: staged through the context's device scratch, synchronous) or
 *     MIFC_MEM_DEVICE (resident in HBM, no copies; the call still returns
 *     only after the result flag is known).  The *_enqueue variants never
 *     synchronise.
 *   - every operator body is a hand-written HIP kernel; there is no CPU
 *     fallback.  Without a usable gfx950 device mifc_create() returns NULL.
 *   - in-place use (output aliasing an input) is supported for the
 *     elementwise operators only, as in the reference.
 */
#ifndef MIFC_H
#define MIFC_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIFC_ABI_VERSION 1

/* miutil::ValuesDefined, FieldDefined.h:41 */
enum { MIFC_ALL_DEFINED = 0, MIFC_NONE_DEFINED = 1, MIFC_SOME_DEFINED = 2 };
enum { MIFC_MEM_HOST = 0, MIFC_MEM_DEVICE = 1 };

typedef struct mifc_ctx mifc_ctx;

/* ---- context ------------------------------------------------------------ */
int mifc_abi_version(void);
/* number of visible HIP devices (0 when there is no GPU / no driver) */
int mifc_device_count(void);
/* Binds to HIP device `device`; owns a stream, scratch and staging buffers.
 * NULL on failure.  A context may be used from one thread at a time; create
 * one per thread for concurrent callers (the reference is re-entrant). */
mifc_ctx* mifc_create(int device);
void mifc_destroy(mifc_ctx* ctx);
const char* mifc_last_error(const mifc_ctx* ctx);
/* Run subsequent work on a caller-owned hipStream_t, e.g. the PyTorch current
 * stream.  NULL means HIP's null (default) stream -- which is what PyTorch's
 * default stream is.  mifc_use_own_stream() switches back to the context's own
 * non-blocking stream (the initial state). */
/* Switching streams is ordered against work already enqueued on the old stream
 * that still reads context-owned scratch: the new stream waits for it. */
int mifc_set_stream(mifc_ctx* ctx, void* hip_stream);
int mifc_use_own_stream(mifc_ctx* ctx);
int mifc_synchronize(mifc_ctx* ctx);
/* Always returns 0 and leaves "<what>: not built on the GPU (...)" in mifc_last_error(): what the
 * source-compatible C++ API calls for the one reference function it does not forward
 * (neighbourFunctions, until its forwarding line is switched to mifc_neighbourFunctions), so that
 * its `false` can be told from an argument-validation failure. */
int mifc_not_built(mifc_ctx* ctx, const char* what);
/* The library's tuning / diagnostic environment variables (MIFC_*: which of several
 * equivalent kernel forms runs; none changes a result) are read when a context is
 * created, never on a call path.  Re-read them (tests, A/B tools). */
int mifc_reload_env(mifc_ctx* ctx);
/* Device memory for callers that do not link HIP themselves. */
void* mifc_device_alloc(mifc_ctx* ctx, size_t bytes);
int mifc_device_free(mifc_ctx* ctx, void* dptr);
int mifc_copy_to_device(mifc_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int mifc_copy_to_host(mifc_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
/* Device memory for a batch that is allocated once and computed on many times, PLACED: which physical memory the
 * arrays a streaming kernel touches lie on decides its time by up to 12 %, stably for as long as they live (DESIGN.md
 * 4.1).  n_arrays arrays of bytes_each bytes; their addresses come back in arrays_out[n_arrays].
 *   MIFC_PLACE_AS_ALLOCATED  n_arrays plain allocations, as they come
 *   MIFC_PLACE_SEARCH        a pool of up to 48 arrays (never more than budget_bytes, 0 = no budget of the caller's, and
 *                            never more than 90 % of the free device memory) is allocated, index sets of it are timed with
 *                            the probe -- structured and random sets, then coordinate descent, at most 160 probes -- the
 *                            fastest set is kept and the rest freed (what mi-fieldcalc_amd/placement.py does for bench.py)
 *   MIFC_PLACE_VMM           opt-in: ONE physical allocation made and mapped by the library (hipMemCreate / hipMemMap),
 *                            the arrays a measured-good distance apart inside it; no search
 *                            (profiles/r03/experiments/vmm_placement_*.txt, and the caveat in mifc_placement.hip)
 * probe(user, arrays) -> milliseconds of a representative kernel over the candidate arrays, in arrays_out order (a negative
 * value aborts the call); NULL = the library times its own fused vorticity+divergence launch over the first four arrays
 * as (u, v, rvort, diverg) of a nx x ny x nlev batch, which must fit bytes_each.  report may be NULL.
 * Free with mifc_batch_free_placed (all arrays of one call together). */
enum { MIFC_PLACE_AS_ALLOCATED = 0, MIFC_PLACE_SEARCH = 1, MIFC_PLACE_VMM = 2 };
typedef float (*mifc_placement_probe_fn)(void* user, void* const* arrays);
typedef struct mifc_placement_report {
  int strategy, pool_size, probes;
  float as_allocated_ms; /* the first n_arrays arrays of the pool: what allocating the batch in one go gives */
  float chosen_ms, probe_ms_min, probe_ms_median, probe_ms_max;
  size_t array_distance_bytes; /* MIFC_PLACE_VMM: distance between the arrays inside the one allocation */
} mifc_placement_report;
int mifc_batch_alloc_placed(mifc_ctx* ctx, int n_arrays, size_t bytes_each, int strategy, size_t budget_bytes, int nx, int ny, int nlev,
                            mifc_placement_probe_fn probe, void* probe_user, void** arrays_out, mifc_placement_report* report);
int mifc_batch_free_placed(mifc_ctx* ctx, void** arrays, int n_arrays);
/* Host-pointer (MIFC_MEM_HOST) callers: declare a host array that is passed to
 * many calls unchanged -- xmapr, ymapr, fcoriolis of a grid (FieldCalculations.h:
 * every stencil operator takes them) -- so that it is uploaded once instead of
 * per call.  The content must not change while held; hold again to refresh,
 * release before freeing the array.  No counterpart in the reference, whose
 * operators read the caller's memory directly. */
int mifc_hold_field(mifc_ctx* ctx, const float* host_field, size_t n_floats);
int mifc_release_field(mifc_ctx* ctx, const float* host_field);
/* The asynchronous entry points zero the caller's undefined counters before they count (one small fill per call).
 * A caller that issues many small calls back to back -- or records them into a graph, where every fill is a node of
 * ~5 us -- can zero ALL its counters with one mifc_zero_counts_enqueue and switch the per-call fills off:
 * mifc_counts_accumulate(ctx, 1) makes mifc_stencil_levels_enqueue, mifc_vortdiv_levels*_enqueue and
 * mifc_hlevel_derived_*_enqueue ADD to the counters they are given (0 switches back; the synchronous entries and the
 * slab plans are not affected). */
int mifc_counts_accumulate(mifc_ctx* ctx, int on);
int mifc_zero_counts_enqueue(mifc_ctx* ctx, unsigned long long* counts_dev, size_t n);
/* miutil::checkDefined(size_t,size_t), FieldDefined.cc:62-70 */
int mifc_classify(unsigned long long n_undefined, unsigned long long n);

/* ---- elementwise, one field per call ------------------------------------ */
/* miutil::fieldcalc::vectorabs, FieldCalculations.h:204 / FieldCalculations.cc:1819 */
int mifc_vectorabs(mifc_ctx* ctx, int nx, int ny, const float* u, const float* v, float* ff, int* fdefined, float undef, int memkind);
/* pleveltemp FieldCalculations.h:113 / .cc:328; hleveltemp .h:154 / .cc:1046; aleveltemp .h:172 / .cc:1310 */
int mifc_pleveltemp(mifc_ctx* ctx, int nx, int ny, const float* tinp, float p, const char* unit, int compute, float* tout, int* fdefined,
                    float undef, int memkind);
int mifc_hleveltemp(mifc_ctx* ctx, int nx, int ny, const float* tinp, const float* ps, float alevel, float blevel, const char* unit, int compute,
                    float* tout, int* fdefined, float undef, int memkind);
int mifc_aleveltemp(mifc_ctx* ctx, int nx, int ny, const float* tinp, const float* p, const char* unit, int compute, float* tout, int* fdefined,
                    float undef, int memkind);
/* plevelhum FieldCalculations.h:117 / .cc:400; hlevelhum .h:160 / .cc:1145; alevelhum .h:176 / .cc:1394; cvhum .h:200 / .cc:1738 */
int mifc_plevelhum(mifc_ctx* ctx, int nx, int ny, const float* t, const float* huminp, float p, const char* unit, int compute, float* humout,
                   int* fdefined, float undef, int memkind);
int mifc_hlevelhum(mifc_ctx* ctx, int nx, int ny, const float* t, const float* huminp, const float* ps, float alevel, float blevel,
                   const char* unit, int compute, float* humout, int* fdefined, float undef, int memkind);
int mifc_alevelhum(mifc_ctx* ctx, int nx, int ny, const float* t, const float* huminp, const float* p, const char* unit, int compute,
                   float* humout, int* fdefined, float undef, int memkind);
int mifc_cvhum(mifc_ctx* ctx, int nx, int ny, const float* t, const float* huminp, const char* unit, int compute, float* humout, int* fdefined,
               float undef, int memkind);

/* ---- 5-point stencils, one field per call ------------------------------- */
/* relvort FieldCalculations.h:206 / .cc:1843; absvort .h:208 / .cc:1875; divergence .h:211 / .cc:1910 */
int mifc_relvort(mifc_ctx* ctx, int nx, int ny, const float* u, const float* v, const float* xmapr, const float* ymapr, float* rvort,
                 int* fdefined, float undef, int memkind);
int mifc_absvort(mifc_ctx* ctx, int nx, int ny, const float* u, const float* v, const float* xmapr, const float* ymapr, const float* fcoriolis,
                 float* avort, int* fdefined, float undef, int memkind);
int mifc_divergence(mifc_ctx* ctx, int nx, int ny, const float* u, const float* v, const float* xmapr, const float* ymapr, float* diverg,
                    int* fdefined, float undef, int memkind);
/* gradient FieldCalculations.h:216 / .cc:1985 (compute 1..4) */
int mifc_gradient(mifc_ctx* ctx, int nx, int ny, const float* field, const float* xmapr, const float* ymapr, int compute, float* fgrad,
                  int* fdefined, float undef, int memkind);
/* plevelgwind_xcomp .h:127 / .cc:638; plevelgwind_ycomp .h:130 / .cc:674; plevelgvort .h:133 / .cc:708 */
int mifc_plevelgwind_xcomp(mifc_ctx* ctx, int nx, int ny, const float* z, const float* xmapr, const float* ymapr, const float* fcoriolis, float* ug,
                           int* fdefined, float undef, int memkind);
int mifc_plevelgwind_ycomp(mifc_ctx* ctx, int nx, int ny, const float* z, const float* xmapr, const float* ymapr, const float* fcoriolis, float* vg,
                           int* fdefined, float undef, int memkind);
int mifc_plevelgvort(mifc_ctx* ctx, int nx, int ny, const float* z, const float* xmapr, const float* ymapr, const float* fcoriolis, float* gvort,
                     int* fdefined, float undef, int memkind);
/* ilevelgwind FieldCalculations.h:185 / .cc:1511 */
int mifc_ilevelgwind(mifc_ctx* ctx, int nx, int ny, const float* mpot, const float* xmapr, const float* ymapr, const float* fcoriolis, float* ug,
                     float* vg, int* fdefined, float undef, int memkind);

/* ---- next operators of the same family, one field per call -- */
/* advection FieldCalculations.h:213 / .cc:1942; jacobian .h:235 / .cc:2424 */
int mifc_advection(mifc_ctx* ctx, int nx, int ny, const float* f, const float* u, const float* v, const float* xmapr, const float* ymapr, float hours,
                   float* advec, int* fdefined, float undef, int memkind);
int mifc_jacobian(mifc_ctx* ctx, int nx, int ny, const float* field1, const float* field2, const float* xmapr, const float* ymapr, float* fjacobian,
                  int* fdefined, float undef, int memkind);
/* momentumXcoordinate .h:229 / .cc:2351; momentumYcoordinate .h:232 / .cc:2387 (pointwise) */
int mifc_momentumXcoordinate(mifc_ctx* ctx, int nx, int ny, const float* v, const float* xmapr, const float* fcoriolis, float fcoriolisMin, float* mxy,
                             int* fdefined, float undef, int memkind);
int mifc_momentumYcoordinate(mifc_ctx* ctx, int nx, int ny, const float* u, const float* ymapr, const float* fcoriolis, float fcoriolisMin, float* nxy,
                             int* fdefined, float undef, int memkind);
/* thermalFrontParameter .h:225 / .cc:2266 (two passes: |grad T|, then the front parameter) */
int mifc_thermalFrontParameter(mifc_ctx* ctx, int nx, int ny, const float* tx, const float* xmapr, const float* ymapr, float* tfp, int* fdefined,
                               float undef, int memkind);
/* plevelqvector .h:122 / .cc:505 (three passes: geostrophic wind x, y, then the Q-vector component;
 * compute 1/2 = x component from T / theta, 3/4 = y component) */
int mifc_plevelqvector(mifc_ctx* ctx, int nx, int ny, const float* z, const float* t, const float* xmapr, const float* ymapr,
                       const float* fcoriolis, float p, int compute, float* qcomp, int* fdefined, float undef, int memkind);

/* ---- the rest of the pointwise catalogue, one field per call ----
 * Each entry replaces the miutil::fieldcalc function of the same name; the
 * comment gives FieldCalculations.h:line / FieldCalculations.cc:line.  Argument
 * order is the reference's (fieldOPER* take `compute` first, like there).  The
 * reference's void functions return 1 here. */
/* plevelthe .h:115 / .cc:369; hlevelthe .h:157 / .cc:1100; alevelthe .h:174 / .cc:1355 */
int mifc_plevelthe(mifc_ctx* ctx, int nx, int ny, const float* t, const float* rh, float p, int compute, float* the, int* fdefined, float undef,
                   int memkind);
int mifc_hlevelthe(mifc_ctx* ctx, int nx, int ny, const float* t, const float* q, const float* ps, float alevel, float blevel, int compute,
                   float* the, int* fdefined, float undef, int memkind);
int mifc_alevelthe(mifc_ctx* ctx, int nx, int ny, const float* t, const float* q, const float* p, int compute, float* the, int* fdefined, float undef,
                   int memkind);
/* plevelducting .h:125 / .cc:597; hlevelducting .h:163 / .cc:1219; alevelducting .h:179 / .cc:1460 */
int mifc_plevelducting(mifc_ctx* ctx, int nx, int ny, const float* t, const float* h, float p, int compute, float* duct, int* fdefined, float undef,
                       int memkind);
int mifc_hlevelducting(mifc_ctx* ctx, int nx, int ny, const float* t, const float* h, const float* ps, float alevel, float blevel, int compute,
                       float* duct, int* fdefined, float undef, int memkind);
int mifc_alevelducting(mifc_ctx* ctx, int nx, int ny, const float* t, const float* h, const float* p, int compute, float* duct, int* fdefined,
                       float undef, int memkind);
/* hlevelpressure .h:166 / .cc:1276; pleveldz2tmean .h:120 / .cc:466 */
int mifc_hlevelpressure(mifc_ctx* ctx, int nx, int ny, const float* ps, float alevel, float blevel, float* p, int* fdefined, float undef,
                        int memkind);
int mifc_pleveldz2tmean(mifc_ctx* ctx, int nx, int ny, const float* z1, const float* z2, float p1, float p2, int compute, float* tmean,
                        int* fdefined, float undef, int memkind);
/* kIndex .h:136 / .cc:745; ductingIndex .h:139 / .cc:816; showalterIndex .h:141 / .cc:872; boydenIndex .h:144 / .cc:973; sweatIndex .h:147 / .cc:1016 */
int mifc_kIndex(mifc_ctx* ctx, int nx, int ny, const float* t500, const float* t700, const float* rh700, const float* t850, const float* rh850,
                float p500, float p700, float p850, int compute, float* kfield, int* fdefined, float undef, int memkind);
int mifc_ductingIndex(mifc_ctx* ctx, int nx, int ny, const float* t850, const float* rh850, float p850, int compute, float* duct, int* fdefined,
                      float undef, int memkind);
int mifc_showalterIndex(mifc_ctx* ctx, int nx, int ny, const float* t500, const float* t850, const float* rh850, float p500, float p850, int compute,
                        float* sfield, int* fdefined, float undef, int memkind);
int mifc_boydenIndex(mifc_ctx* ctx, int nx, int ny, const float* t700, const float* z700, const float* z1000, float p700, float p1000, int compute,
                     float* bfield, int* fdefined, float undef, int memkind);
int mifc_sweatIndex(mifc_ctx* ctx, int nx, int ny, const float* t850, const float* t500, const float* td850, const float* td500, const float* u850,
                    const float* v850, const float* u500, const float* v500, float* sindex, int* fdefined, float undef, int memkind);
/* seaSoundSpeed .h:192 / .cc:1555; cvtemp .h:198 / .cc:1608; abshum .h:202 / .cc:1676; windCooling .h:220 / .cc:2181;
 * underCooledRain .h:222 / .cc:2231; pressure2FlightLevel .h:227 / .cc:2311; snow_in_cm .h:303 / .cc:3063 */
int mifc_seaSoundSpeed(mifc_ctx* ctx, int nx, int ny, const float* t, const float* s, float z, int compute, float* soundspeed, int* fdefined,
                       float undef, int memkind);
int mifc_cvtemp(mifc_ctx* ctx, int nx, int ny, const float* tinp, int compute, float* tout, int* fdefined, float undef, int memkind);
int mifc_abshum(mifc_ctx* ctx, int nx, int ny, const float* t, const float* rhum, float* abshumout, int* fdefined, float undef, int memkind);
int mifc_windCooling(mifc_ctx* ctx, int nx, int ny, const float* t, const float* u, const float* v, int compute, float* dtcool, int* fdefined,
                     float undef, int memkind);
int mifc_underCooledRain(mifc_ctx* ctx, int nx, int ny, const float* precip, const float* snow, const float* tk, float precipMin, float snowRateMax,
                         float tcMax, float* undercooled, int* fdefined, float undef, int memkind);
int mifc_pressure2FlightLevel(mifc_ctx* ctx, int nx, int ny, const float* pressure, float* flightlevel, int* fdefined, float undef, int memkind);
int mifc_snow_in_cm(mifc_ctx* ctx, int nx, int ny, const float* snow_water, const float* tk2m, const float* td2m, float* snow_cm, int* fdefined,
                    float undef, int memkind);
/* values2classes .h:252 / .cc:2462: `values` (class limits, std::vector<float> there) is always a HOST array */
int mifc_values2classes(mifc_ctx* ctx, int nx, int ny, const float* fvalue, float* fclass, const float* values, int nvalues, int* fdefined,
                        float undef, int memkind);
/* shapiro2_filter .h:218 / .cc:2076 (second-order Shapiro filter, four sweeps; field == fsmooth allowed,
 * the flag always becomes ALL_DEFINED) */
int mifc_shapiro2_filter(mifc_ctx* ctx, int nx, int ny, const float* field, float* fsmooth, int* fdefined, float undef, int memkind);
/* vesselIcingOverland .h:238 / FieldCalculationsVesselIcing.cc:77; vesselIcingMertins .h:241 / :114
 * (the two iterative models, vesselIcingModStall and vesselIcingMincog, follow below) */
int mifc_vesselIcingOverland(mifc_ctx* ctx, int nx, int ny, const float* airtemp, const float* seatemp, const float* u, const float* v,
                             const float* sal, const float* aice, float* icing, int* fdefined, float undef, int memkind);
int mifc_vesselIcingMertins(mifc_ctx* ctx, int nx, int ny, const float* airtemp, const float* seatemp, const float* u, const float* v,
                            const float* sal, const float* aice, float* icing, int* fdefined, float undef, int memkind);
/* field algebra .h:254-282 / .cc:2501-2669 */
int mifc_minvalueFields(mifc_ctx* ctx, int nx, int ny, const float* field1, const float* field2, float* fres, int* fdefined, float undef, int memkind);
int mifc_maxvalueFields(mifc_ctx* ctx, int nx, int ny, const float* field1, const float* field2, float* fres, int* fdefined, float undef, int memkind);
int mifc_minvalueFieldConst(mifc_ctx* ctx, int nx, int ny, const float* field1, float value, float* fres, int* fdefined, float undef, int memkind);
int mifc_maxvalueFieldConst(mifc_ctx* ctx, int nx, int ny, const float* field1, float value, float* fres, int* fdefined, float undef, int memkind);
int mifc_absvalueField(mifc_ctx* ctx, int nx, int ny, const float* field, float* fres, int* fdefined, float undef, int memkind);
int mifc_log10Field(mifc_ctx* ctx, int nx, int ny, const float* field, float* fres, int* fdefined, float undef, int memkind);
int mifc_pow10Field(mifc_ctx* ctx, int nx, int ny, const float* field, float* fres, int* fdefined, float undef, int memkind);
int mifc_logField(mifc_ctx* ctx, int nx, int ny, const float* field, float* fres, int* fdefined, float undef, int memkind);
int mifc_expField(mifc_ctx* ctx, int nx, int ny, const float* field, float* fres, int* fdefined, float undef, int memkind);
int mifc_powerField(mifc_ctx* ctx, int nx, int ny, const float* field, float value, float* fres, int* fdefined, float undef, int memkind);
int mifc_replaceUndefined(mifc_ctx* ctx, int nx, int ny, const float* field, float value, float* fres, int* fdefined, float undef, int memkind);
int mifc_replaceDefined(mifc_ctx* ctx, int nx, int ny, const float* field, float value, float* fres, int* fdefined, float undef, int memkind);
int mifc_fieldOPERfield(mifc_ctx* ctx, int compute, int nx, int ny, const float* field1, const float* field2, float* fres, int* fdefined, float undef,
                        int memkind);
int mifc_fieldOPERconstant(mifc_ctx* ctx, int compute, int nx, int ny, const float* field, float value, float* fres, int* fdefined, float undef,
                           int memkind);
int mifc_constantOPERfield(mifc_ctx* ctx, int compute, int nx, int ny, float value, const float* field, float* fres, int* fdefined, float undef,
                           int memkind);

/* ---- EXTENSION, NOT part of miutil::fieldcalc ------------------------------------------------
 * BASELINE.json's north_star names "wind speed/direction from u/v"; the reference has the speed
 * (vectorabs) but no direction function (FieldCalculations.cc:1951-1952 mention it in a comment
 * only), so there is no reference result to be identical to.  Defined here as the meteorological
 * direction the wind blows FROM, degrees clockwise from north, in [0, 360):
 *   dd = 270 - atan2(v, u) * 180 / pi   (calm: 0),   undefined where u or v is undefined,
 * with the flag handling of vectorabs (.cc:1819-1841).  Parity is against this definition only. */
int mifc_winddir(mifc_ctx* ctx, int nx, int ny, const float* u, const float* v, float* dd, int* fdefined, float undef, int memkind);

/* ---- reductions over ensemble members ---------------------
 * sumFields .h:284 / .cc:2671; meanValue .h:286 / .cc:2696; stddevValue .h:289 / .cc:2726;
 * extremeValue .h:292 / .cc:2759; probability .h:294 / .cc:2807.
 * The reference takes std::vector<float*> fields, std::vector<ValuesDefined>
 * fDefinedIn and std::vector<float> limits; here `fields` is a HOST array of
 * nfields pointers (each a host or a device field according to memkind),
 * `fdefined_in` a HOST int array of nfields flags, `limits` a HOST array.
 * Members are reduced in index order, like the reference's inner loop. */
int mifc_sumFields(mifc_ctx* ctx, int nx, int ny, const float* const* fields, int nfields, float* fres, int* fdefined, float undef, int memkind);
int mifc_meanValue(mifc_ctx* ctx, int nx, int ny, const float* const* fields, const int* fdefined_in, int nfields, float* fres, int* fdefined_out,
                   float undef, int memkind);
int mifc_stddevValue(mifc_ctx* ctx, int nx, int ny, const float* const* fields, const int* fdefined_in, int nfields, float* fres,
                     int* fdefined_out, float undef, int memkind);
int mifc_extremeValue(mifc_ctx* ctx, int compute, int nx, int ny, const float* const* fields, int nfields, float* fres, int* fdefined, float undef,
                      int memkind);
int mifc_probability(mifc_ctx* ctx, int compute, int nx, int ny, const float* const* fields, const int* fdefined_in, int nfields,
                     const float* limits, int nlimits, float* fres, int* fdefined_out, float undef, int memkind);

/* ---- the ensemble reductions over a level batch, several in one pass over the members -----------------------
 * The five functions above for nmem members of [nlev][ny][nx] each and a list of products: for every level l and product
 * k, products[k].out[l] and products[k].fdefined[l] are bit for bit what the single-field function of products[k].stat
 * returns for level l of the members, its quirks included (members reduced in index order; sumFields stops at the first
 * undefined member; Welford in float; sqrt in double; probability tests != undef only and leaves out the members flagged
 * NONE_DEFINED; the index variants of extremeValue store (float)j).  Every member is read once per call, whatever the
 * number of products.
 *   `fields` is a HOST array of nmem pointers, each to [nlev][ny][nx]; `fdefined_in` a HOST int[nmem * nlev], member-major
 *   (j * nlev + l), NULL = all SOME_DEFINED: the reference's fDefinedIn[j] of meanValue, stddevValue and probability.
 *   `products` is a HOST array.  sumFields and extremeValue take ONE in/out flag in the reference: here that is
 *   products[k].fdefined[l], on input the state of that level's members (ALL_DEFINED switches the per-cell tests off), on
 *   output the result flag.  For the other statistics products[k].fdefined[l] is output only.
 * One list holds at most one SUM, one MEAN, one STDDEV, one EXTREME per compute 1..4 and eight PROBABILITY products.
 * Refused calls return 0, write nothing and give the reason in mifc_last_error().  They are: nproducts < 1 or a list past
 * these limits; an unknown stat; EXTREME compute outside 1..4; PROBABILITY compute outside 1..6, nlimits outside 1..2, or
 * compute 3 / 6 with one limit (the reference returns false); EXTREME with nmem == 0 (likewise); nlev < 1, or a negative
 * nx, ny or nmem; a null pointer; an output that overlaps another output or a member; a call made while a mifc_graph
 * capture is open.  nmem == 0 with the other statistics gives what the reference gives for an empty vector.
 * memkind works as everywhere else; host memory works at any size: the call stages a bounded chunk of levels (or of one
 * level's cells) at a time, MIFC_ENSEMBLE_CHUNK_MIB of device memory (default 256).  DESIGN.md 4.14. */
enum { MIFC_ENS_SUM = 0, MIFC_ENS_MEAN = 1, MIFC_ENS_STDDEV = 2, MIFC_ENS_EXTREME = 3, MIFC_ENS_PROBABILITY = 4 };
typedef struct mifc_ens_product {
  int stat;        /* MIFC_ENS_* */
  int compute;     /* EXTREME 1..4, PROBABILITY 1..6 (the reference's numbering); ignored otherwise */
  float limits[2]; /* PROBABILITY */
  int nlimits;     /* PROBABILITY: 1 or 2 */
  float* out;      /* [nlev][ny][nx], host or device per memkind */
  int* fdefined;   /* HOST int[nlev]; see above */
} mifc_ens_product;
int mifc_ensemble_levels(mifc_ctx* ctx, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nmem,
                         const mifc_ens_product* products, int nproducts, float undef, int memkind);

/* ---- EXTENSION: percentiles across ensemble members ---------------------------------------------------------
 * Not a miutil::fieldcalc function; the reference's rule for choosing a percentile is neighbourFunctions compute 4
 * (FieldCalculations.cc:2955-3061).  Inputs are nmem members.  Each member is a [nlev][ny][nx] float field, with one
 * input flag per member and level.  For each level l and cell i:
 *   1. Defined members.  Member j counts at (l, i) under exactly meanValue's rule (FieldCalculations.cc:2710):
 *      is_defined(flag[j][l] == ALL_DEFINED, x, undef).  A member flagged ALL_DEFINED is taken at its word.  Let n be
 *      the number of members that count.
 *   2. If n == 0, every output at that cell is undef.
 *   3. Order.  The counted values are sorted ascending in IEEE total order: -inf < ... < -0 < +0 < ... < +inf.  Every
 *      NaN (which can only reach the sort through an ALL_DEFINED member) sorts above +inf, and the result is then some
 *      NaN (payload free).  The order is independent of member order, so the result does not depend on which member
 *      holds which value.
 *   4. Percentile p is a float in [0, 100].  The two methods are:
 *      * MIFC_QUANTILE_LOWER = 0, the reference's neighbourFunctions rule.  ii = (int)(((float)n * p) / 100.0f), all
 *        in float, truncated.  It is clamped to n - 1, so p = 100 gives the maximum instead of the reference's
 *        out-of-range read.  The result is x[ii], the stored value bit for bit.
 *      * MIFC_QUANTILE_LINEAR = 1, numpy's default "linear" method (Hyndman-Fan type 7) with fixed arithmetic.  All
 *        steps are in double, each rounded, with no contraction: h = ((double)(n - 1) * (double)p) / 100.0,
 *        k = (int)h, t = h - k.  If t == 0 the result is x[k] bit for bit.  Otherwise it is
 *        (float)(x[k] + t * (x[k+1] - x[k])), with both x values widened to double.
 *   5. Output flags.  fdefined_out[l] = checkDefined(#cells with n == 0, nx*ny).  This is by construction the flag
 *      meanValue returns on the same level and member flags.
 * Special cases:
 *   * nmem == 0 behaves like meanValue with no fields: all outputs undef, flags NONE_DEFINED, return 1.
 *   * Refused calls return 0, write nothing and give the reason in mifc_last_error().  They are: an unknown method;
 *     nq < 1; a p that is NaN or outside [0, 100]; nlev < 1, or a negative nx, ny or nmem; a null pointer; two outputs
 *     that are the same array (or overlap); a call made while a mifc_graph capture is open.
 *   * An output may be exactly one of the member arrays (in-place).  Each cell reads only its own index.
 * Arguments follow the ensemble reductions above: `fields` is a HOST array of nmem pointers, each pointing to
 * [nlev][ny][nx]; `fdefined_in` a HOST int[nmem * nlev], member-major (j * nlev + l), NULL = all SOME_DEFINED;
 * `percentiles` a HOST float[nq]; `fres` a HOST array of nq output pointers, each pointing to [nlev][ny][nx];
 * `fdefined_out` a HOST int[nlev].  memkind works as everywhere else; host memory works at any size: the call stages a
 * bounded chunk of levels (or of one level's cells) at a time, MIFC_QUANTILE_CHUNK_MIB of device memory (default 256).
 * Sorting network in registers up to 64 members, an exact bisection over the keys above. */
enum { MIFC_QUANTILE_LOWER = 0, MIFC_QUANTILE_LINEAR = 1 };
int mifc_ensembleQuantiles(mifc_ctx* ctx, int method, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nmem,
                           const float* percentiles, int nq, float* const* fres, int* fdefined_out, float undef, int memkind);

/* mifc_last_ensemble_form: the launch shape of the calling thread's last successful call of mifc_sumFields, mifc_meanValue,
 * mifc_stddevValue, mifc_extremeValue, mifc_probability, mifc_ensemble_levels or mifc_ensembleQuantiles, a diagnostic for
 * tests ("" before the first; a refused call and a call on no cells leave it as it was):
 *   "entry=single c=4|1 tail=0|1 ..."                         c: cells per lane; tail: the 16-byte launch was followed by
 *                                                             the scalar launch for the last n % 4 cells
 *   "entry=levels c=4|1 welford=0|1 flagged=0|1 np=0|3|8 ..."  the template arguments of the kernel instance that ran (a
 *                                                             list of stddev and one to three probabilities reports
 *                                                             flagged=1; c=1 is the one scalar instance, 1 1 8)
 *   "entry=quantiles tier=8|16|32|64|0 ..."                   the sorting network's capacity, 0: the bisection
 * each followed by "inline=1|0 launches=<n> lev_chunk=<levels> cell_chunk=<cells> partials=0|1": kernel arguments (1) or
 * device table (0); the kernel launches of the call, one per staged chunk (two for single with tail=1); the staging plan
 * (for single 1 and nx * ny); whether the undefined counts went through the per-workgroup table.  Where a call staged
 * several chunks, c, the template arguments and partials are those of its first launch. */
const char* mifc_last_ensemble_form(void);

/* ---- EXTENSION: interpolation of level batches to constant surfaces ------------------------------------------
 * Not a miutil::fieldcalc function: the reference leaves the step from model levels to the pressure (or height, or
 * isentropic) surfaces its plevel* / ilevel* operators work on to its caller.  nfields fields of [nlev][ny][nx] and one
 * coordinate per level and cell go in, nfields fields of [ntargets][ny][nx] come out.  For each cell i and target t,
 * ct = targets[t]:
 *   1. Coordinate.  mifc_vinterp_hlevels: c_k = alevel[k] + blevel[k] * ps[i], evaluated in float exactly like the
 *      reference's p_hlevel (FieldCalculations.cc:303): float product, then float sum, no contraction; every c_k of the
 *      cell is defined where is_defined(fdef_ps == ALL_DEFINED, ps[i], undef).  mifc_vinterp_fields: c_k = coord[k][i],
 *      defined where is_defined(fdef_coord[k] == ALL_DEFINED, c_k, undef).
 *   2. Bracket.  The first k in index order, 0 <= k < nlev - 1, with c_k and c_{k+1} both defined and
 *      min(c_k, c_{k+1}) <= ct <= max(c_k, c_{k+1}).  No monotonicity and no level order (top-down, bottom-up) is
 *      assumed.  A NaN coordinate (which can only get in through an ALL_DEFINED flag) fails both comparisons and never
 *      brackets.  Without a bracket every field is undef at (t, i): above the top, below the ground.
 *   3. Values.  Field f needs x_k and x_{k+1} defined, each under is_defined(fdefined_in[f * nlev + level] ==
 *      ALL_DEFINED, x, undef); otherwise its result is undef.
 *   4. MIFC_VINTERP_LOG with min(c_k, c_{k+1}) <= 0 at the bracket: undef.
 *   5. c_k == c_{k+1}: the result is x_k bit for bit, nothing is divided.
 *   6. Otherwise the weight, in double, every operation rounded on its own (no contraction):
 *      MIFC_VINTERP_LINEAR = 0: w = ((double)ct - (double)c_k) / ((double)c_{k+1} - (double)c_k);
 *      MIFC_VINTERP_LOG = 1: the same with log() of each of the three values, in double;
 *      and the result is (float)((double)x_k + w * ((double)x_{k+1} - (double)x_k)).
 *   7. Flags.  fdefined_out[f * ntargets + t] = checkDefined(cells that rules 2 to 4 left undef, nx * ny).
 * LINEAR is bit for bit this definition.  LOG depends on the device's double log(): a result is the definition's
 * float or its neighbour (the weight is off by a few ulp of double at most), undef cells and flags are exact.
 * Arguments: `fields` is a HOST array of nfields pointers, each to [nlev][ny][nx]; `fdefined_in` a HOST
 * int[nfields * nlev], field-major (f * nlev + k), NULL = all SOME_DEFINED; `alevel`, `blevel` (HOST float[nlev]) and
 * `targets` (HOST float[ntargets]) are host arrays; `ps` is [ny][nx], `coord` [nlev][ny][nx], `fdef_coord` a HOST
 * int[nlev], NULL = all SOME_DEFINED; `fres` is a HOST array of nfields pointers, each to [ntargets][ny][nx];
 * `fdefined_out` a HOST int[nfields * ntargets], field-major (f * ntargets + t).
 * Refused calls return 0, write nothing and give the reason in mifc_last_error().  They are: nlev < 2; nfields outside
 * 1..8; ntargets outside 1..64; a negative nx or ny; a null pointer; an unknown method; a NaN target; LOG with a target
 * <= 0; hybrid form only: a level whose (alevel, blevel) the reference's bad_hlevel (FieldCalculations.cc:298) rejects;
 * an output that overlaps an input, the coordinate, ps or another output; a call made while a mifc_graph capture is open.
 * memkind works as everywhere else; host memory works at any size: columns are independent, so the call stages a band of
 * rows at a time, MIFC_VINTERP_CHUNK_MIB of device memory (default 256).  Every input level is read once per 32
 * targets. */
enum { MIFC_VINTERP_LINEAR = 0, MIFC_VINTERP_LOG = 1 };
int mifc_vinterp_hlevels(mifc_ctx* ctx, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields,
                         const float* ps, int fdef_ps, const float* alevel, const float* blevel, const float* targets, int ntargets,
                         int method, float* const* fres, int* fdefined_out, float undef, int memkind);
int mifc_vinterp_fields(mifc_ctx* ctx, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields,
                        const float* coord, const int* fdef_coord /* HOST int[nlev], NULL = SOME_DEFINED */, const float* targets,
                        int ntargets, int method, float* const* fres, int* fdefined_out, float undef, int memkind);

/* ---- EXTENSION: interpolation of level batches to per-cell target surfaces -----------------------------------
 * Not a miutil::fieldcalc function.  mifc_vinterp_* above takes a level batch to surfaces that are one number for the
 * whole grid; here the target is a plane: the hybrid levels of another model or orography (a2 + b2 * ps2), a
 * terrain-following height set, the LCL pressure of mifc_vparcel_*, the COORD_OF_MAX of mifc_vlayer_*, ps - 30 hPa.
 * nfields fields of [nlev][ny][nx], one coordinate per level and cell and ntargets target planes go in, nfields fields
 * of [ntargets][ny][nx] come out.  For each cell i and target t:
 *   1. Source coordinate.  c_k exactly as rule 1 of mifc_vinterp_* gives it (mifc_vregrid_hlevels: the float product,
 *      then the float sum, defined where ps[i] is; mifc_vregrid_fields: coord[k][i], defined under fdef_coord[k]).
 *      mifc_vregrid_levels: c_k = levels[k] for every cell, always defined, bit for bit (a level of -0 stays -0: its
 *      sign reaches the result through the weight of rule 4).
 *   2. Target.  ct = tcoord[t][i] is usable when is_defined(fdef_tcoord[t] == ALL_DEFINED, ct, undef) holds and ct is
 *      not NaN; with MIFC_VINTERP_LOG it must also be > 0.  Otherwise every field is undef at (t, i): a result, not a
 *      refusal.
 *   3. Bracket.  Of the k, 0 <= k < nlev - 1, with c_k and c_{k+1} both defined and
 *      min(c_k, c_{k+1}) <= ct <= max(c_k, c_{k+1}), MIFC_VREGRID_FROM_FIRST = 0 takes the smallest and
 *      MIFC_VREGRID_FROM_LAST = 1 the largest.  The comparisons are float comparisons (-0 == +0; a NaN coordinate never
 *      brackets).  No monotonicity and no level order is assumed.
 *   4. Values, weight, result.  Rules 3 to 6 of mifc_vinterp_* word for word, on the pair (k, k + 1) in that
 *      orientation whichever way the levels are searched: x_k and x_{k+1} defined under their flags, else undef;
 *      MIFC_VINTERP_LOG with min(c_k, c_{k+1}) <= 0 at the bracket: undef; c_k == c_{k+1}: x_k bit for bit; otherwise
 *      w in double from ct, c_k, c_{k+1} (MIFC_VINTERP_LOG: from the log() of each, all three taken in double per
 *      cell) and (float)((double)x_k + w * ((double)x_{k+1} - (double)x_k)).
 *   5. No bracket.  MIFC_VREGRID_OUTSIDE_UNDEF = 0: undef.  MIFC_VREGRID_OUTSIDE_CLAMP = 1: over the levels of the cell
 *      whose coordinate is defined and not NaN, kmin is the lowest index that attains the smallest coordinate and kmax
 *      the lowest index that attains the largest.  ct < c_kmin gives x_kmin, ct > c_kmax gives x_kmax, each copied bit
 *      for bit without arithmetic (also with MIFC_VINTERP_LOG), undef where that value is undefined under its level's
 *      flag.  Anything else -- a ct inside the range that holes left without a bracket, a cell without a usable level
 *      -- is undef.
 *   6. Flags.  fdefined_out[f * ntargets + t] = checkDefined(cells that rules 2 to 5 left undef, nx * ny).  A computed
 *      NaN or infinity is a value: not counted.
 * MIFC_VINTERP_LINEAR is bit for bit this definition (restated in numpy in tests/vregrid_restate.py).
 * MIFC_VINTERP_LOG depends on the device's double log(): a result is the definition's float or its neighbour, undef
 * cells and flags are exact -- the statement mifc_vinterp_* makes.
 * Arguments: `fields`, `fdefined_in`, `ps`, `alevel`, `blevel`, `coord`, `fdef_coord`, `fres` as for mifc_vinterp_*,
 * nfields 1..8; `levels` a HOST float[nlev]; `tcoord` is [ntargets][ny][nx] in the memory kind of the fields,
 * `fdef_tcoord` a HOST int[ntargets], NULL = all SOME_DEFINED; ntargets 1..256; `method` MIFC_VINTERP_LINEAR or
 * MIFC_VINTERP_LOG; `fdefined_out` a HOST int[nfields * ntargets], field-major.
 * Refused calls return 0, write nothing and give the reason in mifc_last_error().  They are: nlev < 2; nfields outside
 * 1..8; ntargets outside 1..256; a negative nx or ny; a null pointer (fdefined_in, fdef_coord and fdef_tcoord may be
 * null); an unknown method, from or outside; a NaN in levels; hybrid form only: a level that the reference's bad_hlevel
 * (FieldCalculations.cc:298) rejects; an output that overlaps an input, the coordinate, ps, tcoord or another output; a
 * call made while a mifc_graph capture is open.  nx * ny == 0: the flags are ALL_DEFINED, nothing else is written.
 * memkind works as everywhere else; host memory works at any size: the call stages a band of rows at a time, tcoord as
 * one more group of ntargets planes, within MIFC_VREGRID_CHUNK_MIB of device memory (default 256).  Every input level is
 * read once per pass of `tb` target planes.  mifc_last_vregrid_form: a diagnostic for tests, the
 * calling thread's last call that launched: "v=4|1 tb=<planes per pass> passes=<n> from=first|last outside=undef|clamp
 * coord=hybrid|field|levels method=linear|log launches=<n>". */
enum { MIFC_VREGRID_FROM_FIRST = 0, MIFC_VREGRID_FROM_LAST = 1 };
enum { MIFC_VREGRID_OUTSIDE_UNDEF = 0, MIFC_VREGRID_OUTSIDE_CLAMP = 1 };
int mifc_vregrid_hlevels(mifc_ctx* ctx, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields,
                         const float* ps, int fdef_ps, const float* alevel, const float* blevel, const float* tcoord,
                         const int* fdef_tcoord /* HOST int[ntargets], NULL = SOME_DEFINED */, int ntargets, int method, int from,
                         int outside, float* const* fres, int* fdefined_out, float undef, int memkind);
int mifc_vregrid_fields(mifc_ctx* ctx, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields,
                        const float* coord, const int* fdef_coord /* HOST int[nlev], NULL = SOME_DEFINED */, const float* tcoord,
                        const int* fdef_tcoord, int ntargets, int method, int from, int outside, float* const* fres,
                        int* fdefined_out, float undef, int memkind);
int mifc_vregrid_levels(mifc_ctx* ctx, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields,
                        const float* levels /* HOST float[nlev] */, const float* tcoord, const int* fdef_tcoord, int ntargets,
                        int method, int from, int outside, float* const* fres, int* fdefined_out, float undef, int memkind);
const char* mifc_last_vregrid_form(void);

/* ---- EXTENSION: layer integrals, means and extremes of level batches -----------------------------------------
 * Not a miutil::fieldcalc function: the reference leaves every reduction over levels (precipitable water, a layer-mean
 * wind, the maximum wind of a layer and where it sits, a pressure-weighted mean between two surfaces) to a host loop of
 * its caller.  nfields fields of [nlev][ny][nx] and one coordinate per level and cell go in -- the same inputs as
 * mifc_vinterp_* above --, fres[f] is [nproducts][ny][nx].  `products` is a HOST array of distinct codes:
 * MIFC_VLAYER_INTEGRAL, _MEAN, _MAX, _MIN, _COORD_OF_MAX, _COORD_OF_MIN.  The layer is [lo, hi] in the coordinate;
 * +-infinity means open; lo_field / hi_field are optional [ny][nx] fields of the same memory kind that give the bound
 * per cell (ps - 100 for the lowest 100 hPa), NULL = use the scalar.  Per cell i:
 *   1. Coordinate.  c_k exactly as rule 1 of mifc_vinterp_* gives it, in both forms (hybrid: the float product, then the
 *      float sum).  A coordinate is usable when it is defined by that rule AND is not NaN.  If any c_k of the cell is
 *      not usable, every product of every field is undef at i.
 *   2. Bounds.  L = lo_field[i] if given, else lo; H likewise.  A bound from a field is always tested: NaN or == undef
 *      makes the cell undef.  !(L < H): the cell is undef.
 *   3. Pairs.  For k = 0 .. nlev - 2 in index order: p = (c_k <= c_{k+1}) ? c_k : c_{k+1}, q the other one;
 *      a = (p >= L) ? p : L, b = (q <= H) ? q : H.  The pair takes part iff a < b.  No level order and no monotonicity
 *      is assumed; overlapping pairs of a non-monotone column each count.  If no pair takes part, the cell is undef for
 *      every field.
 *   4. Values.  Field f needs x_k and x_{k+1} defined at EVERY pair that takes part, each under
 *      is_defined(fdefined_in[f * nlev + level] == ALL_DEFINED, x, undef); otherwise all products of f are undef at i (an
 *      integral with a hole in it is a wrong number, not a partial one).  Levels outside the layer do not matter.
 *   5. End values, in double, every operation rounded on its own.  For an end e of {a, b}: e == c_k: v = (double)x_k;
 *      else e == c_{k+1}: v = (double)x_{k+1}; else w = ((double)e - c_k) / ((double)c_{k+1} - c_k) and
 *      v = x_k + w * (x_{k+1} - x_k).  d = (double)b - (double)a; ext += d; acc_f += ((v_a + v_b) * 0.5) * d.
 *   6. Products.  INTEGRAL = (float)acc_f.  MEAN = (float)(acc_f / ext).  The extremes work on (float)v, the end nearer
 *      level k first and then the other, in pair order: the first candidate initialises both extremes, a later one
 *      replaces the maximum on strict > and the minimum on strict <, so the first occurrence wins and a NaN that comes
 *      first stays.  COORD_OF_MAX / COORD_OF_MIN is the float e of the winning candidate: always a level's coordinate or
 *      a bound, never computed.
 *   7. Flags.  fdefined_out[f * nproducts + p] = checkDefined(cells that rules 1 to 4 left undef, nx * ny): the same
 *      for every product of a field.  A computed NaN or infinity is not counted.
 * Results are bit for bit this definition (restated in numpy in tests/vlayer_restate.py).
 * Arguments as for mifc_vinterp_*: `fields`, `fres` HOST arrays of nfields pointers; `fdefined_in` HOST int[nfields *
 * nlev] or NULL; `alevel`, `blevel` HOST float[nlev]; `fdef_coord` HOST int[nlev] or NULL; `fdefined_out` HOST
 * int[nfields * nproducts], field-major.
 * Refused calls return 0, write nothing and give the reason in mifc_last_error().  They are: nlev < 2; nfields outside
 * 1..8; nproducts outside 1..6; an unknown or repeated product code; a negative nx or ny; a null pointer that is
 * required; with both bounds scalar !(lo < hi), with one scalar bound that scalar NaN; hybrid form only: a level whose
 * (alevel, blevel) the reference's bad_hlevel (FieldCalculations.cc:298) rejects; an output that overlaps an input, the
 * coordinate, ps, a bound field or another output; a call made while a mifc_graph capture is open.
 * memkind works as everywhere else; host memory works at any size: the call stages a band of rows at a time,
 * MIFC_VLAYER_CHUNK_MIB of device memory (default 256).  Every field level is read once per call. */
enum {
  MIFC_VLAYER_INTEGRAL = 1,
  MIFC_VLAYER_MEAN = 2,
  MIFC_VLAYER_MAX = 3,
  MIFC_VLAYER_MIN = 4,
  MIFC_VLAYER_COORD_OF_MAX = 5,
  MIFC_VLAYER_COORD_OF_MIN = 6
};
int mifc_vlayer_hlevels(mifc_ctx* ctx, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields,
                        const float* ps, int fdef_ps, const float* alevel, const float* blevel, float lo, float hi,
                        const float* lo_field, const float* hi_field, const int* products, int nproducts, float* const* fres,
                        int* fdefined_out, float undef, int memkind);
int mifc_vlayer_fields(mifc_ctx* ctx, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields,
                       const float* coord, const int* fdef_coord /* HOST int[nlev], NULL = SOME_DEFINED */, float lo, float hi,
                       const float* lo_field, const float* hi_field, const int* products, int nproducts, float* const* fres,
                       int* fdefined_out, float undef, int memkind);

/* ---- EXTENSION: vertical derivatives of level batches, with vector magnitude ---------------------------------
 * Not a miutil::fieldcalc function: static stability (d theta / dp), the lapse rate, the vertical wind shear, dp / d theta
 * for isentropic potential vorticity, the thermal wind -- the reference leaves every difference across levels to a host
 * loop of its caller.  nfields fields of [nlev][ny][nx] and one coordinate per level go in -- the inputs of
 * mifc_vinterp_* and mifc_vlayer_* above, or (mifc_vderiv_levels) one coordinate value per level: pressure levels, the
 * `targets` of an earlier mifc_vinterp_* call --, fres[f] is [nlev][ny][nx]: one derivative per input level.  fmag is
 * optional: nfields / 2 outputs [nlev][ny][nx], fmag[j] the magnitude of the derivative of the vector whose components
 * are the fields 2j and 2j + 1 (u, v: the shear).  fres may be NULL as a whole when fmag is given: only the magnitudes are
 * written.  Per cell i, field f and output level k:
 *   1. Coordinate.  c_k exactly as rule 1 of mifc_vinterp_* gives it (hybrid: the float product, then the float sum);
 *      mifc_vderiv_levels: c_k = levels[k], always defined.  A coordinate is usable when it is defined by that rule AND
 *      is not NaN.  Unlike mifc_vlayer_*, an unusable coordinate affects only the levels that touch it.
 *   2. Points.  Point m is usable for f when c_m is usable and x_m passes is_defined(fdefined_in[f * nlev + m] ==
 *      ALL_DEFINED, x_m, undef).  If point k itself is not usable the result is undef.
 *   3. Sides.  The lower side k - 1 takes part when k > 0, point k - 1 is usable and c_{k-1} != c_k; the upper side k + 1
 *      likewise with k < nlev - 1.  No level order and no monotonicity is assumed.
 *   4. Both sides take part.  All in double, every operation rounded on its own (no contraction).
 *      MIFC_VDERIV_CENTRED = 0: dc = c_{k+1} - c_{k-1}; dc == 0 (a folded column): undef; otherwise w = 1.0 / dc and
 *      r = (x_{k+1} - x_{k-1}) * w.
 *      MIFC_VDERIV_WEIGHTED = 1 (second order on uneven spacing): h1 = c_k - c_{k-1}, h2 = c_{k+1} - c_k, s = h1 + h2;
 *      s == 0: undef; otherwise w1 = h2 / (h1 * s), w2 = h1 / (h2 * s), r = (x_k - x_{k-1}) * w1 + (x_{k+1} - x_k) * w2.
 *   5. One side takes part (the first and the last level, the level next to a hole or to the ground of a pressure-level
 *      batch), both methods: with (a, b) the two points in index order w = 1.0 / (c_b - c_a), r = (x_b - x_a) * w.
 *   6. No side takes part: undef.
 *   7. The result is (float)r.  A computed NaN or infinity is a value: not undef, not counted.
 *   8. Magnitude.  fmag[j] is the reference's absval (math_util.h:57) of the two float results, sqrtf(a * a + b * b) in
 *      float, uncontracted, the square root correctly rounded; undef where either component is undef by rules 2 to 6.
 *   9. Flags.  fdefined_out[f * nlev + k] = checkDefined(cells left undef at level k, nx * ny); fdefined_mag[j * nlev + k]
 *      the same for the magnitude.
 * The weights depend on the coordinate only: the divisions are paid once per cell and level however many fields the
 * call carries, in the `levels` form once per level.  Results are bit for bit this definition (restated in numpy in
 * tests/vderiv_restate.py).
 * Arguments as for mifc_vinterp_*: `fields`, `fres` HOST arrays of nfields pointers, `fmag` a HOST array of nfields / 2
 * pointers; `fdefined_in` HOST int[nfields * nlev] or NULL; `alevel`, `blevel`, `levels` HOST float[nlev]; `fdef_coord`
 * HOST int[nlev] or NULL; `fdefined_out` HOST int[nfields * nlev], `fdefined_mag` HOST int[(nfields / 2) * nlev].
 * Refused calls return 0, write nothing and give the reason in mifc_last_error().  They are: nlev < 2; nfields outside
 * 1..8; a negative nx or ny; an unknown method; a null pointer that is required; fres and fmag both NULL; fmag with an
 * odd nfields; fmag without fdefined_mag; fres without fdefined_out; hybrid form: a level whose (alevel, blevel) the
 * reference's bad_hlevel (FieldCalculations.cc:298) rejects; `levels` form: a NaN level; an output that overlaps an
 * input, the coordinate, ps or another output by byte range (in-place is not offered); a call made while a mifc_graph
 * capture is open.
 * memkind works as everywhere else; host memory works at any size: the call stages a band of rows at a time,
 * MIFC_VDERIV_CHUNK_MIB of device memory (default 256).  Every input level is read once and every output level written
 * once per call. */
enum { MIFC_VDERIV_CENTRED = 0, MIFC_VDERIV_WEIGHTED = 1 };
int mifc_vderiv_hlevels(mifc_ctx* ctx, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields,
                        const float* ps, int fdef_ps, const float* alevel, const float* blevel, int method, float* const* fres,
                        int* fdefined_out, float* const* fmag, int* fdefined_mag, float undef, int memkind);
int mifc_vderiv_fields(mifc_ctx* ctx, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields,
                       const float* coord, const int* fdef_coord /* HOST int[nlev], NULL = SOME_DEFINED */, int method,
                       float* const* fres, int* fdefined_out, float* const* fmag, int* fdefined_mag, float undef, int memkind);
int mifc_vderiv_levels(mifc_ctx* ctx, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields,
                       const float* levels /* HOST float[nlev] */, int method, float* const* fres, int* fdefined_out,
                       float* const* fmag, int* fdefined_mag, float undef, int memkind);

/* ---- EXTENSION: running vertical integrals of level batches --------------------------------------------------
 * Not a miutil::fieldcalc function: the height of hybrid levels (the hydrostatic integration of virtual temperature over
 * ln p from the surface upward), the mass above or below every level, the optical depth or cloud water path down to each
 * level, the running precipitable water, the thickness between pressure levels -- any integral of x dc whose upper limit
 * is every level in turn; the reference leaves them to a host loop of its caller.  nfields fields of [nlev][ny][nx] and
 * one coordinate per level go in -- the three coordinate forms of mifc_vderiv_* above --, fres[f] is [nlev][ny][nx]: the
 * integral up to each input level, itself a level batch (a height batch for mifc_vinterp_fields, say).  Per cell i and
 * field f:
 *   1. Coordinate.  c_k exactly as rule 1 of mifc_vinterp_* gives it (hybrid: the float product, then the float sum);
 *      mifc_vcumul_levels: c_k = levels[k].  A coordinate is usable when it is defined by that rule, is not NaN and, with
 *      MIFC_VCUMUL_LOG, is > 0.  g(c) = (double)c for MIFC_VCUMUL_LINEAR = 0, log((double)c) for MIFC_VCUMUL_LOG = 1.
 *   2. Walk order.  k(0), k(1), ... is 0, 1, ..., nlev - 1 for MIFC_VCUMUL_FROM_FIRST = 0 and nlev - 1, ..., 0 for
 *      MIFC_VCUMUL_FROM_LAST = 1.  No monotonicity is assumed; the integral is signed.
 *   3. Point.  Point m is usable for f when c_m is usable and x_m passes is_defined(fdefined_in[f * nlev + m] ==
 *      ALL_DEFINED, x_m, undef).
 *   4. Start.  S = +0.0.  If `start` is given it must be usable in the sense of rule 1 under fdef_start; otherwise every
 *      level of every field is undef at i.  If it is given and point k(0) is usable, S = x_{k(0)} * (g(c_{k(0)}) -
 *      g(start_i)): the integrand is held constant between the start and the first level.
 *   5. Step.  With a = k(m), b = k(m + 1): S += ((x_a + x_b) * 0.5) * (g(c_b) - g(c_a)), all in double, every operation
 *      rounded on its own (no contraction): the operation order of rule 5 of mifc_vlayer_*.
 *   6. Holes.  An integral with a hole in it is a wrong number, not a partial one: from the first point in walk order that
 *      is not usable for f, that level and every later one are undef for f; earlier levels are unaffected.  A base[f]
 *      that fails is_defined(fdef_base[f] == ALL_DEFINED, base_f[i], undef) or is NaN makes every level of f undef at i.
 *   7. Result.  (float)((double)base_f[i] + scale_f * S) at each level: the product rounded, then the sum; without a
 *      base the sum is absent.  A computed NaN or infinity is a value: not undef, not counted.
 *   8. Flags.  fdefined_out[f * nlev + k] = checkDefined(cells left undef at level k, nx * ny).
 * MIFC_VCUMUL_LINEAR is bit for bit this definition (restated in numpy in tests/vcumul_restate.py).  MIFC_VCUMUL_LOG
 * depends on the device's double log(): a result is the definition's float or its neighbour, as for MIFC_VINTERP_LOG;
 * undef cells and flags are exact.  In the `levels` form g(levels[k]) is computed once per level on the host.  The
 * logarithm is paid once per cell and level however many fields the call carries.
 * Arguments as for mifc_vderiv_*: `fields`, `fres` HOST arrays of nfields pointers (1..8); `fdefined_in`,
 * `fdefined_out` HOST int[nfields * nlev], field-major; `alevel`, `blevel`, `levels` HOST float[nlev]; `fdef_coord`
 * HOST int[nlev] or NULL.  `start` is optional: [ny][nx] of the call's memory kind, the coordinate at which the integral
 * begins (ps); NULL: it begins at the first walked level.  `base` is optional: a HOST array of nfields pointers to
 * [ny][nx] (the table or any entry may be NULL), the value added to the result (the surface height); `fdef_base` HOST
 * int[nfields] or NULL = SOME_DEFINED.  `scale` is optional: HOST double[nfields], NULL = 1.0 (-Rd / g, 1 / g).
 * Refused calls return 0, write nothing and give the reason in mifc_last_error().  They are: nlev < 2; nfields outside
 * 1..8; a negative nx or ny; an unknown method or from; a null pointer that is required; a NaN scale[f]; hybrid form: a
 * level whose (alevel, blevel) the reference's bad_hlevel (FieldCalculations.cc:298) rejects; `levels` form: a NaN
 * level, or MIFC_VCUMUL_LOG with a level <= 0; an output that overlaps an input, the coordinate, ps, start, a base plane
 * or another output by byte range (in-place is not offered); a call made while a mifc_graph capture is open.  Zero
 * cells: the flags are ALL_DEFINED, the call returns 1.
 * memkind works as everywhere else; host memory works at any size: the call stages a band of rows at a time,
 * MIFC_VCUMUL_CHUNK_MIB of device memory (default 256).  Every input level is read once and every output level written
 * once per call.  mifc_last_vcumul_form: a diagnostic for tests, the calling thread's last call that
 * launched: "v=4 fields=4 method=log from=last launches=2" -- cells per lane, fields of the first pass, launches in all. */
enum { MIFC_VCUMUL_LINEAR = 0, MIFC_VCUMUL_LOG = 1 };
enum { MIFC_VCUMUL_FROM_FIRST = 0, MIFC_VCUMUL_FROM_LAST = 1 };
int mifc_vcumul_hlevels(mifc_ctx* ctx, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields,
                        const float* ps, int fdef_ps, const float* alevel, const float* blevel, int method, int from,
                        const float* start, int fdef_start, const float* const* base, const int* fdef_base, const double* scale,
                        float* const* fres, int* fdefined_out, float undef, int memkind);
int mifc_vcumul_fields(mifc_ctx* ctx, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields,
                       const float* coord, const int* fdef_coord /* HOST int[nlev], NULL = SOME_DEFINED */, int method, int from,
                       const float* start, int fdef_start, const float* const* base, const int* fdef_base, const double* scale,
                       float* const* fres, int* fdefined_out, float undef, int memkind);
int mifc_vcumul_levels(mifc_ctx* ctx, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields,
                       const float* levels /* HOST float[nlev] */, int method, int from, const float* start, int fdef_start,
                       const float* const* base, const int* fdef_base, const double* scale, float* const* fres,
                       int* fdefined_out, float undef, int memkind);
const char* mifc_last_vcumul_form(void);

/* ---- EXTENSION: parcel ascent over level batches: CAPE, CIN, LCL, LFC, EL -------------------------------------
 * Not a miutil::fieldcalc function.  The reference lifts a parcel across ONE layer, in showalterIndex
 * (FieldCalculations.cc:872): along the dry adiabat to the upper level, then humidity and heat adjusted there in seven
 * iterations.  Stepping that adjustment from level to level through a batch gives the parcel curve; one more walk of the
 * column gives the convective available potential energy, the inhibition and the three levels a forecaster reads off a
 * sounding.  t is [nlev][ny][nx] in K, pressure in hPa in one of the three coordinate forms of mifc_vcumul_*.  The
 * parcel's source is a level of the batch (src_level >= 0: that level's t and pressure, with the specific humidity q_src
 * [ny][nx] in kg/kg) or three planes (src_level == -1: t_src, q_src, p_src -- a mixed-layer parcel from mifc_vlayer_*
 * means).  Outputs, each optional, at least one: the planes cape (J/kg), cin (J/kg, <= 0), plcl, plfc, pel (hPa) and the
 * batch tparcel [nlev][ny][nx], the parcel temperature at every walked level.  Constants as MetConstants.h: cp = 1004,
 * Rd = 287, eps = 0.622, xlh = 2.501e6, t0 = 273.15, kappa = Rd / cp, all float.  Per cell:
 *   1. Walk and usable points.  Walk order k(0), k(1), ... as rule 2 of mifc_vcumul_* (from = MIFC_VPARCEL_FROM_FIRST /
 *      _LAST).  p_k exactly as rule 1 of mifc_vinterp_* gives it (hybrid: the float product, then the float sum;
 *      mifc_vparcel_levels: levels[k]).  A point is usable when p_k is defined by that rule, is not NaN, is > 0 and is
 *      strictly below the pressure of the previous point of the walk (the source first), and t_k passes
 *      is_defined(fdefined_in[k] == ALL_DEFINED, t_k, undef) and is not NaN.  With a source level the walk is the positions
 *      behind that level; levels in front of it are not walked.  With source planes the positions in walk order are
 *      skipped until the first whose pressure is < p_src (an undefined pressure is not); it is the first walked point.
 *      The first walked point that is not usable ends the walk: tparcel is undef from there on and every plane is undef
 *      at the cell -- an integral with a hole is a wrong number (rule 6 of mifc_vcumul_*).  The source is usable when its
 *      temperature, humidity and pressure are defined under their flags (the level's flag, fdef_tsrc, fdef_qsrc,
 *      fdef_psrc, the pressure form's rule), none is NaN, the pressure is > 0 and the temperature (cp * T) / cp lies in
 *      the saturation table (MetConstants.h:64-80); otherwise everything is undef at the cell.
 *   2. State.  tcl = cp * T_src and qcl = q_src, both float.  pi(p) = cp * powf(p * p0inv, kappa), the reference's
 *      pi_from_p, float.  The parcel temperature at any point is tcl / cp (float); at a source level tparcel holds it too.
 *   3. Step from point a to the next point b.  Dry: tcl = tcl * (pi_b / pi_a), the float quotient rounded first, then the
 *      float product.  Saturation test: x = tcl / cp - t0 looked up as showalterIndex does (:949-953), qsat = eps * esat /
 *      p_b in float (the product, then the quotient).  A temperature outside the table here ends the walk as in rule 1.
 *      If qcl > qsat the seven trips of :948-960 run verbatim with p500 := p_b, its `break` outside the table and its a1
 *      from qcl included; otherwise the state is unchanged.  tparcel_b = tcl / cp.  The deficit of the point is
 *      d_b = (double)qsat - (double)qcl with the values of the test (before the trips); at the source d = qsat_src - q_src.
 *   4. Buoyancy.  B_b = (double)tparcel_b - (double)t_b; at the source B = +0.  Between two points B is linear in
 *      ln p, l = log((double)p).  There is NO virtual-temperature correction: humidity does not enter B.
 *   5. LCL.  The source if q_src >= qsat_src: plcl = p_src.  Otherwise at the first point b with qcl > qsat, a the point
 *      before it: w = d_a / (d_a - d_b), l_lcl = l_a + w * (l_b - l_a), B_lcl = B_a + w * (B_b - B_a), plcl =
 *      (float)exp(l_lcl).  The LCL cuts the piece (a, b) of B into (a, LCL) and (LCL, b).  Never saturated: plcl, plfc,
 *      pel, cin undef, cape = +0.
 *   6. Pieces, in walk order.  For a piece from (Ba, la) to (Bb, lb), h = la - lb: `up` is !(Ba > 0) and Bb > 0, `down`
 *      is Ba > 0 and !(Bb > 0).  With up or down: w0 = Ba / (Ba - Bb), lx = la + w0 * (lb - la), h1 = w0 * h, h2 = h - h1,
 *      A1 = (Ba * 0.5) * h1, A2 = (Bb * 0.5) * h2; pos = A2, neg = A1 for up and pos = A1, neg = A2 for down.  Otherwise
 *      A = ((Ba + Bb) * 0.5) * h is pos where both are > 0, else neg.  While no LFC is known: cin_sum += neg; if the piece
 *      lies at or above the LCL and is `up`, the LFC is its zero, plfc = (float)exp(lx), and cape_sum += pos.  Once the
 *      LFC is known: cape_sum += pos, and a `down` piece sets pel = (float)exp(lx) (the highest one stays).  The LFC is the
 *      LCL itself when B_lcl > 0 (settled between the two pieces of rule 5).  No LFC: plfc, pel, cin undef, cape = +0.
 *   7. EL.  pel is undef if no piece went down behind the LFC or if B > 0 at the last walked point; CAPE then ends there.
 *   8. Integrals.  cape = (float)(287.0 * cape_sum), cin = (float)(287.0 * cin_sum); the sums start at +0.0; everything
 *      in rules 4 to 8 is double, every operation rounded on its own (no contraction), in the order written here and in
 *      tests/vparcel_restate.py.
 *   9. Flags.  fdefined_out[0..4] = checkDefined(cells left undef, nx * ny) of cape, cin, plcl, plfc, pel,
 *      fdefined_out[5 + k] of tparcel's level k; the entries of outputs that are not asked for are not written.
 * tests/vparcel_restate.py is this definition in numpy.  Undef cells and flags are exact.  Values depend on the device's
 * x^kappa (the correctly rounded float or its neighbour) and on its double log / exp: they lie within the response of the
 * definition to a one-ulp change of pi (tests/test_gpu_vparcel.py); a cell's bits do not depend on the cells per lane,
 * the launch shape, the memory kind or the banding.  In the `levels` form pi of every level is computed once on the host.
 * Arguments: t, ps / p, t_src, q_src, p_src and the outputs in the call's memory kind; fdefined_in HOST int[nlev] or NULL
 * = SOME_DEFINED; alevel, blevel, levels HOST float[nlev]; fdef_coord HOST int[nlev] or NULL; fdefined_out HOST
 * int[5 + nlev].  t_src and p_src are not read with a source level and may be NULL then.
 * Refused calls return 0, write nothing and give the reason in mifc_last_error().  They are: nlev < 2; a negative nx or
 * ny; an unknown from; src_level outside -1..nlev - 1; a null pointer that is required; no output at all; hybrid form: a
 * level whose (alevel, blevel) the reference's bad_hlevel (FieldCalculations.cc:298) rejects; `levels` form: a NaN level
 * or a level <= 0; an output that overlaps an input, the pressure, ps, a source plane or another output by byte range; a
 * call made while a mifc_graph capture is open.  Zero cells: the flags are ALL_DEFINED, the call returns 1.
 * memkind works as everywhere else; host memory works at any size: the call stages a band of rows at a time,
 * MIFC_VPARCEL_CHUNK_MIB of device memory (default 256).  Every input level is read once per call.
 * mifc_last_vparcel_form: a diagnostic for tests, the calling thread's last call that launched:
 * "v=4 form=hlevels from=last src=136 outputs=6 launches=1". */
enum { MIFC_VPARCEL_FROM_FIRST = 0, MIFC_VPARCEL_FROM_LAST = 1 };
int mifc_vparcel_hlevels(mifc_ctx* ctx, int nx, int ny, int nlev, const float* t, const int* fdefined_in, const float* ps, int fdef_ps,
                         const float* alevel, const float* blevel, int from, int src_level, const float* t_src, int fdef_tsrc,
                         const float* q_src, int fdef_qsrc, const float* p_src, int fdef_psrc, float* cape, float* cin, float* plcl,
                         float* plfc, float* pel, float* tparcel, int* fdefined_out, float undef, int memkind);
int mifc_vparcel_fields(mifc_ctx* ctx, int nx, int ny, int nlev, const float* t, const int* fdefined_in, const float* p,
                        const int* fdef_coord /* HOST int[nlev], NULL = SOME_DEFINED */, int from, int src_level, const float* t_src,
                        int fdef_tsrc, const float* q_src, int fdef_qsrc, const float* p_src, int fdef_psrc, float* cape, float* cin,
                        float* plcl, float* plfc, float* pel, float* tparcel, int* fdefined_out, float undef, int memkind);
int mifc_vparcel_levels(mifc_ctx* ctx, int nx, int ny, int nlev, const float* t, const int* fdefined_in,
                        const float* levels /* HOST float[nlev] */, int from, int src_level, const float* t_src, int fdef_tsrc,
                        const float* q_src, int fdef_qsrc, const float* p_src, int fdef_psrc, float* cape, float* cin, float* plcl,
                        float* plfc, float* pel, float* tparcel, int* fdefined_out, float undef, int memkind);
const char* mifc_last_vparcel_form(void);

/* ---- EXTENSION: Ertel potential vorticity of level batches ----------------------------------------------------
 * Not a miutil::fieldcalc function: the one diagnostic that differences a level batch along all three axes, and the
 * coordinate batch of the dynamic tropopause (mifc_vinterp_fields with PV as the coordinate and 2 PVU as the target).
 * u, v, th (the wind components and the potential temperature), each [nlev][ny][nx], one coordinate p per level -- the
 * three coordinate forms of mifc_vderiv_* above --, the map ratios xmapr = xm / (2 hx), ymapr = ym / (2 hy) of the
 * reference's stencil operators and, optionally, fcoriolis go in ([ny][nx] each); fpv is [nlev][ny][nx].
 * Per level k and cell (x, y): (xc, yc) = (clamp(x, 1, nx - 2), clamp(y, 1, ny - 2)), i = yc * nx + xc, and everything
 * below is evaluated at i: the outer ring carries the value of its nearest interior cell, which is what the reference's
 * fillEdges produces (FieldCalculations.cc:59-74).
 *   1. Coordinate.  c_k exactly as rule 1 of mifc_vinterp_* gives it, usable as in rule 1 of mifc_vderiv_*.
 *   2. Vertical derivatives.  D_u, D_v, D_th at (k, i) are the double r of rules 2 to 6 of mifc_vderiv_* BEFORE its
 *      rounding to float, each per field, with the call's method (MIFC_VDERIV_CENTRED / MIFC_VDERIV_WEIGHTED).  A field
 *      whose derivative those rules leave undef (centre not usable, no side, zero denominator) makes the cell undef.
 *   3. Horizontal terms, at level k, in the reference's arithmetic (FieldCalculations.cc:1862):
 *      dx(a) = (0.5 * (double)xmapr[i]) * (double)(a[i + 1] - a[i - 1]),
 *      dy(a) = (0.5 * (double)ymapr[i]) * (double)(a[i + nx] - a[i - nx]): the difference in float, the two products in
 *      double.  Needed: dx(v), dy(u), dx(th), dy(th).  Each of the eight neighbour values must pass
 *      is_defined(fdefined_in[f * nlev + k] == ALL_DEFINED, value, undef), otherwise the cell is undef.  xmapr, ymapr and
 *      fcoriolis are not tested, as in the reference; the coordinate of the neighbours plays no part.
 *   4. Product, in double, every operation rounded on its own, in this order: zeta = dx(v) - dy(u);
 *      za = zeta + (double)fcoriolis[i] (fcoriolis == NULL: the addition is absent); t1 = za * D_th; t2 = D_v * dx(th);
 *      t3 = D_u * dy(th); S = (t1 - t2) + t3.
 *   5. Result.  (float)(scale * S).  A computed NaN or infinity is a value: not undef, not counted.
 *   6. Flag.  fdefined_out[k] = checkDefined(interior cells left undef at level k, (nx - 2) * (ny - 2)); the ring is a
 *      copy and is not counted.
 * This is PV = -g [(f + zeta) dth/dp - dv/dp dth/dx + du/dp dth/dy] for scale = -g, the horizontal differences taken
 * along the surfaces of the batch, so the formula holds on pressure, hybrid and any other levels; with p in hPa
 * scale = -g * 1e4 gives PVU.  Bit for bit this definition (restated in numpy in tests/pvort_restate.py).
 * `fdefined_in` HOST int[3 * nlev] in the order u, v, th, NULL = SOME_DEFINED; `fdefined_out` HOST int[nlev]; `alevel`,
 * `blevel`, `levels` HOST float[nlev]; `fdef_coord` HOST int[nlev] or NULL.
 * Refused calls return 0, write nothing and give the reason in mifc_last_error().  They are: nlev < 2; a negative nx or
 * ny; nx < 3 or ny < 3 with a grid that is not empty (the reference's stencil operators return false there); an unknown
 * method; a NaN scale; a null pointer that is required; hybrid form: a level whose (alevel, blevel) the reference's
 * bad_hlevel rejects; `levels` form: a NaN level; fpv overlapping any input by byte range; a call made while a
 * mifc_graph capture is open.  Zero cells: the flags are ALL_DEFINED, the call returns 1.
 * memkind works as everywhere else; host memory works at any size: the call stages a band of rows at a time with the
 * neighbour rows it needs, MIFC_PVORT_CHUNK_MIB of device memory (default 256); the result does not depend on the bands.
 * One launch walks the levels once per workgroup tile.  mifc_last_pvort_form: a diagnostic for tests,
 * the calling thread's last call that launched: "v=4 kind=hybrid method=weighted tile=128x8 launches=1 bands=1". */
int mifc_pvort_hlevels(mifc_ctx* ctx, int nx, int ny, int nlev, const float* u, const float* v, const float* th,
                       const int* fdefined_in /* HOST int[3 * nlev], order u, v, th; NULL = SOME_DEFINED */, const float* ps, int fdef_ps,
                       const float* alevel, const float* blevel, const float* xmapr, const float* ymapr,
                       const float* fcoriolis /* may be NULL */, int method, double scale, float* fpv, int* fdefined_out, float undef,
                       int memkind);
int mifc_pvort_fields(mifc_ctx* ctx, int nx, int ny, int nlev, const float* u, const float* v, const float* th, const int* fdefined_in,
                      const float* p, const int* fdef_coord /* HOST int[nlev] or NULL */, const float* xmapr, const float* ymapr,
                      const float* fcoriolis, int method, double scale, float* fpv, int* fdefined_out, float undef, int memkind);
int mifc_pvort_levels(mifc_ctx* ctx, int nx, int ny, int nlev, const float* u, const float* v, const float* th, const int* fdefined_in,
                      const float* levels /* HOST float[nlev] */, const float* xmapr, const float* ymapr, const float* fcoriolis, int method,
                      double scale, float* fpv, int* fdefined_out, float undef, int memkind);
const char* mifc_last_pvort_form(void);

/* ---- EXTENSION: level batches sampled at arbitrary points (regridding, cross-sections, soundings) ------------
 * Not a miutil::fieldcalc function: the reference's callers take a field to a flight route, a section line, a list of
 * stations or the grid of another projection on the host, level by level (their field class has an
 * interpolate(npos, xpos, ypos, ...) with a nearest, a bilinear and a cubic method).  nfields fields of [nlev][ny][nx]
 * and npos positions go in, fres[f] is [nlev][npos] -- itself a level batch of shape (nlev, 1, npos), which
 * mifc_vinterp_*, mifc_vlayer_* and mifc_vderiv_* take unchanged: a vertical cross-section on pressure surfaces is this
 * call on the fields and on the pressure batch (or ps), then mifc_vinterp_*.  Positions are in grid-index units: x = 0 is
 * column 0, x = nx - 1 the last column.  Vector components are not rotated by this call: mifc_hinterp_vector_levels
 * below samples pairs and rotates them in the same pass.  Per point p, field f and level k:
 *   1. Position.  x = xpos[p], y = ypos[p].  The position is unusable if !is_defined(false, x, undef) or
 *      !is_defined(false, y, undef) (NaN, or equal to undef), and, with xd = (double)x, yd = (double)y, unless
 *      xd >= 0.0 && xd <= (double)(nx - 1) && yd >= 0.0 && yd <= (double)(ny - 1).  An unusable position gives undef for
 *      every field and level at p.  -0.0 is inside; infinities are outside.
 *   2. Cell.  i0 = (int)xd, j0 = (int)yd (truncation); a = xd - i0, b = yd - j0 (double, exact).  Column i0 + 1 is read
 *      only when a != 0, row j0 + 1 only when b != 0: x == nx - 1 is legal and reads nothing outside the grid, and so is
 *      nx == 1 or ny == 1.
 *   3. A value v of field f, level k is defined iff is_defined(fdefined_in[f * nlev + k] == ALL_DEFINED, v, undef): a
 *      stored undef under ALL_DEFINED is a value.
 *   4. MIFC_HINTERP_NEAREST = 0: i = (int)(xd + 0.5), j = (int)(yd + 0.5); the result is field[k][j][i] bit for bit if
 *      that value is defined, else undef.
 *   5. MIFC_HINTERP_BILINEAR = 1: the needed corners are (j0, i0) always, (j0, i0 + 1) iff a != 0, (j0 + 1, i0) iff
 *      b != 0, (j0 + 1, i0 + 1) iff both.  If any needed corner is undefined the result is undef.  Otherwise, the corners
 *      widened to double, r0 = a == 0 ? x00 : x00 + a * (x10 - x00); b == 0: the result is (float)r0 (a point on a node
 *      returns the node bit for bit); otherwise r1 = a == 0 ? x01 : x01 + a * (x11 - x01) and the result is
 *      (float)(r0 + b * (r1 - r0)).
 *   6. MIFC_HINTERP_BICUBIC = 2 (Catmull-Rom) applies only when a != 0 || b != 0, 1 <= i0 <= nx - 3 and
 *      1 <= j0 <= ny - 3, and all 16 values of the rows j0 - 1 .. j0 + 2 by the columns i0 - 1 .. i0 + 2 are defined;
 *      if any of these fails, that (point, field, level) follows rule 5 unchanged.  Weights in double, t = a for the
 *      columns and t = b for the rows: w-1 = ((-0.5 * t + 1.0) * t - 0.5) * t, w0 = ((1.5 * t - 2.5) * t) * t + 1.0,
 *      w1 = ((-1.5 * t + 2.0) * t + 0.5) * t, w2 = ((0.5 * t - 0.5) * t) * t.  Row sums
 *      s_m = ((w-1 * x_m,-1 + w0 * x_m,0) + w1 * x_m,1) + w2 * x_m,2 for the four rows; the result is
 *      (float)(((wy-1 * s_-1 + wy0 * s_0) + wy1 * s_1) + wy2 * s_2).
 *   7. Flags.  fdefined_out[f * nlev + k] = checkDefined(points that rules 1, 4, 5 left undef, npos).  A computed result
 *      is never counted, whatever its value.
 * Every operation is an IEEE float or double operation rounded on its own (no contraction): results are bit for bit this
 * definition (restated in numpy in tests/hinterp_restate.py).
 * Arguments: `fields`, `fdefined_in`, nfields (1..8), undef and memkind as for mifc_vderiv_fields: `fields` a HOST array
 * of nfields pointers to [nlev][ny][nx] batches, `fdefined_in` a HOST int[nfields * nlev] or NULL (all SOME_DEFINED).
 * `xpos`, `ypos` are float[npos] and live where memkind says, like the fields; `fres` is a HOST array of nfields
 * pointers, each to [nlev][npos] in the same memory kind; `fdefined_out` a HOST int[nfields * nlev].  Any alignment of
 * any pointer is accepted.
 * Refused calls return 0, write nothing and give the reason in mifc_last_error().  They are: nlev < 1; nfields outside
 * 1..8; npos < 1; nx < 1 or ny < 1; nx * ny > 2^31 - 1; an unknown method; a null pointer that is required; an output
 * that overlaps a field, xpos, ypos or another output by byte range; a bad memkind; a call made while a mifc_graph
 * capture is open.
 * Device memory is used where it is: no copies, one synchronisation at the end.  Host memory works at any size: levels
 * are independent, so the positions are uploaded once and the call stages whole levels of every field at a time,
 * MIFC_HINTERP_CHUNK_MIB of device memory (default 256) but never less than one level.
 * mifc_last_hinterp_form: the launch shape of the calling thread's last mifc_hinterp_levels call, a diagnostic for
 * tests: "method=<name> nf=<fields per launch> tested=0|1 blocks=<grid.x> level_chunks=<grid.y> chunk=<levels per
 * chunk> launches=<n>"; "" before the first call. */
enum { MIFC_HINTERP_NEAREST = 0, MIFC_HINTERP_BILINEAR = 1, MIFC_HINTERP_BICUBIC = 2 };
int mifc_hinterp_levels(mifc_ctx* ctx, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields,
                        int npos, const float* xpos, const float* ypos, int method,
                        float* const* fres, int* fdefined_out, float undef, int memkind);
const char* mifc_last_hinterp_form(void);

/* ---- EXTENSION: vector pairs of level batches rotated, on the grid and while sampling -------------------------
 * Not a miutil::fieldcalc function: a vector on a grid whose axes are not east and north (a rotated or polar-stereographic
 * model; wind regridded to another projection; along- and across-section wind) has to be rotated point by point.  With
 * field algebra that is six mifc_fieldOPERfield calls per pair and level, 72 B per cell where 16 B do, every product
 * rounded to float.  Two entries share one rule.
 *
 * Rule R, the rotation.  It applies per cell or point, per pair q and per level k.
 *   R1. The coefficients are c = cosa[p] and s = sina[p], one value per cell or point, shared by all levels and pairs.
 *       They are defined iff is_defined(fdef_rot == ALL_DEFINED, c, s, undef).  The library does not normalise them.  The
 *       sign convention is the caller's; the usual one gives u' = c*u - s*v, v' = s*u + c*v.
 *   R2. A pair result is a hole, and both outputs are undef, if any of these is undefined: the coefficients; u; v.  Each
 *       component is tested by its own input flag: a stored undef under ALL_DEFINED is a value.
 *   R3. Otherwise all four values are widened to double, and u' = (float)(c*u - s*v), v' = (float)(s*u + c*v).  Every
 *       operation is rounded on its own, with no contraction.  The two products are exact in double (24 x 24 bits).  Each
 *       result therefore carries one double rounding and one float rounding.  With (c, s) = (1, 0) a pair comes back bit
 *       for bit, except the sign of a zero: u = -0.0, v = -3 gives +0.0.
 *   R4. Flags: fdefined_out[(2q) * nlev + k] = fdefined_out[(2q + 1) * nlev + k] = checkDefined(holes of pair q at level
 *       k, number of cells or points).
 * (Restated in numpy in tests/vrotate_restate.py.)
 *
 * mifc_vrotate_levels, on the grid.  `fields` is a HOST array of 2 * npairs pointers (u0, v0, u1, v1, ...) to
 * [nlev][ny][nx] batches, npairs 1..4; `fdefined_in` a HOST int[2 * npairs * nlev] in that order or NULL (all
 * SOME_DEFINED); cosa, sina are [ny][nx] and live where memkind says, like the fields; `fres` is laid out like `fields`,
 * `fdefined_out` like `fdefined_in`.  nlev == 1 is legal.  In-place is not offered.  Refused calls return 0, write
 * nothing and give the reason in mifc_last_error(): nlev < 1; npairs outside 1..4; nx < 1 or ny < 1; nx * ny > 2^31 - 1;
 * a null pointer; an output that overlaps a field, cosa, sina or another output by byte range; a bad memkind; a call made
 * while a mifc_graph capture is open.  Device memory is used where it is (four cells per lane through 16-byte accesses
 * where every pointer and the level size allow, else one); host memory works at any size: cells are independent, so the
 * call stages a band of rows of every level and of the coefficients at a time (MIFC_VDERIV_CHUNK_MIB of device memory,
 * default 256, the budget of the other vector product).  mifc_last_vrotate_form: the launch shape of the calling thread's
 * last mifc_vrotate_levels call, a diagnostic for tests: "v=4|1 np=<pairs per launch> tested=0|1 blocks=<grid.x>
 * level_chunks=<grid.y> chunk=<levels per chunk> launches=<n>"; "" before the first call.
 *
 * mifc_hinterp_vector_levels, while sampling: mifc_hinterp_levels with npairs (1..4) in the place of nfields, `fields`,
 * `fres` and the flags laid out as above, and cosa, sina (float[npos], where memkind says) and fdef_rot behind ypos.  Each
 * component is sampled exactly by rules 1-7 of mifc_hinterp_levels, including its own bicubic-or-bilinear decision, and
 * rounded to float; the two floats are then rotated by rule R with the point's coefficients.  By definition the call
 * equals two calls bit for bit, flags included: mifc_hinterp_levels, then mifc_vrotate_levels on the (nlev, 1, npos)
 * batches with the flags of the first call and the coefficients as a (1, npos) plane.  A component is undefined (R2) where
 * rules 1, 4 and 5 left a hole.  The one call carries these holes, the second of two calls can only recognise them by
 * their value: the two differ where a component flagged ALL_DEFINED stores undef or NaN all the same -- the sampling hands
 * such a value on as the value it is (rule 3), this call rotates it, two calls take it for a hole.  The same holds for a
 * sampled value that the arithmetic made NaN or bit-equal to undef (inf - inf between two corners; the midpoint of 0 and
 * 2e35f): a computed result is a value (rule 7) and is rotated here, while the second of two calls, whose input flag is the
 * first call's output flag, takes it for a hole wherever that flag is not ALL_DEFINED.  A point whose
 * coefficients are undefined is treated like an unusable position: undef for every pair and level, counted once.  The refusals are those
 * of mifc_hinterp_levels ("npairs <n> outside 1..4"; cosa and sina may not be null nor overlap an output); host memory is
 * staged in whole levels (MIFC_HINTERP_CHUNK_MIB).  The call reports through mifc_last_hinterp_form, nf = the components
 * per launch (2 or 4). */
int mifc_vrotate_levels(mifc_ctx* ctx, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int npairs,
                        const float* cosa, const float* sina, int fdef_rot, float* const* fres, int* fdefined_out, float undef,
                        int memkind);
const char* mifc_last_vrotate_form(void);
int mifc_hinterp_vector_levels(mifc_ctx* ctx, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int npairs,
                               int npos, const float* xpos, const float* ypos, const float* cosa, const float* sina, int fdef_rot,
                               int method, float* const* fres, int* fdefined_out, float undef, int memkind);

/* ---- EXTENSION: horizontal statistics of level batches: area and row reductions --------------------------------
 * Not a miutil::fieldcalc function: the minimum and maximum of a field (a colour scale), an area-weighted domain mean, a
 * zonal mean, the bias or RMSE between two batches are numbers, and the reference's callers copy the whole batch to the
 * host for each of them.  This call turns a device-resident batch into numbers; its row-wise mean is itself a level batch
 * of shape (nlev, nrows, 1) that mifc_vinterp_fields takes, and the (nlev, 1, npos) output of mifc_hinterp_levels can be
 * reduced in turn.  Results are reproducible bit for bit whatever the launch shape, the memory kind or the staging: the
 * order of every addition is part of the definition.
 * Inputs: fields[f], up to 8 batches [nlev][ny][nx], with flags fdefined_in[f * nlev + k] (NULL: SOME_DEFINED); optional
 * minus[f], batches of the same shape with flags fdefined_minus (minus == NULL: none; it may not be given for only some
 * fields); optional pivot, a HOST double[nfields * nlev] (NULL: 0.0); optional weight, a float [ny][nx] shared by all
 * levels and fields, with one flag fdef_weight; optional box, a HOST int[4] = {i0, i1, j0, j1}, half-open (NULL: the whole
 * level); mode MIFC_HSTATS_AREA (one result per field and level, nrows = 1) or MIFC_HSTATS_ROWS (one per grid row of the
 * box, nrows = j1 - j0, row r is grid row j0 + r); products, a bit mask of MIFC_HSTATS_MOMENTS and MIFC_HSTATS_EXTREMES.
 * Per field f and level k:
 *   1. Included cell.  Cell (j, i) is included iff i0 <= i < i1 and j0 <= j < j1; x = fields[f][k][j][i] is defined,
 *      is_defined(flag == ALL_DEFINED, x, undef) (a stored undef under ALL_DEFINED is a value, as in mifc_hinterp_levels
 *      rule 3); with minus, y = minus[f][k][j][i] is defined by its own flag; with weight, weight[j][i] is defined by
 *      fdef_weight.  A caller masks a region by storing undef in weight.
 *   2. Cell quantities, all in double, each operation rounded on its own, no contraction:
 *      d = ((double)x - (double)y) - pivot (without minus the first subtraction is absent, d = (double)x - pivot; with
 *      pivot NULL d = (double)x exactly); w = (double)weight, or 1.0 without a weight; q1 = w * d; q2 = (w * d) * d.  An
 *      excluded cell contributes w = q1 = q2 = +0.0; because accumulators start at +0.0 this is identical to skipping it.
 *   3. Row segment sum, the order of every sum W = sum of w, S1 = sum of q1, S2 = sum of q2.  A grid row is cut by
 *      absolute column into segments of 4096 cells, segment s holding the columns 4096 s .. 4096 s + 4095.  Within a
 *      segment cell i belongs to partial l = (i / 4) mod 64.  Partial l is the sequential sum, in ascending i, of its
 *      cells, starting from +0.0: at most 16 trips of four consecutive cells.  The 64 partials are merged by
 *      for s in 32, 16, 8, 4, 2, 1: P[t] = P[t] + P[t + s] for t < s; the segment sum is P[0].  The mapping depends only on
 *      the column index, not on the address, the alignment, the box or the staging.
 *   4. Combination.  ROWS: the result of row r is the sequential sum, ascending, of its segment sums, starting from +0.0.
 *      AREA: the result is the sequential sum of ALL segment sums of the box rows in row-major order (row j0 segment 0,
 *      segment 1, ..., then row j0 + 1, ...), starting from +0.0.
 *   5. N is the exact number of included cells, stored as a double.
 *   6. Extremes are over d.  MIN is the smallest d of the included cells under the ordered comparison <, starting from
 *      +inf; IMIN is the smallest flat index j * nx + i within the level among the cells whose d equals it, and MIN is that
 *      cell's d bit for bit, so -0.0 and +0.0 tie and the first one wins.  MAX and IMAX mirror this with > from -inf.
 *      Nothing selected gives MIN = +inf, MAX = -inf, IMIN = IMAX = -1.  A NaN, or a d equal to the starting infinity, is
 *      never selected; a NaN value under ALL_DEFINED makes the sums NaN and is never an extreme.  The definition is
 *      independent of order (the kernels break ties by index when they merge).
 *   7. Outputs.  stats is double[nfields][nlev][nrows][8] in the order N, W, S1, S2, MIN, MAX, IMIN, IMAX
 *      (MIFC_HSTATS_N .. MIFC_HSTATS_IMAX) and lives where memkind says; the four slots of a group that is not requested
 *      are not written.  Optional mean (a HOST array of nfields pointers, NULL: none; it requires MOMENTS): mean[f] is
 *      float[nlev][nrows], where memkind says, (float)(pivot + S1 / W), undef where N == 0 or W == 0.0, with
 *      fdefined_mean[f * nlev + k] = checkDefined(rows left undef, nrows) (a HOST int[nfields * nlev]).
 *      What a caller derives from stats: the mean pivot + S1 / W; the variance about the mean S2 / W - (S1 / W)^2; the RMSE
 *      of x - y with pivot 0, sqrt(S2 / W).  When |mean| >> sigma, a second call with pivot = mean removes the
 *      cancellation; both passes stay on the device.
 *   8. Refusals.  A refused call returns 0, writes nothing and gives the reason in mifc_last_error(): nlev < 1; nfields
 *      outside 1..8; nx < 1 or ny < 1; nx * ny > 2^31 - 1; a null pointer that is required; a box that is empty or outside
 *      the grid; an unknown mode; products == 0 or unknown bits; mean without MOMENTS; an output that overlaps an input or
 *      another output by byte range; a bad memkind; a call made while a mifc_graph capture is open.
 * (Restated in numpy in tests/hstats_restate.py.)
 * Device memory is used where it is (16-byte loads where every row of every batch is on the 16-byte grid, else dwords; the
 * result is the same): no copies, one synchronisation at the end.  Host memory works at any size: rows are independent up
 * to rule 4, so the call stages a band of rows of every level at a time, MIFC_HSTATS_CHUNK_MIB of device memory (default
 * 256), and combines the partial sums of all bands at the end -- bit for bit the result of one device call
 * (DESIGN.md 4.22).  Not offered: reduction along y only; products of two fields.  Histograms and percentiles over an area: the
 * mifc_hdist_* entries below.
 * mifc_last_hstats_form: the launch shape of the calling thread's last mifc_hstats_levels call, a diagnostic for tests:
 * "mode=area|rows v=4|1 nf=<fields per launch> w=0|1 minus=0|1 tested=0|1 products=<mask> segs=<segments per row>
 * blocks=<grid.x> launches=<n> bands=<n>" (launches: of the segment kernel); "" before the first call. */
enum { MIFC_HSTATS_AREA = 0, MIFC_HSTATS_ROWS = 1 };
enum { MIFC_HSTATS_MOMENTS = 1, MIFC_HSTATS_EXTREMES = 2 };
enum { MIFC_HSTATS_N = 0, MIFC_HSTATS_W = 1, MIFC_HSTATS_S1 = 2, MIFC_HSTATS_S2 = 3, MIFC_HSTATS_MIN = 4, MIFC_HSTATS_MAX = 5,
       MIFC_HSTATS_IMIN = 6, MIFC_HSTATS_IMAX = 7 };
int mifc_hstats_levels(mifc_ctx* ctx, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields,
                       const float* const* minus, const int* fdefined_minus, const double* pivot, const float* weight,
                       int fdef_weight, const int* box, int mode, int products, double* stats, float* const* mean,
                       int* fdefined_mean, float undef, int memkind);
const char* mifc_last_hstats_form(void);

/* ---- EXTENSION: level batches regridded by a sparse weight table (conservative remapping, region averages) ----
 * Not a miutil::fieldcalc function.  mifc_hinterp_levels samples points, so it cannot conserve a quantity: precipitation,
 * fluxes, cloud cover and land or ice fractions, and any field taken to a coarser grid, are regridded with area-overlap
 * weights, which every regridding tool (ESMF/SCRIP, CDO, xESMF) delivers as a sparse weight table -- one row of
 * (source cell, weight) entries per destination cell, computed once per grid pair and applied at every time step.  The
 * same table form carries first- and second-order conservative remaps, patch recovery, nearest-neighbour remaps, averages
 * over catchments or regions and any other linear horizontal operator.  The result is again a level batch
 * (nlev, ndst_y, ndst_x), which every vertical entry and mifc_hstats_levels accept unchanged.
 *
 * Table.  A table has ndst rows over nsrc = nx * ny source cells, in CSR form: rowptr is int[ndst + 1], col is int[nnz],
 * the flat index j * nx + i, w is float[nnz].  The entries of a row may come in any order and may repeat a column.  The
 * given order is part of the definition.
 * Sums.  Per destination d, field f and level k, entries e = rowptr[d] .. rowptr[d + 1] - 1 in that order:
 *   1. x_e = fields[f][k][col[e]] is defined iff is_defined(fdefined_in[f * nlev + k] == ALL_DEFINED, x_e, undef).  This is
 *      rule 3 of mifc_hinterp_levels: a stored undef under ALL_DEFINED is a value.
 *   2. Sums are in double, sequential, each starting from +0.0.  Every operation is rounded on its own, with no
 *      contraction.  S = S + (double)w_e * (double)x_e over the defined entries; the product is exact.
 *      Wdef = Wdef + (double)w_e over the defined entries.  Wall is the same sum over all entries; it is a property of
 *      the row, computed once when the plan is made.  nbad is the number of undefined entries.
 *   3. MIFC_HREMAP_STRICT = 0: the result is undef if the row is empty or nbad > 0, else (float)S.
 *   4. MIFC_HREMAP_RENORM = 1, with min_frac a double in [0, 1]: an empty row gives undef; nbad == 0 gives (float)S, the
 *      same bits as STRICT; otherwise the result is undef if every entry is undefined, or Wdef == 0.0, or
 *      !(fabs(Wdef) >= min_frac * fabs(Wall)); otherwise the result is (float)((S / Wdef) * Wall).  RENORM is meant for
 *      non-negative weights.
 *   5. fdefined_out[f * nlev + k] = checkDefined(destinations left undef, ndst).  A computed result is never counted,
 *      whatever its value.
 *   6. Consequences: a one-entry row of weight 1 returns the source value bit for bit, except that -0.0 comes back as
 *      +0.0; a NaN under ALL_DEFINED makes the result NaN; there is no tolerance anywhere.
 * (Restated in numpy in tests/hremap_restate.py.)
 *
 * Plan.  mifc_hremap_plan_create is off the hot path: it brings the three arrays to the host whatever their memory kind
 * (memkind says where all three live), then validates them and converts them.  The plan owns its device copy; the caller
 * may free or overwrite its arrays afterwards.  A later kernel reads only memory the library itself validated, so no
 * caller data can send a lane outside [0, nsrc).  Creation is refused with NULL and a reason in mifc_last_error() for:
 * nsrc < 1 or ndst < 1; rowptr[0] != 0, or a decreasing rowptr; nnz = rowptr[ndst] negative; a col outside [0, nsrc); a
 * weight that is NaN or infinite; a null pointer; a bad memkind; an open graph capture.  nnz == 0 is legal: every
 * destination is undef (col and w are not read then and may be NULL).  The device layout is sliced ELL with slices of 64 destinations, padded to the longest row of
 * each slice: one very long row makes its 63 neighbours as long.  mifc_hremap_plan_info gives nnz, the
 * longest row and the number of empty rows (any of the three pointers may be NULL).  A plan belongs to its context, is
 * destroyed before it, and may be used by any number of calls; mifc_hremap_plan_destroy(NULL) does nothing.
 *
 * Entry.  `fields`, `fdefined_in`, nfields (1..8), undef, memkind and pointer alignment are as for mifc_hinterp_levels;
 * fres[f] is [nlev][ndst]; `fdefined_out` a HOST int[nfields * nlev].  Refused calls return 0, write nothing and give the
 * reason in mifc_last_error().  They are: a null plan, or a plan of another context; nx * ny != nsrc of the plan;
 * nlev < 1; nfields outside 1..8; an unknown mode; min_frac NaN or outside [0, 1] (it is ignored but still checked under
 * STRICT); a required null pointer; an output that overlaps a field or another output by byte range; a bad memkind; an
 * open graph capture.
 * Device memory is used where it is, with one synchronisation at the end.  Host memory works at any size: whole levels
 * are staged per chunk, MIFC_HREMAP_CHUNK_MIB of device memory (default 256) but never less than one level.
 * Not offered: a wave-per-row form for very long rows, for which mifc_hstats_levels with a weight plane remains the tool;
 * transposed application; double weights.
 * mifc_last_hremap_form: the launch shape of the calling thread's last mifc_hremap_levels call, a diagnostic for tests:
 * "mode=strict|renorm nf=<fields per launch> tested=0|1 blocks=<grid.x> level_chunks=<grid.y> chunk=<levels per chunk>
 * width=<largest slice width> launches=<n>"; "" before the first call. */
enum { MIFC_HREMAP_STRICT = 0, MIFC_HREMAP_RENORM = 1 };
typedef struct mifc_hremap_plan mifc_hremap_plan;
mifc_hremap_plan* mifc_hremap_plan_create(mifc_ctx* ctx, int nsrc, int ndst, const int* rowptr, const int* col, const float* w, int memkind);
void mifc_hremap_plan_destroy(mifc_hremap_plan* plan);
int mifc_hremap_plan_info(const mifc_hremap_plan* plan, long long* nnz, int* max_row, int* empty_rows);
int mifc_hremap_levels(mifc_ctx* ctx, const mifc_hremap_plan* plan, int nx, int ny, int nlev, const float* const* fields,
                       const int* fdefined_in, int nfields, int mode, double min_frac,
                       float* const* fres, int* fdefined_out, float undef, int memkind);
const char* mifc_last_hremap_form(void);

/* ---- EXTENSION: field expressions over level batches, a register program per cell in one pass ------------------
 * Not a miutil::fieldcalc function.  Field algebra (fieldOPERfield, fieldOPERconstant, constantOPERfield, min/maxvalueField*,
 * abs/log/log10/exp/pow10/powerField) is what callers compose everything with that has no named operator, one field and
 * one operation at a time: a launch and 12 B per cell per operation, every intermediate through memory.  mifc_fexpr_levels
 * evaluates a small register program per cell over level batches in one launch, 4 * (inputs + outputs) bytes per cell.
 * Every operation is rounded exactly as the single-field entry rounds it, so a program made of those operations gives the
 * bits of the chain of calls it replaces (called with SOME_DEFINED flags).
 *   1. Registers.  A cell has MIFC_FEXPR_NREGS = 16 float registers.  Registers 0 .. nfields - 1 start as the cell's value
 *      of fields[f] at this level, the next nplanes registers as the cell's value of planes[p] (the same plane at every
 *      level); the others are unset.  nfields 0..8, nplanes 0..4, nfields + nplanes 1..12.  A program may overwrite input
 *      registers.
 *   2. Instructions.  mifc_fexpr_ins {op, dst, a, b, c}: dst is a register; a source byte is a register (0..15),
 *      MIFC_FEXPR_LEVEL(s), row s of level_scalars (float[nscalars][nlev], nscalars <= 4) at this level, or
 *      MIFC_FEXPR_CONST(j), consts[j] (nconsts <= 16).  Source bytes an operation does not read (b of a one-operand
 *      operation, c of all but SELECT and MASK) and pad are ignored.  ncode 1..64.
 *   3. Operations, one float result each, every one rounded on its own, nothing contracted:
 *        ADD SUB MUL       a op b
 *        DIV               a / b, undef where b == 0 (divideUndef, FieldCalculations.cc:84)
 *        MIN, MAX          b < a ? b : a,  a < b ? b : a (std::min / std::max of minvalueFields, maxvalueFields)
 *        ABS NEG SQRT      of a; SQRT is the correctly rounded float square root
 *        LOG LOG10 EXP POW10   of a, the functions of mifc_logField, mifc_log10Field, mifc_expField, mifc_pow10Field
 *        POW               a ^ b, the function of mifc_powerField (b any operand)
 *        LT LE EQ NE       a op b: 1.0f or 0.0f
 *        MOV               a
 *        SELECT            c != 0 ? a : b; it reads c and the chosen operand only
 *        IFDEF             a where a is defined, else b as it is (b is not tested)
 *        MASK              a as it is where c is defined and c != 0, else undef (a is not tested)
 *   4. Undefined.  There is no defined bit: a register holds undef as a value, and "x is defined" is the library's test
 *      everywhere, !isnan(x) && x != undef.  Except for IFDEF and MASK as said in 3, the result of an operation is undef
 *      if an operand it reads is not defined; otherwise it is the arithmetic result, which may itself be NaN, infinite or
 *      == undef (the next operation then finds it undefined, as a chain of single-field calls would).  Input flags are
 *      not taken: every operand is always tested.
 *   5. Outputs.  fres[o] receives register out_regs[o], o < nout (1..4), after the last instruction.
 *      fdefined_out[o * nlev + k] = checkDefined(cells of output o at level k with value == undef, nx * ny); a NaN is not
 *      counted, as everywhere else.
 *   6. Refused, with 0, nothing written and the reason in mifc_last_error(): an open mifc_graph capture; nlev < 1; counts
 *      outside the limits of 1, 2 and 5; an unknown op; a register or operand index out of range; a register that is read,
 *      by an instruction or by out_regs, before anything set it; a null pointer that is needed; negative nx or ny; more
 *      than 2^31 - 1 cells per level; an unknown memkind; an output that overlaps a field, a plane or another output by
 *      byte range (in place is not offered).  nx * ny == 0 succeeds and writes only flags (ALL_DEFINED).
 * (Restated in numpy in tests/fexpr_restate.py; the program check is mi-fieldcalc_amd/csrc/mifc_fexpr_prog.h.)
 * `fields`, `planes` and `fres` are HOST tables of pointers to memory of `memkind`; level_scalars, consts, code, out_regs
 * and fdefined_out are HOST arrays.  Device memory is used where it is, with one synchronisation at the end: four cells
 * per lane through 16-byte accesses where every pointer is on the 16-byte grid (a level size that is no multiple of four
 * leaves up to three cells per level to a second, small launch), one cell per lane otherwise.  Host memory works at any
 * size, a band of rows of every level at a time in MIFC_FEXPR_CHUNK_MIB of device memory (default 256).
 * mifc_last_fexpr_form: the launch shape of the calling thread's last mifc_fexpr_levels call that launched, a diagnostic
 * for tests: "family=fexpr form=vector|scalar grid=<grid.x> nlev=<grid.y> ncode=<n> nregs=<registers in use> nout=<n>
 * tail=<cells per level of the tail launch> partials=0 tables=0|1 bands=<problems launched>"; "" before the first. */
enum { MIFC_FEXPR_ADD = 0, MIFC_FEXPR_SUB = 1, MIFC_FEXPR_MUL = 2, MIFC_FEXPR_DIV = 3, MIFC_FEXPR_MIN = 4, MIFC_FEXPR_MAX = 5,
       MIFC_FEXPR_ABS = 6, MIFC_FEXPR_NEG = 7, MIFC_FEXPR_SQRT = 8, MIFC_FEXPR_LOG = 9, MIFC_FEXPR_LOG10 = 10, MIFC_FEXPR_EXP = 11,
       MIFC_FEXPR_POW10 = 12, MIFC_FEXPR_POW = 13, MIFC_FEXPR_LT = 14, MIFC_FEXPR_LE = 15, MIFC_FEXPR_EQ = 16, MIFC_FEXPR_NE = 17,
       MIFC_FEXPR_SELECT = 18, MIFC_FEXPR_IFDEF = 19, MIFC_FEXPR_MASK = 20, MIFC_FEXPR_MOV = 21, MIFC_FEXPR_NOPS = 22 };
enum { MIFC_FEXPR_NREGS = 16, MIFC_FEXPR_MAX_FIELDS = 8, MIFC_FEXPR_MAX_PLANES = 4, MIFC_FEXPR_MAX_INPUTS = 12, MIFC_FEXPR_MAX_SCALARS = 4,
       MIFC_FEXPR_MAX_CONSTS = 16, MIFC_FEXPR_MAX_CODE = 64, MIFC_FEXPR_MAX_OUT = 4 };
#define MIFC_FEXPR_LEVEL(s) (16 + (s))
#define MIFC_FEXPR_CONST(j) (32 + (j))
typedef struct { unsigned char op, dst, a, b, c, pad[3]; } mifc_fexpr_ins; /* 8 bytes */
int mifc_fexpr_levels(mifc_ctx* ctx, int nx, int ny, int nlev, const float* const* fields, int nfields, const float* const* planes,
                      int nplanes, const float* level_scalars, int nscalars, const float* consts, int nconsts,
                      const mifc_fexpr_ins* code, int ncode, const int* out_regs, int nout, float* const* fres,
                      int* fdefined_out, float undef, int memkind);
const char* mifc_last_fexpr_form(void);

/* ---- EXTENSION: area histograms and exact percentiles of level batches -----------------------------------------
 * Not a miutil::fieldcalc function.  mifc_hstats_levels stops at counts, sums and extremes; a robust colour scale (the 2 %
 * and 98 % of a level), the area fraction above a threshold, an empirical CDF for quantile mapping, the median and the
 * inter-quartile range of a field or of an error field (mifc_fexpr_levels makes x - y first) and histogram verification
 * need the shape of the distribution, and the reference's callers copy the whole batch to the host for it.  Counts and
 * order statistics do not depend on the order of work: both entries are defined exactly and give the same bits whatever
 * the launch shape, the memory kind or the staging.
 * Common inputs: fields[f], up to 8 batches [nlev][ny][nx], with flags fdefined_in[f * nlev + k] (NULL: SOME_DEFINED);
 * optional mask, a float [ny][nx] shared by all levels and fields, with one flag fdef_mask (the plane a caller passes to
 * mifc_hstats_levels as weight works here: only whether a cell is defined matters); optional box, a HOST
 * int[4] = {i0, i1, j0, j1}, half-open (NULL: the whole level); undef, memkind.
 *   1. Included cell (rule 1 of mifc_hstats_levels without minus).  Cell (j, i) of field f and level k is included iff
 *      i0 <= i < i1 and j0 <= j < j1; x = fields[f][k][j][i] is defined, is_defined(flag == ALL_DEFINED, x, undef) -- a
 *      stored undef or a NaN under ALL_DEFINED is a value --; with mask, mask[j][i] is defined by fdef_mask.
 * mifc_hdist_histogram_levels:
 *   2. Edges.  edges is a HOST float[nfields * nedges], each field with its own edges[f][0 .. nedges), 1 <= nedges <= 1024,
 *      strictly ascending under < (so -0.0 and +0.0 cannot both be edges), none a NaN; -inf and +inf are allowed.
 *   3. Bins.  The bin of an included x that is no NaN is b = #{e : edges[f][e] <= x} with the IEEE comparison: b = 0 below
 *      the first edge, b = nedges at or above the last, -0.0 and +0.0 in the same bin; numpy.searchsorted(edges, x,
 *      side="right").  An included NaN is counted in a slot of its own.
 *   4. Output.  hist is int[nfields][nlev][nrows][nedges + 2], where memkind says: slots 0 .. nedges are the bins, slot
 *      nedges + 1 is the NaN count; excluded cells are counted nowhere (the caller knows the box).  mode is MIFC_HSTATS_AREA
 *      (one result per field and level, nrows = 1) or MIFC_HSTATS_ROWS (one per grid row of the box, nrows = j1 - j0, row r
 *      is grid row j0 + r; the sum over the rows is the AREA result, and on a latitude-longitude grid an exact
 *      area-weighted histogram is a small weighted sum over rows on the caller's side).  Counts fit an int: nx * ny <=
 *      2^31 - 1.
 * mifc_hdist_quantile_levels (AREA only):
 *   5. n is the number of included cells of (field, level).  Order and rank are rules 3 and 4 of mifc_ensembleQuantiles word
 *      for word: the included values sorted ascending in IEEE total order, -0 < +0, every NaN above +inf (the result is
 *      then some NaN); method MIFC_QUANTILE_LOWER, ii = (int)(((float)n * p) / 100.0f) in float, clamped to n - 1, the
 *      result x[ii] bit for bit; MIFC_QUANTILE_LINEAR, h = ((double)(n - 1) * (double)p) / 100.0, k = (int)h, t = h - k,
 *      the result x[k] bit for bit where t == 0, else (float)(x[k] + t * (x[k+1] - x[k])) in double, every operation
 *      rounded, no contraction.  percentiles is a HOST float[nq], 1 <= nq <= 16, each in [0, 100].
 *   6. Output.  quant is float[nfields][nlev][nq], where memkind says, undef where n == 0; quant[f] is a level batch of
 *      shape (nlev, 1, nq).  fdefined_q[f * nlev + k] (HOST) is ALL_DEFINED, or NONE_DEFINED where n == 0.  The result is
 *      defined without reference to any algorithm.
 *   7. Refusals.  A refused call returns 0, writes nothing and gives the reason in mifc_last_error(): nlev < 1; nfields
 *      outside 1..8; nx < 1 or ny < 1; nx * ny > 2^31 - 1; a bad memkind; a box that is empty or outside the grid; an unknown
 *      mode or method; nedges outside 1..1024; nq outside 1..16; a null pointer that is required; an edge that is a NaN or
 *      not above the edge before it (the field and the index are named); a p that is NaN or outside [0, 100]; an output
 *      that overlaps an input by byte range; a call made while a mifc_graph capture is open.
 * (Restated in numpy in tests/hdist_restate.py; the arithmetic of the rules is mi-fieldcalc_amd/csrc/mifc_hdist_rules.h.)
 * Device memory is used where it is (16-byte loads where every row of every batch is on the 16-byte grid, else dwords),
 * with one synchronisation at the end.  Host memory works at any size: counts add, so the histogram stages a band of rows
 * of every level at a time; an order statistic needs all of its level, so the percentiles stage chunks of whole levels,
 * never less than one; both within MIFC_HDIST_CHUNK_MIB of device memory (default 256), which also bounds the counters of
 * the selection.  Not offered: weighted (non-integer) histograms; percentiles per row; two-dimensional
 * (joint) histograms; uniform-bin shortcuts that are not defined by the edge comparisons.
 * mifc_last_hdist_form: the launch shape of the calling thread's last mifc_hdist_* call, a diagnostic for tests:
 * "entry=hist|quant mode=area|rows|lower|linear v=4|1 nf=<fields> nbins=<bins of the histogram, digits of a pass> mask=0|1
 * tested=0|1 prefix=<the fewest key bits that the extremes of a (field, level) share> passes=<the most digit passes a
 * (field, level) needed> launches=<walks over the cells> bands=<n> chunks=<n>"; "" before the first call. */
int mifc_hdist_histogram_levels(mifc_ctx* ctx, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields,
                                const float* edges, int nedges, const float* mask, int fdef_mask, const int* box, int mode, int* hist,
                                float undef, int memkind);
int mifc_hdist_quantile_levels(mifc_ctx* ctx, int nx, int ny, int nlev, const float* const* fields, const int* fdefined_in, int nfields,
                               const float* percentiles, int nq, int method, const float* mask, int fdef_mask, const int* box,
                               float* quant, int* fdefined_q, float undef, int memkind);
const char* mifc_last_hdist_form(void);

/* ---- EXTENSION: trajectories through a series of wind level batches --------------------------------------------
 * Not a miutil::fieldcalc function: the reference's callers carry points along the wind of a level on the host, slice by
 * slice -- where the air of a plume came from, a backward trajectory from every grid cell (an origin map), temperature or
 * humidity along the path.  Every other entry takes the state at one time; this one moves along the time axis.  nt time
 * slices of the wind components u, v ([nlev][ny][nx] each), their times, the map-ratio planes of the stencil operators
 * and npos start positions go in.  Every level carries its own copy of the npos particles: particle (k, p) moves with the
 * wind of level k only.  The index speed of a wind component u is u * xmapr per second (compare 0.5 * xmapr *
 * (f[i+1] - f[i-1]) in the stencil operators), of v it is v * ymapr.  The run goes from slice j_start to slice j_end,
 * forward (j_end > j_start, dir = +1) or backward (dir = -1); nslots = |j_end - j_start| + 1, slot n belongs to slice
 * j_start + n * dir.  xres, yres and tres[f] are [nslots][nlev][npos].
 * Definition.  Every operation is an IEEE double operation rounded on its own, with no contraction; results are bit for
 * bit this definition.  Per particle (k, p):
 *   1. Start.  x = xpos0[p], y = ypos0[p].  Usable is exactly rule 1 of mifc_hinterp_levels: defined, and inside
 *      [0, nx - 1] x [0, ny - 1] in double.  An unusable start makes the particle lost from slot 0 on.  Otherwise slot 0
 *      holds xpos0[p], ypos0[p] bit for bit, and the state is (xd, yd) = ((double)x, (double)y).
 *   2. Sampling a plane at a double position (xd, yd).  First the inside test of rule 1:
 *      xd >= 0.0 && xd <= nx - 1 && yd >= 0.0 && yd <= ny - 1; a NaN fails it.  Then rule 2 of mifc_hinterp_levels gives
 *      i0, j0, a, b; column i0 + 1 is needed only when a != 0, row j0 + 1 only when b != 0.  Rule 3 gives the definedness
 *      of each needed corner under the flag of that plane.  Rule 5 gives the value, without its final rounding to float:
 *      r0 when b == 0, else r0 + b * (r1 - r0).
 *   3. Index velocity G(xd, yd, w) in the interval from slice A to slice B = A + dir.  If the inside test fails, the
 *      particle is lost.  Sample u_A, u_B, v_A, v_B of level k, and xmapr, ymapr, by 2; the planes use flag fdef_map.  Both
 *      slices are needed at every w: if any needed corner of any of the six planes is undefined, the particle is lost.
 *      uu = w == 0 ? u_A : (w == 1 ? u_B : u_A + w * (u_B - u_A)), and vv likewise.  G = (uu * mx, vv * my).
 *   4. Interval.  tau = times[B] - times[A] (negative on a backward run), h = tau / (double)nsub, hh = 0.5 * h,
 *      w_s = (double)s / (double)nsub.  For s = 0 .. nsub - 1: g0 = G(x_s, w_s); x* = x_s + h * g0 (each component); then
 *      niter times: g1 = G(x*, w_{s+1}), then x* = x_s + hh * (g0 + g1) (Petterssen); niter = 0 is the Euler step;
 *      x_{s+1} = x*.  After the last substep the position must pass the inside test, otherwise the particle is lost.
 *   5. Slot.  A particle that survives the interval to slice B writes (float)xd, (float)yd to slot n + 1, and its state
 *      becomes those floats widened again.  Because the state passes through float at every slice, a run j0 -> j2 equals
 *      the run j0 -> j1 followed by a run j1 -> j2 started from slot 1's positions, bit for bit; this also makes the
 *      result independent of how the call is staged.
 *   6. Lost.  A particle lost in the interval n -> n + 1 has undef in xres, yres and every tres[f] at slots n + 1 ..;
 *      its earlier slots stay.
 *   7. Trace.  At every slot where the particle is alive, tres[f] is exactly rules 2-5 of mifc_hinterp_levels, BILINEAR
 *      with a float result, taken from slice j_start + n * dir of trace field f, level k, at the slot's float position.  A
 *      trace hole gives undef at that slot only; the particle is not lost.  By definition it equals a
 *      mifc_hinterp_levels call on that level with nlev = 1, at the positions of that slot.
 *   8. Flags.  g = 0: checkDefined(lost particles at slot n, level k; npos); g = 1 + f: checkDefined(lost + trace holes;
 *      npos).  A computed value is never counted.
 * (Restated in Python in tests/htraj_restate.py; the arithmetic is mi-fieldcalc_amd/csrc/mifc_htraj_rules.h.)
 * Arguments.  `u`, `v`: HOST arrays of nt pointers, one per time slice, each to a [nlev][ny][nx] batch where memkind
 * says.  `fdefined_in`: HOST int[2 * nt * nlev], index (c * nt + t) * nlev + k with c = 0 for u and c = 1 for v; NULL means
 * all SOME_DEFINED.  `times`: HOST double[nt], in seconds.  `xmapr`, `ymapr`: [ny][nx] planes in the memory kind of the
 * fields, flag fdef_map.  `xpos0`, `ypos0`: float[npos], in grid-index units as in mifc_hinterp_levels, in the memory kind
 * of the fields.  `trace`: HOST array of ntrace * nt pointers, index f * nt + t, each to [nlev][ny][nx]; `fdef_trace`: HOST
 * int[ntrace * nt * nlev], index (f * nt + t) * nlev + k, NULL means all SOME_DEFINED.  Only slices between j_start and
 * j_end inclusive are dereferenced.  `tres`: HOST array of ntrace pointers.  `fdefined_out`: HOST
 * int[(1 + ntrace) * nslots * nlev], index (g * nslots + n) * nlev + k; g = 0 is the positions (x and y share it),
 * g = 1 + f is trace field f.  Any alignment of any pointer is accepted.
 * Refused calls return 0, write nothing and give the reason in mifc_last_error().  They are: nt < 2, nlev < 1 or
 * npos < 1; nx < 1 or ny < 1; nx or ny above 2^24 (the bounds must be exact floats, so that rounding a double inside the
 * grid cannot leave it); nx * ny > 2^31 - 1; j_start or j_end outside 0..nt-1, or j_start == j_end; nsub outside 1..64;
 * niter outside 0..8; ntrace outside 0..4; a times[j] in the used range that is not finite, or used times that are not
 * strictly increasing with j; undef >= 0 && undef <= max(nx, ny) - 1 (a computed position could then not be told from a
 * hole; a NaN undef is fine); a required null pointer (trace, tres and fdef_trace may be null when ntrace == 0); an
 * output that overlaps an input or another output by byte range; a bad memkind; a call made while a mifc_graph capture
 * is open.
 * Device memory is used where it is: one launch per interval, queued interval after interval, one synchronisation at
 * the end.  Host memory works at any size, because levels are independent: the call stages a chunk of levels and walks
 * the intervals with two slice buffers (slice B goes up while A stays); the map planes and the start positions go up
 * once, the slots come down.  MIFC_HTRAJ_CHUNK_MIB of device memory (default 256), but never less than one level
 * (DESIGN.md 4.26).
 * mifc_last_htraj_form: the launch shape of the calling thread's last mifc_htraj_levels call, a diagnostic for tests:
 * "niter=<n> nsub=<n> ntrace=<n> tested=0|1 blocks=<grid.x> level_chunks=<grid.y> chunk=<levels per chunk>
 * intervals=<n> launches=<n> staged=<level chunks staged from host, 0 for device memory>"; "" before the first call. */
int mifc_htraj_levels(mifc_ctx* ctx, int nx, int ny, int nlev, int nt, const float* const* u, const float* const* v, const int* fdefined_in,
                      const double* times, const float* xmapr, const float* ymapr, int fdef_map, int npos, const float* xpos0,
                      const float* ypos0, int j_start, int j_end, int nsub, int niter, const float* const* trace, const int* fdef_trace,
                      int ntrace, float* xres, float* yres, float* const* tres, int* fdefined_out, float undef, int memkind);
const char* mifc_last_htraj_form(void);

/* ---- neighbourhood statistics ----------------------------------------------
 * neighbourProbFunctions .h:297 / .cc:2862; neighbourFunctions .h:300 / .cc:2955.  Bit-identical to the
 * reference, its quirks included: the input flag must be ALL_DEFINED; the constants are truncated to int
 * (prob: limit = c[0], range = c[1]; functions, compute < 4: range = c[0], step = c[1] only when
 * nconstants == 2, else 3; compute >= 4: limit = c[0], range = c[1], step = c[2] only when nconstants == 3);
 * the field is compared against (float)limit.  `constants` is always a HOST array.
 *   neighbourProbFunctions: 0/1 per cell (compute 5: field > limit, 6: field < limit); range 0 returns that
 *     field with the flag unchanged (and writes nothing for another compute); otherwise the (2r+1)^2 box
 *     count / N, cells closer than r to the edge undef, flag SOME_DEFINED.  field == fres is allowed.  The
 *     count is exact; the reference's float summed-area table is only while nx * ny <= 2^24.
 *   neighbourFunctions: undef border, then each centre (r, r + step, ... < n - r) writes its value --
 *     compute 1 mean, 2 max, 3 min, 4 percentile c[0], 5 / 6 fraction above / below limit, else +0 -- into
 *     its step x step block; interior cells no block covers keep the caller's content (host memory too).
 * Refused (0, nothing written, mifc_last_error() says why) where the reference is undefined: prob with
 * range < 0 or > nx / ny, prob with compute not 5 / 6 and range > 0, functions with step / 2 > range,
 * a percentile index outside the window, functions with field == fres, a NaN or out-of-int-range constant
 * ("Neighbourhood statistics").  The reference's own `false` leaves mifc_last_error() empty. */
int mifc_neighbourProbFunctions(mifc_ctx* ctx, int nx, int ny, const float* field, const float* constants, int nconstants, int compute,
                                float* fres, int* fdefined, float undef, int memkind);
int mifc_neighbourFunctions(mifc_ctx* ctx, int nx, int ny, const float* field, const float* constants, int nconstants, int compute,
                            float* fres, int* fdefined, float undef, int memkind);
/* Either function over a [nlev][ny][nx] batch in one launch, the scalars shared: `which` is MIFC_NEIGHBOUR_PROB or
 * MIFC_NEIGHBOUR_FUNCTIONS, fdefined[nlev] in/out.  Returns 0 and writes nothing if any level's flag is not
 * ALL_DEFINED. */
enum { MIFC_NEIGHBOUR_PROB = 0, MIFC_NEIGHBOUR_FUNCTIONS = 1 };
int mifc_neighbour_levels(mifc_ctx* ctx, int which, int compute, int nx, int ny, int nlev, const float* field, const float* constants,
                          int nconstants, float* fres, int* fdefined, float undef, int memkind);

/* ---- iterative vessel icing ----------------------------------------------------
 * vesselIcingModStall .h:244 / FieldCalculationsVesselIcing.cc:182; vesselIcingMincog .h:248 / :677 (alt == 1:
 * MINCOG org, anything else: MINCOG adj).  Icing rate in cm/h.  A cell is computed where sal, wave, x_wind, y_wind,
 * airtemp, rh, sst, p, aice and depth are defined (not Pw; no test with an ALL_DEFINED input flag) and aice < 0.4,
 * for MINCOG also sst > -54.1126 sal / (1000 - sal); the flag becomes checkDefined(undefined cells, nx * ny).
 * The reference's `false` (0, nothing written, mifc_last_error() empty): vs, alpha, zmin or zmax negative,
 * zmax < zmin, or zmax - zmin not integral (a NaN among them takes the reference's path).  Refused (0, nothing
 * written, mifc_last_error() says why) where the reference is undefined: (zmax - zmin) * 2 + 1 levels do not fit an
 * int.  `icing` may be any of the inputs: each cell reads only its own index.  At least 99.9 % of the defined cells
 * are bit-identical to the reference, every one within 1e-5 |ref| + 5e-5 cm/h. */
int mifc_vesselIcingModStall(mifc_ctx* ctx, int nx, int ny, const float* sal, const float* wave, const float* x_wind, const float* y_wind,
                             const float* airtemp, const float* rh, const float* sst, const float* p, const float* Pw, const float* aice,
                             const float* depth, float vs, float alpha, float zmin, float zmax, float* icing, int* fdefined, float undef,
                             int memkind);
int mifc_vesselIcingMincog(mifc_ctx* ctx, int nx, int ny, const float* sal, const float* wave, const float* x_wind, const float* y_wind,
                           const float* airtemp, const float* rh, const float* sst, const float* p, const float* Pw, const float* aice,
                           const float* depth, float vs, float alpha, float zmin, float zmax, int alt, float* icing, int* fdefined, float undef,
                           int memkind);
/* Either model over a [nlev][ny][nx] batch (ensemble members, lead times) in one launch, the scalars shared; alt is
 * read by MINCOG only.  Bit k of shared_mask set: input k (0 sal, 1 wave, 2 x_wind, 3 y_wind, 4 airtemp, 5 rh, 6 sst,
 * 7 p, 8 Pw, 9 aice, 10 depth) is ONE [ny][nx] field used by every level (bathymetry, say).  fdefined[nlev] in/out.
 * `icing` may alias a per-level input, not a shared one (refused, device memory). */
enum { MIFC_ICING_MODSTALL = 1, MIFC_ICING_MINCOG = 2 };
int mifc_vesselIcing_levels(mifc_ctx* ctx, int model, int nlev, int nx, int ny, const float* sal, const float* wave, const float* x_wind,
                            const float* y_wind, const float* airtemp, const float* rh, const float* sst, const float* p, const float* Pw,
                            const float* aice, const float* depth, unsigned int shared_mask, float vs, float alpha, float zmin, float zmax, int alt,
                            float* icing, int* fdefined, float undef, int memkind);

/* ---- batched over vertical levels / ensemble members (new surface) ------ */
/* The reference is called once per 2-D field; a caller that wants vorticity
 * AND divergence on nlev levels makes 2*nlev calls.  These
 * entry points do the same work in one fused pass per level-batch.
 *
 * u, v, rvort, diverg : [nlev][ny][nx];  xmapr, ymapr (, fcoriolis) : [ny][nx],
 * shared by all levels.  rvort or diverg may be NULL to skip that output.
 * fdefined : host int[nlev], in = input state per level, out = state of the
 * result(s) of that level -- identical for rvort and diverg because
 * FieldCalculations.cc:1861 and :1927 test the same four neighbours.
 * Result per level is bit-identical to relvort()+divergence() on that level. */
int mifc_vortdiv_levels(mifc_ctx* ctx, int nx, int ny, int nlev, const float* u, const float* v, const float* xmapr, const float* ymapr,
                        float* rvort, float* diverg, int* fdefined, float undef, int memkind);
/* Asynchronous form, device pointers only: enqueues on the context's stream
 * and returns.  `fdefined_in` (host int[nlev], may be NULL = all
 * MIFC_SOME_DEFINED) is read before returning.  `n_undefined_dev` is a device
 * array of nlev 64-bit counters that the call zeroes and the kernel fills;
 * classify each against (nx*ny - 2*nx) with mifc_classify() once the stream
 * has drained.  It may be NULL when every level is MIFC_ALL_DEFINED. */
int mifc_vortdiv_levels_enqueue(mifc_ctx* ctx, int nx, int ny, int nlev, const float* u, const float* v, const float* xmapr, const float* ymapr,
                                float* rvort, float* diverg, const int* fdefined_in, float undef, unsigned long long* n_undefined_dev);

/* The same with explicit level strides (in floats, multiples of 4, >= nx*ny):
 * level l of u / v starts at u + l*in_level_stride, of rvort / diverg at
 * rvort + l*out_level_stride.  A batch whose levels are padded to
 * mifc_batch_level_stride(nx, ny) floats streams through HBM evenly whatever
 * nx*ny is (a level size close to a multiple of 4 MiB makes the
 * eight levels a workgroup walks side by side meet in the same memory channels). */
size_t mifc_batch_level_stride(int nx, int ny);
int mifc_vortdiv_levels_strided_enqueue(mifc_ctx* ctx, int nx, int ny, int nlev, const float* u, const float* v, const float* xmapr,
                                        const float* ymapr, float* rvort, float* diverg, size_t in_level_stride, size_t out_level_stride,
                                        const int* fdefined_in, float undef, unsigned long long* n_undefined_dev);

/* Vorticity, divergence AND the wind speed ff = vectorabs(u, v) (FieldCalculations.cc:1819) of a level batch in one
 * pass: what BASELINE.json config 5 computes per ensemble member from u and v.  As two calls ff reads u and v a second
 * time (12 B per cell); here it is a third output of the fused kernel, computed from the rows that are in LDS anyway
 * (20 B per cell for the three results instead of 16 + 12).  ff : [nlev][ny][nx], every cell (rows 0 and ny-1 included);
 * n_undefined_ff_dev : device u64[nlev], classify against nx*ny (:1839); n_undefined_dev as in
 * mifc_vortdiv_levels_enqueue.  The input flag of a level governs all three results, as it would in the three reference
 * calls.  Per level each result is bit-identical to its reference function.  Launches the three-output kernel does not
 * take (shallow or small batches, nx % 4 != 0, ...) run the pair and a batched vectorabs: same results, two launches. */
int mifc_vortdiv_ff_levels_enqueue(mifc_ctx* ctx, int nx, int ny, int nlev, const float* u, const float* v, const float* xmapr,
                                   const float* ymapr, float* rvort, float* diverg, float* ff, const int* fdefined_in, float undef,
                                   unsigned long long* n_undefined_dev, unsigned long long* n_undefined_ff_dev);

/* Any stencil operator over a batch of levels (generic form of the call above).
 * op selects the reference function:
 *   MIFC_OP_RELVORT .cc:1843, _ABSVORT :1875, _DIVERGENCE :1910, _VORTDIV (both),
 *   MIFC_OP_GRADIENT_X/_Y/_ABS/_LAPLACE = gradient compute 1..4 :1985,
 *   MIFC_OP_GWIND_X :638, _GWIND_Y :674, _GVORT :708, MIFC_OP_IGWIND :1511 (two outputs),
 *   MIFC_OP_JACOBIAN :2424 (f0 = field1, f1 = field2).
 * f0 = u | z | field | mpot, f1 = v (wind operators and the Jacobian); fcoriolis where the
 * operator takes it, else NULL; out1 only for _VORTDIV / _IGWIND.  f0, f1, out0,
 * out1 : [nlev][ny][nx]; xmapr, ymapr, fcoriolis : [ny][nx] shared.
 * fdefined : host int[nlev] in/out, per level exactly as the single-field call. */
enum {
  MIFC_OP_RELVORT = 0, MIFC_OP_ABSVORT = 1, MIFC_OP_DIVERGENCE = 2, MIFC_OP_VORTDIV = 3,
  MIFC_OP_GRADIENT_X = 4, MIFC_OP_GRADIENT_Y = 5, MIFC_OP_GRADIENT_ABS = 6, MIFC_OP_GRADIENT_LAPLACE = 7,
  MIFC_OP_GWIND_X = 8, MIFC_OP_GWIND_Y = 9, MIFC_OP_GVORT = 10, MIFC_OP_IGWIND = 11,
  MIFC_OP_JACOBIAN = 13,
  /* mifc_stencil_levels_ex only: */
  MIFC_OP_ADVECTION = 12, MIFC_OP_TFP = 14, MIFC_OP_QVECTOR = 15, MIFC_OP_SHAPIRO2 = 17
};
int mifc_stencil_levels(mifc_ctx* ctx, int op, int nx, int ny, int nlev, const float* f0, const float* f1, const float* xmapr, const float* ymapr,
                        const float* fcoriolis, float* out0, float* out1, int* fdefined, float undef, int memkind);

/* Asynchronous form of mifc_stencil_levels, device pointers only (the generic form of
 * mifc_vortdiv_levels_enqueue): enqueues on the context's stream and returns; nothing is read back.
 * fdefined_in : host int[nlev] or NULL (= every level MIFC_SOME_DEFINED), read before returning.
 * n_undefined_dev : device array of nlev 64-bit counters, zeroed by the call and filled by the kernel
 * (NULL allowed when every level is MIFC_ALL_DEFINED).  Once the stream has drained the flag of level l
 * is mifc_classify(n_undefined[l], mifc_stencil_count_domain(op, nx, ny)) -- except MIFC_OP_GWIND_X,
 * which is MIFC_NONE_DEFINED whatever the count (FieldCalculations.cc:664).  This is the entry a caller
 * captures into a HIP graph or issues back to back without a host round trip per operator. */
int mifc_stencil_levels_enqueue(mifc_ctx* ctx, int op, int nx, int ny, int nlev, const float* f0, const float* f1, const float* xmapr,
                                const float* ymapr, const float* fcoriolis, float* out0, float* out1, const int* fdefined_in, float undef,
                                unsigned long long* n_undefined_dev);
/* what a level's undefined count of `op` is classified against: nx*ny - 2*nx (FieldCalculations.cc:1868 and
 * friends, also gradient compute 1, :2068), nx*ny for MIFC_OP_IGWIND (:1543) */
unsigned long long mifc_stencil_count_domain(int op, int nx, int ny);

/* Diagnostic: the kernel form the calling thread's last stencil launch took -- "wind_split", "wind_split_ragged",
 * "wind_split_ff", "wind_levelwalk", "wind_rows", "wind_oneshot", "wind_oneshot_tiles", "scalar_split",
 * "scalar_split_ragged", "scalar_levelwalk", "scalar_rows", "scalar_oneshot", "advection_split", "advection_split_ragged", "advection_oneshot", "flat4", "cell"; "" before the first launch.
 * thermalFrontParameter, plevelqvector and shapiro2_filter (single fields and mifc_stencil_levels_ex batches) report the
 * ROUTE of the call instead, set as its last act:
 *   "fused2"            the one-launch two-stage kernel, no level repaired
 *   "fused2_redo"       the same, and at least one level of thermalFrontParameter went again pass by pass (.cc:2286)
 *   "two_stage_passes"  thermalFrontParameter's two passes / plevelqvector's three
 *   "shapiro_fused"     the filter's four sweeps in one launch
 *   "shapiro_sweeps"    the filter's masks plus four sweep launches
 * The tests use it to check that a case reaches the kernel it is meant for; nothing on the data path reads it.  The
 * string is static. */
const char* mifc_last_stencil_form(void);
/* Diagnostic: how the calling thread's last synchronous level-batch call that can stream a host-memory batch through the
 * device in chunks (mifc_vortdiv_levels, mifc_stencil_levels, mifc_stencil_levels_ex, mifc_hlevel_derived_levels,
 * mifc_hlevel_derived_batch and the single-field stencil entries, which share their driver) was run: the number of chunks,
 * and in *levels_per_chunk (NULL allowed) the levels per chunk; 0 and 0 when the batch was staged whole (device memory, a
 * batch below the threshold, MIFC_HOST_PIPELINE=0, a request the pipeline does not carry: advection and the other
 * operators of mifc_stencil_levels_ex, five outputs of the derived batch) or the call was refused.  The
 * tests use it to check that a case went through the pipeline; nothing on the data path reads it. */
int mifc_last_host_chunks(int* levels_per_chunk);
/* The chunking policy of that pipeline for a batch of nlev fields of n cells: the levels per chunk, 0 = staged whole.
 * By default batches from 64 MiB per field are cut into chunks of at most 32 MiB per field (MIFC_HOST_CHUNK_MIB) and
 * nlev / 4 levels; MIFC_HOST_PIPE_MIN_KIB (KiB per field) replaces the threshold, MIFC_HOST_CHUNK_LEVELS sets the levels
 * per chunk (clamped to nlev, no nlev / 4 cap).  Reads the snapshot of the environment that mifc_create and
 * mifc_reload_env take; needs no context and no device. */
int mifc_host_chunk_levels(size_t n, int nlev);
/* Diagnostic: the launch shape of the calling thread's last elementwise (vectorabs, *leveltemp, *levelhum, cvhum, momentum
 * coordinates), catalogue (the other pointwise operators) or fused derived-batch launch, as "key=value" words:
 *   family=ewise|pointwise|derived  op=<kernel instantiation>  form=vector|scalar (four cells per lane | one)
 *   grid=<workgroups of 256 lanes; derived: per level>  partials=0|1 (the undefined counts went through the partials
 *   buffer)  tail=<cells of the extra 64-lane launch>  n=<cells per field>
 * and for family=derived also  nlev=<levels>  inst=ff+rh+theta|ff+rh+theta+td|rh+theta|rh+theta+td|ff|generic
 * check=0|1 (per-cell tests compiled in)  pipe=0|1 (two-trip software pipeline).  A lane of the vector form makes
 * ceil((n / 4) / (grid * 256)) trips at the most.  "" before the first such launch (and after a call that launched
 * nothing the previous report stays).  For tests; nothing on the data path reads it.  The string is thread-local and
 * overwritten by the next query. */
const char* mifc_last_pointwise_form(void);

/* The same plus the rest of the stencil family over a batch of levels, the map
 * and Coriolis fields shared by all levels:
 *   MIFC_OP_ADVECTION .cc:1942  f0 = f, f1 = u, f2 = v, scalar = hours
 *   MIFC_OP_TFP       .cc:2266  f0 = tx                         (thermalFrontParameter)
 *   MIFC_OP_QVECTOR   .cc:505   f0 = z, f1 = t, level_scalars = host float[nlev] pressures p, compute 1..4
 *   MIFC_OP_SHAPIRO2  .cc:2076  f0 = field (out0 == f0 allowed; no map fields)
 * Every other op is forwarded to mifc_stencil_levels.  Per level the result and the flag are those
 * of the single-field reference call; the two-stage operators run as ONE launch per flag group
 * (levels whose input is ALL_DEFINED / the others) with their intermediate fields in LDS. */
int mifc_stencil_levels_ex(mifc_ctx* ctx, int op, int nx, int ny, int nlev, const float* f0, const float* f1, const float* f2, const float* xmapr,
                           const float* ymapr, const float* fcoriolis, const float* level_scalars, float scalar, int compute, float* out0,
                           float* out1, int* fdefined, float undef, int memkind);

/* Fused derived variables on hybrid model levels: one pass producing any of
 *   ff    = vectorabs(u, v)                                   (.cc:1819)
 *   rh    = hlevelhum(t, q, ps, a, b, "", compute=1)  RH in %   (.cc:1145)
 *   theta = hleveltemp(t, ps, a, b, "", compute=3)  T -> theta  (.cc:1046)
 * u, v, t, q, ff, rh, theta : [nlev][ny][nx]; ps : [ny][nx] shared;
 * alevel, blevel : host float[nlev].  Any of ff / rh / theta may be NULL
 * (its inputs are then not read).  fdef_wind / fdef_thermo : host int[nlev]
 * input states of (u,v) and of (t,q,ps); outputs fdef_ff, fdef_rh, fdef_theta
 * : host int[nlev].  Returns 0 if any level has a bad (a,b) pair (.cc:298). */
int mifc_hlevel_derived_levels(mifc_ctx* ctx, int nx, int ny, int nlev, const float* u, const float* v, const float* t, const float* q,
                               const float* ps, const float* alevel, const float* blevel, float* ff, float* rh, float* theta,
                               const int* fdef_wind, const int* fdef_thermo, int* fdef_ff, int* fdef_rh, int* fdef_theta, float undef,
                               int memkind);
/* Asynchronous, device pointers only.  n_undefined_dev: device u64[3*nlev]
 * laid out [ff | rh | theta], zeroed by the call; classify against nx*ny. */
int mifc_hlevel_derived_levels_enqueue(mifc_ctx* ctx, int nx, int ny, int nlev, const float* u, const float* v, const float* t, const float* q,
                                       const float* ps, const float* alevel, const float* blevel, float* ff, float* rh, float* theta,
                                       const int* fdef_wind, const int* fdef_thermo, float undef, unsigned long long* n_undefined_dev);

/* The general form: per level l, any subset of
 *   ff   = vectorabs(u, v)                                               (.cc:1819)
 *   temp = hleveltemp(t, ps, a_l, b_l, temp_unit, temp_compute)          (.cc:1046; compute 1..5)
 *   hum  = hlevelhum(t, h, ps, a_l, b_l, hum_unit, hum_compute)          (.cc:1145; compute 1..12)
 *   hum2 = hlevelhum(t, h, ps, a_l, b_l, hum2_unit, hum2_compute)        a second variant of the SAME inputs,
 *          e.g. hum = RH (compute 1) and hum2 = dew point (compute 9) from T and q
 *   dd   = mifc_winddir(u, v)   EXTENSION, not a reference function (see above): wind direction
 * in ONE pass over u, v, t, h ([nlev][ny][nx]; h = specific humidity or RH as the variants demand; ps [ny][nx]
 * shared).  NULL outputs are skipped (their inputs are not read); unit / compute arguments of a skipped
 * output are ignored.  Results and flags per level are those of the per-level reference calls.  Returns 0
 * where one of those calls would return false (bad (a, b) pair .cc:298, compute out of range) and for
 * temp_compute outside 1..5 (the reference leaves such cells unwritten, .cc:1080-1090).
 * fdef_wind / fdef_thermo: host int[nlev] input states of (u, v) and of (t, h, ps); fdef_ff, fdef_temp,
 * fdef_hum, fdef_hum2, fdef_dd: host int[nlev] results (may be NULL). */
int mifc_hlevel_derived_batch(mifc_ctx* ctx, int nx, int ny, int nlev, const float* u, const float* v, const float* t, const float* h,
                              const float* ps, const float* alevel, const float* blevel, float* ff, float* temp, const char* temp_unit,
                              int temp_compute, float* hum, const char* hum_unit, int hum_compute, float* hum2, const char* hum2_unit,
                              int hum2_compute, float* dd, const int* fdef_wind, const int* fdef_thermo, int* fdef_ff, int* fdef_temp,
                              int* fdef_hum, int* fdef_hum2, int* fdef_dd, float undef, int memkind);
/* Asynchronous, device pointers only.  n_undefined_dev: device u64[5*nlev] laid out
 * [ff | temp | hum | hum2 | dd], zeroed by the call; classify against nx*ny. */
int mifc_hlevel_derived_batch_enqueue(mifc_ctx* ctx, int nx, int ny, int nlev, const float* u, const float* v, const float* t, const float* h,
                                      const float* ps, const float* alevel, const float* blevel, float* ff, float* temp, const char* temp_unit,
                                      int temp_compute, float* hum, const char* hum_unit, int hum_compute, float* hum2, const char* hum2_unit,
                                      int hum2_compute, float* dd, const int* fdef_wind, const int* fdef_thermo, float undef,
                                      unsigned long long* n_undefined_dev);

/* ---- horizontally decomposed single field (row slabs) -------------------- */
/* Vorticity + divergence on one row slab of a larger field (config 4 of
 * BASELINE.json: a 4000x4000 field split over 8 GPUs along y).
 * The slab holds `ny_local` owned rows starting at global row `j0` of a field
 * with `ny_global` rows; u and v point at [ny_local + 2][nx] buffers whose
 * first and last rows are the halo rows (global rows j0-1 and j0+ny_local)
 * filled by the caller's exchange (RCCL send/recv over xGMI; halo content is
 * ignored where it would fall outside the global field).  xmapr, ymapr,
 * rvort, diverg : [ny_local][nx], owned rows only.  The global edge rules of
 * fillEdges (FieldCalculations.cc:59-74) are applied by whichever slab owns
 * the edge rows.  *n_undefined_dev (device u64[1], zeroed by the call)
 * receives this slab's share of the global undefined count; the sum over
 * slabs classifies against nx*ny_global - 2*nx.  Asynchronous, device only. */
int mifc_vortdiv_slab_enqueue(mifc_ctx* ctx, int nx, int ny_global, int j0, int ny_local, const float* u_halo, const float* v_halo,
                              const float* xmapr, const float* ymapr, float* rvort, float* diverg, int fdefined_in, float undef,
                              unsigned long long* n_undefined_dev);

/* The same restricted to the owned rows [row_begin, row_end) of the slab, so that a caller
 * can overlap the halo exchange with compute: enqueue the exchange, launch
 * the interior rows [2, ny_local-2) -- they read no halo row --, wait for the exchange on
 * the stream, launch [0, 2) and [ny_local-2, ny_local).  accumulate_count != 0 leaves
 * *n_undefined_dev as it is and adds to it (zero it with the first launch of a slab only).
 * A range must not separate row 0 from row 1 or row ny_global-1 from row ny_global-2 of
 * the whole field (fillEdges copies one from the other): such a call returns 0. */
int mifc_vortdiv_slab_rows_enqueue(mifc_ctx* ctx, int nx, int ny_global, int j0, int ny_local, int row_begin, int row_end, const float* u_halo,
                                   const float* v_halo, const float* xmapr, const float* ymapr, float* rvort, float* diverg, int fdefined_in,
                                   float undef, unsigned long long* n_undefined_dev, int accumulate_count);
/* ---- launch-bound work as one launch: HIP-graph capture of a sequence of calls ----------------- */
/* The reference is called once per 2-D field; a caller that keeps its loop over levels pays a launch per level for
 * microseconds of traffic (one 1440x720 level of the fused derived kernel: 33 MB = 4 us at peak).  Between
 * mifc_graph_begin and mifc_graph_end the context's ASYNCHRONOUS entry points (mifc_*_enqueue, mifc_slab_plan_begin /
 * _finish) do not run: their launches are recorded with the arguments given; mifc_graph_launch replays the recorded
 * sequence on the context's stream with one runtime call, any number of times (the buffers are read when the graph
 * runs, not when it was recorded).  The synchronous entry points (everything that returns a flag) cannot be recorded:
 * the capture is invalidated and mifc_graph_end returns NULL.  max_levels_per_call: the deepest level batch of the
 * recorded calls (the per-level scratch is sized before the capture starts; 0 = 256).  One capture per context at a
 * time; mifc_set_stream must not be called in between.
 * Lanes: calls that do not depend on each other -- the levels of a caller's loop -- may be recorded side by side
 * (mifc_graph_begin_lanes + mifc_graph_lane(k) before a call): every lane is a chain of its own in the graph, all lanes
 * start together and the graph ends when all have ended, so the launch gaps of one lane are filled by the others.  The
 * caller vouches that calls in different lanes touch different outputs.  Calls that need the context's per-level
 * scratch (stencil batches with mixed flags, derived batches of more than 8 levels) are refused in a multi-lane capture. */
typedef struct mifc_graph mifc_graph;
int mifc_graph_begin(mifc_ctx* ctx, int max_levels_per_call);
int mifc_graph_begin_lanes(mifc_ctx* ctx, int max_levels_per_call, int n_lanes /* 1 .. 16 */);
int mifc_graph_lane(mifc_ctx* ctx, int lane);
mifc_graph* mifc_graph_end(mifc_ctx* ctx);
int mifc_graph_launch(mifc_graph* graph);
void mifc_graph_destroy(mifc_graph* graph);

/* ---- the decomposed step as ONE call (BASELINE.json config 4) --------------- */
/* Communicator: RCCL over xGMI, one process per GPU.  Either the library creates it -- rank 0 calls
 * mifc_comm_unique_id(), the caller distributes the MIFC_COMM_ID_BYTES bytes to every rank by any means it
 * has (MPI, a file, torch.distributed), every rank calls mifc_comm_init() -- or the caller hands over an
 * ncclComm_t it already owns (mifc_comm_adopt: rank and size are read from it; e.g. PyTorch's
 * ProcessGroupNCCL._comm_ptr()).  RCCL is loaded on first use; a process that never calls these never loads it.
 * Slab k of a field lives on rank k: the neighbours of a slab are rank - 1 (above) and rank + 1 (below). */
#define MIFC_COMM_ID_BYTES 128
int mifc_comm_unique_id(char* id_out /* [MIFC_COMM_ID_BYTES] */);
int mifc_comm_init(mifc_ctx* ctx, const char* id /* [MIFC_COMM_ID_BYTES] */, int rank, int world);
int mifc_comm_adopt(mifc_ctx* ctx, void* nccl_comm);
int mifc_comm_release(mifc_ctx* ctx);
/* returns 1 when the context has a communicator; rank / world may be NULL */
int mifc_comm_info(const mifc_ctx* ctx, int* rank, int* world);

/* A plan binds the buffers of one rank's row slab of a level batch:
 *   u_halo, v_halo : [nlev][ny_local + 2][nx], rows 1 .. ny_local of a level owned, rows 0 and ny_local + 1 its
 *                    halo rows (filled by the step from the neighbours; never read at the edges of the whole field)
 *   xmapr, ymapr   : [ny_local][nx] (owned rows, shared by the levels);  rvort, diverg : [nlev][ny_local][nx]
 *   fdefined_in    : input state of every level (MIFC_ALL_DEFINED: no tests, no counters)
 *   n_undefined_dev: device u64[nlev] (NULL allowed for MIFC_ALL_DEFINED)
 * mifc_slab_plan_step() enqueues ONE decomposed step on the context's stream and returns: one row of u and of v per
 * level to / from each neighbour (grouped ncclSend / ncclRecv on a stream of the plan's own), the owned rows that read
 * no halo row meanwhile, then the two boundary strips, then -- tested input, more than one rank -- an ncclAllReduce
 * that leaves the WHOLE field's undefined counts of every level in n_undefined_dev on every rank (classify against
 * nx*ny_global - 2*nx; with one rank or MIFC_ALL_DEFINED nothing is reduced).  Results per level are bit-identical
 * to relvort() + divergence() on the whole field (FieldCalculations.cc:1843-1940), fillEdges included.  The
 * sequence is captured into a HIP graph on the first step and replayed afterwards (MIFC_SLAB_GRAPH=0, or a capture
 * the runtime refuses: enqueued call by call); the buffers, the communicator and the tuning environment are those
 * of the first step.  What the caller wrote to the owned rows of u_halo / v_halo on the context's stream before
 * the call is what is sent. */
typedef struct mifc_slab_plan mifc_slab_plan;
mifc_slab_plan* mifc_slab_plan_create(mifc_ctx* ctx, int nx, int ny_global, int j0, int ny_local, int nlev, float* u_halo, float* v_halo,
                                      const float* xmapr, const float* ymapr, float* rvort, float* diverg, int fdefined_in, float undef,
                                      unsigned long long* n_undefined_dev);
void mifc_slab_plan_destroy(mifc_slab_plan* plan);
int mifc_slab_plan_step(mifc_slab_plan* plan);
/* 1 when the steps replay a captured graph */
int mifc_slab_plan_uses_graph(const mifc_slab_plan* plan);
/* The same step for a caller with a transport of its own (MPI, a host relay, hipMemcpyPeer between the
 * contexts of one process): begin = counters zeroed + the rows that read no halo row; the caller then fills the
 * halo rows, ordered on the context's stream; finish = the boundary strips (the whole slab when it is too thin to
 * split).  Counts stay local: the caller sums them over the slabs. */
int mifc_slab_plan_begin(mifc_slab_plan* plan);
int mifc_slab_plan_finish(mifc_slab_plan* plan);

/* Halo transport for a process that drives several GPUs itself (one context per GPU):
 * copies n_floats from src_dev (memory of src_ctx's device) to dst_dev (dst_ctx's device)
 * over xGMI (hipMemcpyPeerAsync), enqueued on dst_ctx's stream and ordered after the work
 * already queued on src_ctx's stream.  One row of a slab is nx floats.  Processes that own
 * one GPU each exchange the rows with RCCL send/recv instead (mi-fieldcalc_amd/sharding.py,
 * tools/bench_multigpu.py); the slab entry points do not care how the halo rows got there. */
int mifc_halo_copy_enqueue(mifc_ctx* dst_ctx, float* dst_dev, mifc_ctx* src_ctx, const float* src_dev, size_t n_floats);

#ifdef __cplusplus
}
#endif

#endif /* MIFC_H */
