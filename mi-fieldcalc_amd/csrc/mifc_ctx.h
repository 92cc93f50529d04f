// mifc_ctx.h -- internals shared by the host-side translation units of the C
// ABI (mifc_capi.hip and one mifc_capi_<family>.hip per operator family,
// mifc_slab.hip, mifc_graph.hip, ...): the context, the per-call staging of
// host fields and the small helpers every entry point uses, the reference's
// unit / compute remaps among them.  Implemented in mifc_ctx.hip.  Not installed.
#ifndef MIFC_CTX_H
#define MIFC_CTX_H

#include "../../include/mifc.h"
#include "mifc_hostpipe.h"
#include "mifc_kernels.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

using mifc::u64;

struct mifc_ctx
{
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::string err;
  // grow-only device scratch slots, handed out in call order by mifc_host::Staging (the only code that touches them)
  struct Slot
  {
    void* ptr;
    size_t bytes;
  };
  std::vector<Slot> slot;
  size_t slot_cursor = 0; // the next free slot of the running call; 0 between calls
  // per-level flags / counters
  unsigned char* d_flags = nullptr; // 2 * cap_lev bytes (wind | thermo, or just one set)
  u64* d_counts = nullptr;          // 5 * cap_lev
  float* d_ab = nullptr;            // 2 * cap_lev (alevel | blevel; per-level scalars of the batched f1 operators)
  int* d_levels = nullptr;          // cap_lev: level lists of the batched two-stage operators (ALL_DEFINED levels first)
  unsigned int* d_partials = nullptr; // per-workgroup undefined counts of big one-shot launches (grow-only), see mifc_device.h
  size_t partials_cap = 0;
  void* h_pinned = nullptr;         // pinned mirror: counts (3*cap u64) + flags (2*cap) + ab (2*cap float)
  size_t cap_lev = 0;
  // recorded after every async copy that READS the pinned mirror (enqueue
  // variants); waited on before the mirror is rewritten
  hipEvent_t pinned_read = nullptr;
  bool pinned_read_pending = false;
  // recorded after every asynchronous launch that READS the context-owned device scratch
  // (d_flags, d_ab): a switch to another stream makes that stream wait on it before the scratch
  // can be rewritten there (the *_enqueue entry points never synchronise)
  hipEvent_t scratch_read = nullptr;
  bool scratch_read_pending = false;
  // RCCL communicator of the row-slab path (mifc_comm_init / mifc_comm_adopt; mifc_slab.hip): ncclComm_t, its size and
  // this process' rank in it; owned = created by the library (destroyed with the context)
  void* comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  bool comm_owned = false;
  // mifc_counts_accumulate: the *_enqueue entries add to the caller's counters instead of zeroing them first
  bool counts_accumulate = false;
  // mifc_graph_begin .. mifc_graph_end: the *_enqueue calls in between are recorded on capture_stream instead of running
  bool capturing = false;
  hipStream_t capture_stream = nullptr, stream_before_capture = nullptr;
  // lanes of a capture: independent calls recorded side by side (mifc_graph_lane); lane 0 is capture_stream
  std::vector<hipStream_t> lane_streams;
  std::vector<hipEvent_t> lane_events; // [0] fork, [k] join of lane k
  int n_lanes = 1, lane = 0;
  // chunked, full-duplex streaming of host-resident level batches (created on first use)
  mifc::HostPipe* pipe = nullptr;
  // host fields the caller declared constant (mifc_hold_field): device copies that stage_in reuses
  struct HeldField
  {
    const float* host;
    size_t n;
    float* dev;
  };
  std::vector<HeldField> held;
  // measurement aid (mifc_timing_begin / mifc_timing_end_ms): HIP event pairs around every
  // kernel launch of the calls in between, on the stream the kernels are launched on
  static const int NTIMED = 16;
  bool timing = false;
  int n_timed = 0;
  hipEvent_t tev[2 * NTIMED] = {nullptr};
};

namespace mifc_host {

bool fail(mifc_ctx* c, const char* what, hipError_t e);

// Start of every entry point: forget the last error and make the context's device current
// for the calling thread (a process may hold contexts on several GPUs).
inline void enter(mifc_ctx* c)
{
  c->err.clear();
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev != c->device)
    (void)hipSetDevice(c->device);
}

#define MIFC_HIP(c, call)                    \
  do {                                       \
    hipError_t e_ = (call);                  \
    if (e_ != hipSuccess) {                  \
      mifc_host::fail((c), #call, e_);       \
      return 0;                              \
    }                                        \
  } while (0)

// launches wrapped in event pairs while a timing section is open (mifc_timing_begin: the measurement build only)
#ifdef MIFC_MEASUREMENT_BUILD
#define MIFC_LAUNCH(c, call)                                                      \
  do {                                                                            \
    const bool timed_ = (c)->timing && (c)->n_timed < mifc_ctx::NTIMED;           \
    if (timed_)                                                                   \
      (void)hipEventRecord((c)->tev[2 * (c)->n_timed], (c)->stream);              \
    MIFC_HIP(c, call);                                                            \
    if (timed_) {                                                                 \
      (void)hipEventRecord((c)->tev[2 * (c)->n_timed + 1], (c)->stream);          \
      (c)->n_timed += 1;                                                          \
    }                                                                             \
  } while (0)
#else
#define MIFC_LAUNCH(c, call) MIFC_HIP(c, call)
#endif

#define CTX_OR_FAIL(c) \
  if (!(c))            \
    return 0;          \
  mifc_host::enter(c)

bool ensure_levels(mifc_ctx* c, size_t nlev);
// scratch for the per-workgroup counts of a counted one-shot launch over n cells (nullptr below the size where it pays)
unsigned int* partials_for(mifc_ctx* c, size_t n_cells, int* cap);
bool pinned_acquire(mifc_ctx* c);
bool pinned_release(mifc_ctx* c);
bool scratch_release(mifc_ctx* c);
u64* pinned_counts(mifc_ctx* c);
unsigned char* pinned_flags(mifc_ctx* c);
float* pinned_ab(mifc_ctx* c);

// The device homes of one call's host fields.  Every staged field and every scratch block takes the
// context's next slot (each slot an allocation of its own that only grows); the destructor hands the
// slots back.  So a driver called while a caller's Staging is alive continues after the caller's slots
// (the passes of the two-stage operators go through run_stencil() with the batch staged), and calls one
// after the other use the same ones.  A pointer handed out is good until the object goes.  A null pointer, MIFC_MEM_DEVICE
// memory and a host field held by mifc_hold_field pass through and take no slot.
class Staging
{
public:
  Staging(mifc_ctx* c, int memkind) : c_(c), memkind_(memkind), base_(c->slot_cursor) {}
  ~Staging() { c_->slot_cursor = base_; }
  Staging(const Staging&) = delete;
  Staging& operator=(const Staging&) = delete;
  // uploads n floats (asynchronously, on the context's stream) and returns where they are on the device
  const float* in(const float* p, size_t n);
  // a device home for n floats that finish() copies back to p; preload: start from the caller's content
  // (operators that leave cells unwritten)
  float* out(float* p, size_t n, bool preload = false);
  // a block for intermediates, tables or a driver's own sub-allocated staging, whatever the memkind
  void* scratch(size_t bytes);
  // false once a step has failed (the context's error says which); the pointers returned since are null
  bool ok() const { return ok_; }
  // end of the call: the outputs back to the host, then ONE synchronisation of the stream
  bool finish();

private:
  void* take(size_t bytes);
  struct Out
  {
    float* host;
    const void* dev;
    size_t n;
  };
  static const int MAX_OUT = 8;
  mifc_ctx* c_;
  int memkind_;
  size_t base_; // the context's cursor when the call began
  bool ok_ = true;
  int n_out_ = 0;
  Out outs_[MAX_OUT];
};

// mifc_destroy
void free_slots(mifc_ctx* c);

inline size_t align_up(size_t bytes, size_t pow2)
{
  return (bytes + pow2 - 1) & ~(pow2 - 1);
}

// Do [a, a + abytes) and [b, b + bbytes) share a byte?  (Two empty ranges never do, not even at the same address.)
inline bool overlaps(const void* a, size_t abytes, const void* b, size_t bbytes)
{
  const char *pa = static_cast<const char*>(a), *pb = static_cast<const char*>(b);
  return pa < pb + bbytes && pb < pa + abytes;
}

// MetConstants.h:43-53 (host copies, evaluated like the reference does on the CPU)
const float K_CP = 1004.f, K_T0 = 273.15f;
const float K_P0INV = (float)(1. / 1000.0);
const float K_KAPPA = 287.f / 1004.f;

inline bool bad_hlevel(float a, float b) // FieldCalculations.cc:298-301
{
  return (a < 0.0) || (b < 0.0) || (a == 0.0 && b == 0.0) || (b > 1.0);
}

inline bool unit_is(const char* unit, const char* what)
{
  return unit && std::strcmp(unit, what) == 0;
}

// *leveltemp (:340-345, :1060-1065): below compute 3 the unit decides between Celsius and Kelvin
inline int remap_temp_compute(const char* unit, int compute)
{
  if (compute < 3) {
    if (unit_is(unit, "celsius"))
      return 1;
    if (unit_is(unit, "kelvin"))
      return 2;
  }
  return compute;
}

// *levelhum (:422-425, :1174-1177, :1417-1420): the dew-point variants come in a Celsius and a Kelvin numbering
inline int remap_hum_compute(const char* unit, int compute)
{
  if (compute > 8 && unit_is(unit, "celsius"))
    return compute - 4;
  if (compute > 4 && compute <= 8 && unit_is(unit, "kelvin"))
    return compute + 4;
  return compute;
}

inline float hum_tdconv(int compute) // :437, :1181, :1423, after the remap
{
  return (compute >= 9) ? K_T0 : 0;
}

inline int hum_kind_ah(int compute) // numbering of alevelhum / hlevelhum (:1157-1164), after the remap
{
  if (compute <= 2)
    return mifc::HUM_Q_RH;
  if (compute <= 4)
    return mifc::HUM_RH_Q;
  if (compute == 5 || compute == 6 || compute == 9 || compute == 10)
    return mifc::HUM_Q_TD;
  return mifc::HUM_RH_TD;
}

inline bool host_pipeline_enabled()
{
  return mifc::env().host_pipeline; // MIFC_HOST_PIPELINE=0: stage whole batches (for A/B measurements)
}

// what every single-field elementwise call starts from
inline mifc::EwiseParams ewise_base(int op, int nx, int ny, const int* fdefined, float undef)
{
  mifc::EwiseParams P;
  std::memset(&P, 0, sizeof P);
  P.op = op;
  P.n = nx * ny;
  P.all_defined = (*fdefined == MIFC_ALL_DEFINED);
  P.count = 1;
  P.undef = undef;
  P.unit_scale = 100.f;
  return P;
}

} // namespace mifc_host

#endif // MIFC_CTX_H
