// gsr_api.hip -- C ABI of libgsraster.so (include/gsraster.h): context, workspace pool, stage launches.
//
// Host side of the boundary that replaces the reference's third-party `diff_gaussian_rasterization._C`
// (imported at reference gaussian_renderer/__init__.py:14).  No torch linkage: raw device pointers in,
// kernels enqueued on the caller's stream.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <mutex>
#include <thread>
#include <new>
#include <vector>

#include "../../include/gsraster.h"
#include "gsr_kernels.hip.h"
#include "gsr_sort.hip.h"
#include "gsr_knn.hip.h"
#include "gsr_knnq.hip.h"
#include "gsr_pgd.hip.h"
#include "gsr_adam.hip.h"
#include "gsr_densify.hip.h"
#include "gsr_deteval.hip.h"
#include "gsr_groups.hip.h"
#include "gsr_hull.h"
#include "gsr_image.hip.h"
#include "gsr_detect.hip.h"
#include "gsr_detloss.hip.h"
#include "gsr_setdet.hip.h"
#include "gsr_rcnn.hip.h"
#include "gsr_rpn.hip.h"
#include "gsr_fpn.hip.h"
#include "gsr_imgloss.hip.h"
#include "gsr_rpnloss.hip.h"
#include "gsr_objmap.hip.h"

using namespace gsr;

// ---------------------------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int set_err(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

#define HIP_TRY(stage, expr)                                                                          \
  do {                                                                                                \
    hipError_t _e = (expr);                                                                           \
    if (_e != hipSuccess) return set_err(GSR_ERR_DEVICE, "%s: %s (%s)", stage, hipGetErrorString(_e), #expr); \
  } while (0)

#define LAUNCH_CHECK(stage)                                                                       \
  do {                                                                                            \
    hipError_t _e = hipGetLastError();                                                            \
    if (_e != hipSuccess) return set_err(GSR_ERR_DEVICE, "%s: launch failed: %s", stage, hipGetErrorString(_e)); \
  } while (0)

// ---------------------------------------------------------------------------------------------
// workspace pool: grow-only caching of hipMalloc blocks per device; reuse is stream-ordered
// ---------------------------------------------------------------------------------------------
namespace {

struct Block {
  void* p;
  size_t bytes;
  hipStream_t stream;   // stream of the last user
  bool used;
};

struct Pool {
  std::mutex mu;
  std::vector<Block> blocks;
  size_t total = 0;
};

constexpr int MAX_DEV = 32;
Pool g_pool[MAX_DEV];

// Soft cap of a device's pool: beyond it, free blocks last used on OTHER streams are re-used (behind a host-side wait
// for that stream) instead of allocating more.  An eighth of the device's memory (36 GB of an MI355X's 288 GB), at
// least 2 GB; GSR_POOL_CAP_MB overrides.
size_t pool_soft_cap() {
  static const size_t cap = [] {
    if (const char* e = getenv("GSR_POOL_CAP_MB")) { const long long v = atoll(e); if (v > 0) return (size_t)v << 20; }
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || total_b == 0) { (void)hipGetLastError(); return size_t(24) << 30; }
    return std::max<size_t>(total_b / 8, size_t(2) << 30);
  }();
  return cap;
}

int cur_dev() {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess) d = 0;
  return std::min(std::max(d, 0), MAX_DEV - 1);
}

void* pool_alloc(int dev, size_t bytes, hipStream_t st) {
  bytes = std::max<size_t>((bytes + 255) & ~size_t(255), 256);
  Pool& pl = g_pool[dev];
  std::lock_guard<std::mutex> lk(pl.mu);
  // Best fit among the free blocks last used on THIS stream (work enqueued later on the same stream is ordered
  // after the old user by the stream itself).  A block last used on another stream would need a host-side wait
  // for that stream, which would serialise views pipelined over several streams: it is taken only once the pool
  // already holds pool_soft_cap() bytes, otherwise a new block is allocated for this stream.
  int best = -1, other = -1;
  for (size_t i = 0; i < pl.blocks.size(); ++i) {
    const Block& b = pl.blocks[i];
    if (b.used || b.bytes < bytes || b.bytes > bytes + bytes / 2 + (1u << 20)) continue;
    int& slot = (b.stream == st) ? best : other;
    if (slot < 0 || b.bytes < pl.blocks[slot].bytes) slot = (int)i;
  }
  if (best < 0 && other >= 0 && pl.total + bytes > pool_soft_cap()) {
    (void)hipStreamSynchronize(pl.blocks[other].stream);   // cross-stream reuse: wait for the old user
    best = other;
  }
  if (best >= 0) {
    Block& b = pl.blocks[best];
    b.used = true;
    b.stream = st;
    return b.p;
  }
  void* p = nullptr;
  // leave head-room so that a slowly growing pair count re-uses the block instead of reallocating
  const size_t want = bytes + bytes / 8;
  size_t got = want;                                     // what the device allocation really holds
  if (hipMalloc(&p, want) != hipSuccess) {
    (void)hipGetLastError();
    if (other >= 0) {                                    // out of memory: take the other stream's block
      Block& b = pl.blocks[other];
      (void)hipStreamSynchronize(b.stream);
      b.used = true;
      b.stream = st;
      return b.p;
    }
    // give the device back every idle block of this pool (none of them fits), then try once more
    std::vector<Block> keep;
    for (Block& b : pl.blocks) {
      if (b.used) { keep.push_back(b); continue; }
      (void)hipStreamSynchronize(b.stream);
      (void)hipFree(b.p);
      pl.total -= b.bytes;
    }
    pl.blocks.swap(keep);
    if (hipMalloc(&p, want) != hipSuccess) {
      (void)hipGetLastError();
      got = bytes;                                       // no head-room left: the block is recorded at its true size
      if (hipMalloc(&p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
      }
    }
  }
  pl.blocks.push_back(Block{p, got, st, true});
  pl.total += got;
  return p;
}

void pool_free(int dev, void* p) {
  if (!p) return;
  Pool& pl = g_pool[dev];
  std::lock_guard<std::mutex> lk(pl.mu);
  for (Block& b : pl.blocks)
    if (b.p == p) { b.used = false; return; }
}

// A live block is being used on another stream than the one it was taken for (a kept context re-rendered or
// differentiated on stream `st`, ordered behind its earlier users by the caller): when it is freed, stream-ordered reuse
// has to follow THAT stream.
void pool_retag(int dev, void* p, hipStream_t st) {
  if (!p) return;
  Pool& pl = g_pool[dev];
  std::lock_guard<std::mutex> lk(pl.mu);
  for (Block& b : pl.blocks)
    if (b.p == p) { b.stream = st; return; }
}

// A slab = one pool block carved into pieces that start on 256-byte boundaries.  A slab's regions are stated once, as a
// run of take() calls in a function of their own (keep_regions, scratch_regions, seg_regions): on a Slab without a block
// that run is the sizing pass (take hands out null and only advances; block_bytes() is what to ask of the pool), on a
// Slab over the block it hands out the pointers -- so the size and the carving cannot drift apart.  A take that ends
// beyond the block clears `ok`, which the caller turns into a refusal before anything is launched.
struct Slab {
  char* base = nullptr;
  size_t cap = 0, cur = 0;
  bool ok = true;
  Slab() = default;
  Slab(void* blk, size_t bytes) : base(static_cast<char*>(blk)), cap(bytes) {}
  template <typename T>
  T* take(size_t n) {
    cur = (cur + 255) & ~size_t(255);
    T* r = base ? reinterpret_cast<T*>(base + cur) : nullptr;
    cur += n * sizeof(T);
    if (base && cur > cap) ok = false;
    return r;
  }
  size_t block_bytes() const { return cur + 256; }
};

// Host-visible slot of ONE forward's pair count.  The kernel that computes the count (k_storage_scan_hist) stores it
// straight into this pinned, device-mapped host memory and then stores the forward's token behind a system-scope fence;
// the host polls the token.  No copy and no event sits in the stream for it (a 32-byte device-to-host copy is a blit
// kernel plus an event: ~15 us of the forward's critical path, measured).  Slots are pooled and belong to a forward (its
// context, or the call itself when no context is kept), not to the calling thread.
enum { HS_N64 = 0, HS_OVF = 2, HS_TOKEN = 3 };
struct CountSlot {
  volatile uint32_t* host = nullptr;     // 16 words, pinned + mapped
  uint32_t* dev = nullptr;               // the same memory as the device sees it
  uint32_t token = 0;                    // what the forward that owns the slot will write last
};
std::mutex g_slot_mu;
std::vector<CountSlot> g_free_slots;
std::atomic<uint32_t> g_token{1};

bool slot_get(CountSlot& s) {
  bool have = false;
  {
    std::lock_guard<std::mutex> lk(g_slot_mu);
    if (!g_free_slots.empty()) { s = g_free_slots.back(); g_free_slots.pop_back(); have = true; }
  }
  if (!have) {
    void* p = nullptr;
    if (hipHostMalloc(&p, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { (void)hipGetLastError(); return false; }
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, p, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipHostFree(p); return false; }
    s.host = static_cast<volatile uint32_t*>(p);
    s.dev = static_cast<uint32_t*>(d);
    s.host[HS_TOKEN] = 0u;
  }
  uint32_t t = g_token.fetch_add(1);
  if (t == 0u) t = g_token.fetch_add(1);
  s.token = t;
  return true;
}

void slot_put(CountSlot& s) {
  if (!s.host) return;
  std::lock_guard<std::mutex> lk(g_slot_mu);
  g_free_slots.push_back(s);
  s = CountSlot{};
}

inline bool slot_landed(const CountSlot& s) { return s.host[HS_TOKEN] == s.token; }

// Waits until the forward that owns the slot has published its count: spins briefly (the write lands a few tens of
// microseconds after the forward's first kernels), then yields; falls back to a stream synchronise after two seconds.
bool slot_wait(const CountSlot& s, hipStream_t st) {
  for (int i = 0; i < 4000; ++i) {
    if (slot_landed(s)) return true;
    __builtin_ia32_pause();
  }
  const auto t0 = std::chrono::steady_clock::now();
  while (!slot_landed(s)) {
    std::this_thread::yield();
    if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
      if (hipStreamSynchronize(st) != hipSuccess) return false;
      return slot_landed(s);
    }
  }
  return true;
}

// Pair counts seen by earlier forwards, per (device, P, H, W): the capacity guess of an asynchronous-count forward
// (GSR_FLAG_ASYNC_COUNT).  An entry is dropped when a forward overflowed its guess, so the next one counts synchronously.
struct CapKey { int dev, P, H, W; };
struct CapEntry { CapKey k; unsigned long long n; };
std::mutex g_cap_mu;
std::vector<CapEntry> g_caps;

bool cap_lookup(const CapKey& k, unsigned long long& n) {
  std::lock_guard<std::mutex> lk(g_cap_mu);
  for (const CapEntry& e : g_caps)
    if (e.k.dev == k.dev && e.k.P == k.P && e.k.H == k.H && e.k.W == k.W) { n = e.n; return true; }
  return false;
}

void cap_store(const CapKey& k, unsigned long long n, bool erase) {
  std::lock_guard<std::mutex> lk(g_cap_mu);
  for (size_t i = 0; i < g_caps.size(); ++i) {
    const CapKey& q = g_caps[i].k;
    if (q.dev == k.dev && q.P == k.P && q.H == k.H && q.W == k.W) {
      if (erase) { g_caps[i] = g_caps.back(); g_caps.pop_back(); }
      else g_caps[i].n = n;
      return;
    }
  }
  if (!erase) {
    if (g_caps.size() >= 256) g_caps.clear();
    g_caps.push_back(CapEntry{k, n});
  }
}

// Side stream of a caller stream: K1's colour half (SH -> RGB, the bulk of K1's bytes) runs there, beside the binning
// chain of the same view, and is joined before the forward compositor.  One side stream + two events per
// (device, caller stream), created on first use and kept.
struct SideStream { int dev; hipStream_t main, side; hipEvent_t fork, join; };
std::mutex g_side_mu;
std::vector<SideStream> g_sides;

bool side_stream_for(int dev, hipStream_t main, SideStream& out) {
  std::lock_guard<std::mutex> lk(g_side_mu);
  for (const SideStream& s : g_sides)
    if (s.dev == dev && s.main == main) { out = s; return true; }
  SideStream s{dev, main, nullptr, nullptr, nullptr};
  // lowest priority: its one kernel (SH -> RGB) has the whole binning chain's duration to finish in, and must not take
  // wave slots from the chain's short kernels, which sit on the view's critical path
  int least = 0, greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { (void)hipGetLastError(); least = 0; }
  if (hipStreamCreateWithPriority(&s.side, hipStreamNonBlocking, least) != hipSuccess ||
      hipEventCreateWithFlags(&s.fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&s.join, hipEventDisableTiming) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  g_sides.push_back(s);
  out = s;
  return true;
}

// Count slots of forwards whose context was released before the copy landed (forward-only calls with an asynchronous
// count): harvested, without blocking, at the start of later forwards.
struct PendingSlot { CountSlot slot; CapKey key; };
std::mutex g_pending_mu;
std::vector<PendingSlot> g_pending;

void pending_harvest() {
  std::lock_guard<std::mutex> lk(g_pending_mu);
  for (size_t i = 0; i < g_pending.size();) {
    PendingSlot& ps = g_pending[i];
    if (slot_landed(ps.slot)) {
      const unsigned long long n = (unsigned long long)ps.slot.host[HS_N64] | ((unsigned long long)ps.slot.host[HS_N64 + 1] << 32);
      cap_store(ps.key, n, ps.slot.host[HS_OVF] != 0u);
      slot_put(ps.slot);
      g_pending[i] = g_pending.back();
      g_pending.pop_back();
    } else {
      ++i;
    }
  }
}

// ---- per-stage profiling (process-wide: autograd runs backward on its own thread) ------------------
struct ProfSpan { int stage; hipEvent_t a, b; };
std::mutex g_prof_mu;
uint32_t g_prof = 0;   // bit i: stage i is timed
std::vector<ProfSpan> g_spans;
std::vector<hipEvent_t> g_free_events;
float g_ms[GSR_STAGE_COUNT] = {0};
int64_t g_calls[GSR_STAGE_COUNT] = {0};

hipEvent_t get_event_locked() {
  if (!g_free_events.empty()) { hipEvent_t e = g_free_events.back(); g_free_events.pop_back(); return e; }
  hipEvent_t e;
  (void)hipEventCreate(&e);
  return e;
}

struct StageTimer {
  int stage; hipStream_t st; hipEvent_t a{}, b{}; bool on = false;
  // kernel_events: the stage is ONE kernel and the caller hands a and b to hipExtLaunchKernelGGL, which stamps them
  // with the dispatch's own start and end (what a profiler reports as the kernel's duration); events recorded on the
  // stream around a launch also count the time the dispatch waits behind other streams' kernels.
  bool kernel_events;
  StageTimer(int s, hipStream_t stream, bool kernel_ev = false) : stage(s), st(stream), kernel_events(kernel_ev) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    on = (g_prof >> stage) & 1u;
    if (on) { a = get_event_locked(); b = get_event_locked(); if (!kernel_events) (void)hipEventRecord(a, st); }
  }
  ~StageTimer() {
    if (on) {
      if (!kernel_events) (void)hipEventRecord(b, st);
      std::lock_guard<std::mutex> lk(g_prof_mu);
      g_spans.push_back(ProfSpan{stage, a, b});
    }
  }
};

}  // namespace

// ---------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------
// raw parameters of one attribute segment: n Gaussians.  gsr_forward_raw2's second segment (numbered after the first
// P - n Gaussians) travels and is kept as one of these; the raw entry points also describe their first segment with it.
struct RawSeg {
  int32_t n = 0;
  const float *xyz = nullptr, *features_dc = nullptr, *features_rest = nullptr, *objects_dc = nullptr,
              *opacity = nullptr, *scaling = nullptr, *rotation = nullptr;
};

struct GsrCtx {
  int dev = 0;
  GsrSettings st{};
  int P = 0, K = 0;
  int gridx = 0, gridy = 0, ntiles = 0;
  // A batch of views rendered as one virtual scene (gsr_forward_raw_batch; gsr_kernels.hip.h, ViewDev): B views, view v owns
  // the virtual Gaussians [v * Ppad, v * Ppad + P) and the tiles [v * tpv, (v + 1) * tpv); Pv = B * Ppad, ntiles = B * tpv.
  // One view: B = 1, Ppad = Pv = P, tpv = ntiles, vpack = null.
  int B = 1, Ppad = 0, Pv = 0, tpv = 0;
  std::vector<GsrSettings> views;   // B > 1: the views' settings (device pointers owned by the caller); st = views[0]
  ViewDev* vpack = nullptr;
  // Pairs: `nbound` is what the host sized every pair-proportional buffer and grid for -- the exact count when the
  // forward waited for it, the capacity guess of an asynchronous-count forward otherwise; the device-side count lives
  // in dv[DV_N] and reaches the host through `slot` (n_known: already read).
  uint32_t nbound = 0;
  bool n_known = false, overflow = false;
  unsigned long long n64 = 0;
  CountSlot slot;
  hipStream_t fwd_stream = nullptr;   // the forward's stream (fallback of the count wait)
  // inputs (owned by the caller)
  bool raw = false;              // inputs are raw parameters (gsr_forward_raw)
  const float* sh_dc = nullptr;  // raw: _features_dc
  const float *means3D = nullptr, *shs = nullptr, *sh_objs = nullptr, *colors = nullptr, *opac = nullptr,
              *scales = nullptr, *rots = nullptr, *cov3d = nullptr;
  // kept workspace
  void* keep_blk = nullptr;
  void* rank_blk = nullptr;
  void* seg_blk = nullptr;        // boundary records of split tiles (null: no tile is split)
  float4* bnd = nullptr;
  uint32_t* segoff = nullptr;
  uint2* rec_item = nullptr;
  uint32_t seg_shift = 0, rec_cap = 0;
  size_t keep_bytes = 0;
  float4 *G0 = nullptr, *G1 = nullptr, *G2 = nullptr;   // splat records, storage order (the compositors gather them)
  float* D = nullptr;             // [P,9] d rgb / d view direction (lane-group kernels, SH input, backward expected)
  double* abc = nullptr;          // [P] needle marks under GSR_FLAG_NEEDLE_DOUBLE (K1 -> K9; backward expected)
  bool lanegroup = false;         // K1 ran as k_pre_geom + k_pre_color: K8+K9 runs as k_pre_bwd
  uint32_t *order = nullptr, *off = nullptr, *offg = nullptr, *pair_rank = nullptr;
  uint2* ranges = nullptr;
  uint32_t* sched = nullptr;      // [ntiles] tiles longest-list-first + priority class
  float* final_T = nullptr;
  uint32_t* n_contrib = nullptr;
  uint32_t* dv = nullptr;         // device-side scalars of this forward (gsr_sort.hip.h: DV_*)
  // what gsr_ctx_rerender needs beyond the above
  bool async_count = false;       // the forward sized its pair buffers from a guess: K6 looks at dv[DV_OVF]
  bool fwd_only = false;          // kept by gsr_forward_raw2_keep: re-renderable, not differentiable
  bool has_b = false;             // two attribute segments (gsr_forward_raw2_keep): Gaussians >= P - b.n read b
  RawSeg b;
  bool objects_out = false;       // the forward composited the 16 object channels
  bool D_stale = false;           // the last re-render skipped d colour / d direction: no geometry backward until the next
  double* sumsq_out = nullptr;    // gsr_ctx_request_sumsq: where the next overwrite-mode raw backward leaves its six sums of squares
  // depth / alpha maps (gsr_forward*_aux): the forward wrote at least one of them; where (the caller's buffers, used by the
  // forward's K6 launch only); the gradients gsr_ctx_set_aux_grads armed for the next backward
  bool aux = false;
  float *aux_depth_out = nullptr, *aux_alpha_out = nullptr;
  const float *aux_gd = nullptr, *aux_ga = nullptr;
  // which size-gated variants of the binning front end this forward took (gsr_ctx_info 6-9)
  int depth_passes = 0;           // 3 | 4
  int tile_rounds = 0;            // 8 | 16: chunk rounds of k_emit and the tile sort; 0: no pairs
  int scan_items = 0;             // 8 | 16: items per thread of the rank-order scan
  bool group_sums = false;        // K2 read K1's sums through k_bout_group_sum
};

// Host copy of the forward's device-side scalars: waits for the (early) copy if it has not landed yet.
static int ctx_resolve_count(GsrCtx* c) {
  if (c->n_known || !c->slot.host) return GSR_OK;
  if (!slot_wait(c->slot, c->fwd_stream)) return GSR_ERR_DEVICE;
  c->n64 = (unsigned long long)c->slot.host[HS_N64] | ((unsigned long long)c->slot.host[HS_N64 + 1] << 32);
  c->overflow = c->slot.host[HS_OVF] != 0u;
  c->n_known = true;
  const CapKey key{c->dev, c->Pv, c->st.image_height, c->st.image_width};
  cap_store(key, c->n64, c->overflow);
  slot_put(c->slot);
  return GSR_OK;
}

static ViewArgs view_args(const GsrSettings& s) {
  ViewArgs va;
  va.vm = s.viewmatrix; va.pm = s.projmatrix; va.cam = s.campos;
  va.H = s.image_height; va.W = s.image_width;
  va.tanfovx = s.tanfovx; va.tanfovy = s.tanfovy; va.mod = s.scale_modifier; va.deg = s.sh_degree;
  return va;
}

constexpr unsigned long long MAX_PAIRS = 1ull << 31;   // 32-bit pair numbering with head-room

// per-call launch overrides carried in GsrSettings.flags (include/gsraster.h)
static int flag_fwd_npx(uint32_t f) { const int v = (f >> 4) & 7u; return v == 1 ? 1 : v == 2 ? 2 : v == 3 ? 4 : 0; }
static int flag_bwd_npx(uint32_t f) { const int v = (f >> 8) & 3u; return v == 1 ? 2 : v == 2 ? 4 : 0; }
static int flag_tile_map(uint32_t f) { const int v = (f >> 12) & 7u; return (v >= 1 && v <= 4) ? v - 1 : 3; }

static int ceil_log2(uint32_t v) {
  int b = 0;
  while ((1u << b) < v) ++b;
  return b;
}

extern "C" {

const char* gsr_last_error(void) { return g_err; }

void gsr_ctx_free(GsrCtx* c) {
  if (!c) return;
  if (c->slot.host) {                  // the count was never looked at: take it if it has landed, else leave the slot
    if (slot_landed(c->slot)) {                            // to be harvested by a later forward (no host wait here)
      (void)ctx_resolve_count(c);
    } else {
      std::lock_guard<std::mutex> lk(g_pending_mu);
      g_pending.push_back(PendingSlot{c->slot, CapKey{c->dev, c->Pv, c->st.image_height, c->st.image_width}});
      c->slot = CountSlot{};
    }
  }
  pool_free(c->dev, c->keep_blk);
  pool_free(c->dev, c->rank_blk);
  pool_free(c->dev, c->seg_blk);
  delete c;
}

}  // extern "C"

// diagnostic: device buffer [ntiles][2] that the next backward composites stamp with their waves' start/end clocks
static std::atomic<unsigned long long*> g_wave_clock{nullptr};
static std::atomic<unsigned long long*> g_wave_clock_fwd{nullptr};

// ---------------------------------------------------------------------------------------------
// kernel pickers: run-time conditions -> the instantiation to launch.  Each table lists exactly the instantiations that
// exist (the kernels' static_asserts forbid the rest); a launch site calls its picker and launches once.
// ---------------------------------------------------------------------------------------------
template <typename Args>
using Kern = void (*)(Args);   // a kernel that takes its arguments as one struct

// K6.  npx: pixels per lane (1, 2, 4); shared: the tile's 4 / npx waves as one workgroup that stages every batch once
// (k_render_fwd's WPB) -- four pixels per lane have no such form.  wpb == 1: one workgroup of 64 per tile part, else one
// of 64 * wpb per tile.
struct RenderFwdPick { Kern<RenderArgs> kern; int wpb; };
static RenderFwdPick pick_render_fwd(bool obj, int npx, bool shared, bool aux) {
  static constexpr Kern<RenderArgs> table[2][2][5] = {   // [obj][aux][npx 4 | 2 shared | 2 | 1 shared | 1]
      {{k_render_fwd<false, 4>, k_render_fwd<false, 2, 2>, k_render_fwd<false, 2>, k_render_fwd<false, 1, 4>, k_render_fwd<false, 1>},
       {k_render_fwd<false, 4, 1, true>, k_render_fwd<false, 2, 2, true>, k_render_fwd<false, 2, 1, true>,
        k_render_fwd<false, 1, 4, true>, k_render_fwd<false, 1, 1, true>}},
      {{k_render_fwd<true, 4>, k_render_fwd<true, 2, 2>, k_render_fwd<true, 2>, k_render_fwd<true, 1, 4>, k_render_fwd<true, 1>},
       {k_render_fwd<true, 4, 1, true>, k_render_fwd<true, 2, 2, true>, k_render_fwd<true, 2, 1, true>,
        k_render_fwd<true, 1, 4, true>, k_render_fwd<true, 1, 1, true>}}};
  const int form = npx == 4 ? 0 : npx == 2 ? (shared ? 1 : 2) : (shared ? 3 : 4);
  return RenderFwdPick{table[obj][aux][form], (form == 1 || form == 3) ? PXL / npx : 1};
}

// K7.  npx: pixels per lane (4, else 2).  Object channels come first: their walk knows no aux form; without them the aux
// form exists for the geometry walk only and is taken whenever aux gradients are armed (backward_impl has refused the rest).
static Kern<RenderBwdArgs> pick_render_bwd(bool obj, int npx, bool geom, bool aux) {
  static constexpr Kern<RenderBwdArgs> table[2][2][2] = {   // [obj][geom][npx == 4]
      {{k_render_bwd<false, 2, false>, k_render_bwd<false, 4, false>}, {k_render_bwd<false, 2, true>, k_render_bwd<false, 4, true>}},
      {{k_render_bwd<true, 2, false>, k_render_bwd<true, 4, false>}, {k_render_bwd<true, 2, true>, k_render_bwd<true, 4, true>}}};
  static constexpr Kern<RenderBwdArgs> with_aux[2] = {k_render_bwd<false, 2, true, true>, k_render_bwd<false, 4, true, true>};
  return (aux && !obj) ? with_aux[npx == 4] : table[obj][geom][npx == 4];
}

// K8+K9 of the lane-group layouts.  A non-raw context never accumulates; the double needles are looked at only by the
// geometry chain, and not at all by the aux forms (which are geometry chains whatever `geom` says).
static Kern<PreBwdArgs> pick_pre_bwd(bool raw, bool geom, bool acc, bool ndl, bool aux) {
  static constexpr Kern<PreBwdArgs> table[3][3] = {         // [non-raw | raw | raw accumulating][colour only | geometry | ... double needles]
      {k_pre_bwd<false, false>, k_pre_bwd<false, true>, k_pre_bwd<false, true, false, true>},
      {k_pre_bwd<true, false>, k_pre_bwd<true, true>, k_pre_bwd<true, true, false, true>},
      {k_pre_bwd<true, false, true>, k_pre_bwd<true, true, true>, k_pre_bwd<true, true, true, true>}};
  static constexpr Kern<PreBwdArgs> with_aux[3] = {k_pre_bwd<false, true, false, false, true>, k_pre_bwd<true, true, false, false, true>,
                                           k_pre_bwd<true, true, true, false, true>};
  const int row = raw ? (acc ? 2 : 1) : 0;
  return aux ? with_aux[row] : table[row][geom ? (ndl ? 2 : 1) : 0];
}

// K8+K9 of a batch in one launch (the aux form is a geometry chain whatever `geom` says)
static Kern<PreBwdBatchArgs> pick_pre_bwd_batch(bool geom, bool acc, bool aux) {
  static constexpr Kern<PreBwdBatchArgs> table[3][2] = {    // [colour only | geometry | aux][overwrite | accumulate]
      {k_pre_bwd_batch<false, false>, k_pre_bwd_batch<false, true>},
      {k_pre_bwd_batch<true, false>, k_pre_bwd_batch<true, true>},
      {k_pre_bwd_batch<true, false, true>, k_pre_bwd_batch<true, true, true>}};
  return table[aux ? 2 : (geom ? 1 : 0)][acc];
}

// K1, geometry half
static Kern<PreArgs> pick_pre_geom(bool raw, bool needle_double) {
  static constexpr Kern<PreArgs> table[2][2] = {{k_pre_geom<false>, k_pre_geom<false, true>}, {k_pre_geom<true>, k_pre_geom<true, true>}};
  return table[raw][needle_double];
}

// the views' constants of a batch context in one device array (the compositors find a tile's background there)
static void launch_pack_views(const GsrCtx* c, hipStream_t st) {
  ViewPtrs vp{};
  for (int v = 0; v < c->B; ++v) {
    const GsrSettings& sv = c->views[v];
    vp.vm[v] = sv.viewmatrix; vp.pm[v] = sv.projmatrix; vp.cam[v] = sv.campos; vp.bg[v] = sv.bg;
    vp.tanfovx[v] = sv.tanfovx; vp.tanfovy[v] = sv.tanfovy;
  }
  hipLaunchKernelGGL(k_pack_views, dim3(c->B), dim3(64), 0, st, vp, c->B, c->vpack);
}

// Arguments of K1's colour half from a context, for k_pre_color (PreArgs: view 0, or the only one) and for
// k_pre_color_batch: the one or two segments' positions and SH coefficients, the records, D.  Which Gaussians emit pairs
// the kernel reads from `tcnt` (the forward, whose geometry half has just written it) or, tcnt == null, from the kept offg.
template <typename Args>
static void fill_color_inputs(const GsrCtx* c, uint32_t* tcnt, Args& a) {
  a.P = c->P; a.means = c->means3D; a.sh = c->shs; a.sh_dc = c->sh_dc;
  a.Pa = c->has_b ? c->P - c->b.n : c->P; a.means_b = c->has_b ? c->b.xyz : nullptr;
  a.sh_b = c->has_b ? c->b.features_rest : nullptr; a.sh_dc_b = c->has_b ? c->b.features_dc : nullptr;
  a.tcnt = tcnt; a.offg = tcnt ? nullptr : c->offg;
  a.G1 = c->G1; a.G2 = c->G2; a.D = c->D;
}
static PreArgs color_args(const GsrCtx* c, uint32_t* tcnt) {
  PreArgs a{};
  fill_color_inputs(c, tcnt, a);
  a.va = view_args(c->st); a.G0 = c->G0;
  return a;
}
static PreColorBatchArgs color_batch_args(const GsrCtx* c, uint32_t* tcnt) {
  PreColorBatchArgs a{};
  fill_color_inputs(c, tcnt, a);
  a.B = c->B; a.Ppad = c->Ppad; a.deg = c->st.sh_degree; a.vpack = c->vpack;
  return a;
}

// K6 of a context whose binning (pair list, tile ranges, schedule, boundary-record plan) and splat records are in place:
// the last launch of a forward, and all that a re-render of a kept context needs behind the colour kernel.
static int launch_render_fwd(GsrCtx* c, float* out_color, float* out_objects, hipStream_t st) {
  const GsrSettings* s = &c->st;
  const int W = s->image_width, H = s->image_height, ntiles = c->ntiles;
  const size_t HW = (size_t)H * W;
  const float* sh_objs = out_objects ? c->sh_objs : nullptr;
  RenderArgs ra;
  ra.ranges = c->ranges; ra.pair_rank = c->pair_rank; ra.R0 = c->G0; ra.R1 = c->G1; ra.R2 = c->G2;
  ra.sh_objs = sh_objs; ra.bg = s->bg; ra.W = W; ra.H = H; ra.gridx = c->gridx; ra.ntiles = ntiles;
  ra.sh_objs_b = c->has_b ? c->b.objects_dc : nullptr; ra.Pa = c->has_b ? c->P - c->b.n : c->P;
  ra.map_mode = flag_tile_map(s->flags);
  ra.sched = c->sched;
  ra.dv = c->async_count ? c->dv : nullptr;
  ra.wave_clock = g_wave_clock_fwd.load();
  ra.bnd = c->bnd; ra.segoff = c->bnd ? c->segoff : nullptr; ra.seg_shift = c->bnd ? c->seg_shift : 0u;
  ra.out_color = out_color; ra.out_objects = out_objects; ra.final_T = c->final_T; ra.n_contrib = c->n_contrib;
  ra.tpv = c->tpv; ra.vpack = c->vpack; ra.Ppad = c->Ppad;
  ra.out_depth = c->aux_depth_out; ra.out_alpha = c->aux_alpha_out;
  const bool aux = ra.out_depth != nullptr || ra.out_alpha != nullptr;
  // pixels per lane of K6: fewer = more, shorter waves per tile (see k_render_fwd); images with fewer tiles than
  // half the chip's wave slots are split down to one 16x4 strip per wave.  GSR_FLAG_FWD_SPLIT(n) overrides.
  // From 32 000 tiles on (a 4K image, a batch of four or more 1080p views) one wave per tile: four rounds of waves fill the
  // chip either way, and a tile's list is then staged once instead of once per half tile (S-airport-4K K6 0.215 -> 0.207 ms,
  // an 8-view batch of S-nyc-1M 0.140 -> 0.129 ms per view).  Below that the longer work items cost more in the kernel's
  // tail than they save: 8160 tiles 0.196 -> 0.268 ms, an 8-view batch of S-hydrant-full (20 000 tiles) 0.042 -> 0.061.
  const int fwd_npx = flag_fwd_npx(s->flags) ? flag_fwd_npx(s->flags) : (ntiles < 4096 ? 1 : (ntiles < 32000 ? 2 : 4));
  const dim3 gridT(render_grid(ntiles * (PXL / fwd_npx)));
  // the tile's waves as one workgroup that stages every batch once (k_render_fwd's WPB): S-nyc-1M gathers 596 -> 367 MB
  // but runs 0.197 -> 0.224 ms (two workgroup barriers per batch, and the waves of a tile wait for each other), so
  // it is opt-in: GSR_FLAG_FWD_SHARED, or GSR_K6_SHARED=1 in the environment
  static const int k6_env = [] { const char* e = getenv("GSR_K6_SHARED"); return e ? atoi(e) : 0; }();
  const bool k6_shared = k6_env != 0 || (s->flags & GSR_FLAG_FWD_SHARED) != 0;
  const dim3 gridS(render_grid(ntiles));
  const bool obj = out_objects && sh_objs;
  if (out_objects && !obj) {
    hipError_t e = hipMemsetAsync(out_objects, 0, sizeof(float) * NUM_OBJ * HW * (size_t)c->B, st);   // (a batch: [B,16,H,W])
    if (e != hipSuccess) return set_err(GSR_ERR_DEVICE, "objects: %s", hipGetErrorString(e));
  }
  const RenderFwdPick k6 = pick_render_fwd(obj, fwd_npx, k6_shared, aux);
  hipLaunchKernelGGL(k6.kern, k6.wpb > 1 ? gridS : gridT, dim3(64 * k6.wpb), 0, st, ra);
  LAUNCH_CHECK("render forward");
  return GSR_OK;
}

// One forward, as every forward entry point hands it to forward_impl (filled member by member, under the entry point's
// own parameter names where they differ: raw_call).
struct FwdCall {
  const GsrSettings* s = nullptr;   // nviews > 1 (gsr_forward_raw_batch): `s` points at nviews settings; the batch is one
  int nviews = 1;                   // virtual scene (GsrCtx::B)
  int32_t P = 0, K = 0;
  // inputs.  raw: scales / rotations / opacities are the reference model's RAW parameters, shs is _features_rest and
  // sh_dc is _features_dc (K must be 16); activations and their chain rule run inside K1 / K9.
  const float *means3D = nullptr, *shs = nullptr, *sh_dc = nullptr, *sh_objs = nullptr, *colors_precomp = nullptr,
              *opacities = nullptr, *scales = nullptr, *rotations = nullptr, *cov3D_precomp = nullptr;
  const RawSeg* segb = nullptr;     // second attribute segment (gsr_forward_raw2*), counted in P
  bool raw = false, fwd_only = false;   // fwd_only: no backward state is kept (gsr_forward_raw2*)
  // outputs; out_depth / out_alpha: the _aux entry points' maps (either may be null)
  float *out_color = nullptr, *out_objects = nullptr, *out_depth = nullptr, *out_alpha = nullptr;
  int32_t* radii = nullptr;
  GsrCtx** ctx_out = nullptr;
  int64_t* num_rendered = nullptr;
  void* stream = nullptr;
};

// ---------------------------------------------------------------------------------------------
// The forward.  forward_impl (at the end of this section) is its table of contents: check, plan, allocate and carve,
// then one member of FwdRun per pipeline stage.  A new buffer goes into ONE of the region functions (keep_regions,
// scratch_regions, seg_regions); a new stage is one more `int FwdRun::x()` and one more line of forward_impl.
// ---------------------------------------------------------------------------------------------
static int tiles_across(int px) { return (px + TILE - 1) / TILE; }
// a batch: B views as one virtual scene of B * Ppad Gaussians and B * tpv tiles (a batch of one is an ordinary forward)
static int batch_views(const FwdCall& f) { return (f.nviews > 1 && f.P > 0) ? f.nviews : 1; }
static int batch_pad(int32_t P, int B) { return B > 1 ? (int)(((size_t)P + BATCH_PAD - 1) / BATCH_PAD * BATCH_PAD) : P; }

// every refusal of a forward's arguments: nothing has been allocated or launched
static int check_forward(const FwdCall& f) {
  const GsrSettings* const s = f.s;
  const int32_t P = f.P, K = f.K;
  const bool want_aux = f.out_depth != nullptr || f.out_alpha != nullptr;
  if (want_aux && s && (s->flags & GSR_FLAG_NEEDLE_DOUBLE))
    return set_err(GSR_ERR_INVALID, "gsr_forward_aux: depth / alpha maps are not available under GSR_FLAG_NEEDLE_DOUBLE");
  if (want_aux && (f.segb || f.fwd_only))
    return set_err(GSR_ERR_INVALID, "gsr_forward_aux: depth / alpha maps are not available from the two-segment forwards");
  if (!s || !f.out_color) return set_err(GSR_ERR_INVALID, "gsr_forward: null settings / out_color");
  if (P < 0 || s->image_height <= 0 || s->image_width <= 0)
    return set_err(GSR_ERR_INVALID, "gsr_forward: bad sizes P=%d H=%d W=%d", P, s->image_height, s->image_width);
  if (P > 0) {   // an empty scene carries no data pointers: it renders the background
    if (!f.radii || !f.means3D || !f.opacities)
      return set_err(GSR_ERR_INVALID, "gsr_forward: null means3D / opacities / radii");
    if ((f.shs == nullptr) == (f.colors_precomp == nullptr))
      return set_err(GSR_ERR_INVALID, "gsr_forward: provide exactly one of shs / colors_precomp");
    const bool has_sr = f.scales != nullptr && f.rotations != nullptr;
    if (((f.scales != nullptr) != (f.rotations != nullptr)) || (has_sr == (f.cov3D_precomp != nullptr)))
      return set_err(GSR_ERR_INVALID, "gsr_forward: provide exactly one of (scales, rotations) / cov3D_precomp");
  }
  if (P > 0 && f.shs && (s->sh_degree < 0 || s->sh_degree > 3 || K < (s->sh_degree + 1) * (s->sh_degree + 1)))
    return set_err(GSR_ERR_INVALID, "gsr_forward: sh_degree %d needs K >= %d, got K=%d (degree must be 0..3)",
                   s->sh_degree, (s->sh_degree + 1) * (s->sh_degree + 1), K);
  if (!s->bg || !s->viewmatrix || !s->projmatrix || !s->campos)
    return set_err(GSR_ERR_INVALID, "gsr_forward: settings tensors (bg, viewmatrix, projmatrix, campos) must be device pointers");
  const int gridx = tiles_across(s->image_width), gridy = tiles_across(s->image_height);
  if (gridx > 4095 || gridy > 4095) return set_err(GSR_ERR_INVALID, "gsr_forward: image larger than 65520 px per side");
  const int B = batch_views(f);
  if ((size_t)B * (size_t)batch_pad(P, B) > (size_t)RANK_MASK)
    return set_err(GSR_ERR_INVALID, "gsr_forward: more than 2^28 Gaussians (times views of a batch)");
  if ((size_t)B * (size_t)(gridx * gridy) >= (size_t)SCHED_TILE_MASK) return set_err(GSR_ERR_INVALID, "gsr_forward: more than 2^28 tiles in the batch");
  return GSR_OK;
}

// The sizes of one forward and the variants it takes: host arithmetic on the call's arguments, plus the pair count an
// earlier forward of the same (P, H, W) left behind.
struct FwdPlan {
  int32_t P = 0, K = 0;
  int H = 0, W = 0, gridx = 0, gridy = 0;
  int B = 1, Ppad = 0, Pv = 0, tpv = 0, ntiles = 0;   // GsrCtx has their meaning
  size_t HW = 0;                    // pixels of all views
  size_t Pp = 1;                    // max(Pv, 1): what the per-Gaussian regions are sized for
  uint32_t nbP = 0;                 // chunks of the storage scan / depth sort
  uint32_t nk1 = 0, nk1v = 0;       // workgroups of K1's geometry half: all views, per view
  uint32_t nkc = 0;                 // ... of its colour half, per view
  uint32_t ngroups = 0;
  int depth_passes = 3;
  bool group_sums = false;          // K2 reads K1's sums through group sums (k_bout_group_sum)
  bool lanegroup = false, want_D = false, want_abc = false, needle_double = false;
  int cull = 1;
  bool async_count = false;
  unsigned long long cap_pairs = MAX_PAIRS - 1;
  const float* sh_objs = nullptr;   // the call's, or null where the object channels are not wanted
};

static FwdPlan plan_forward(const FwdCall& f, int dev) {
  const GsrSettings* const s = f.s;
  FwdPlan p;
  p.P = f.P; p.K = f.K;
  // objects not wanted -- unless the features are to be kept for the backward (GSR_FLAG_OBJECTS_FOR_BACKWARD_ONLY)
  p.sh_objs = (f.out_objects == nullptr && !(s->flags & GSR_FLAG_OBJECTS_FOR_BACKWARD_ONLY)) ? nullptr : f.sh_objs;
  p.H = s->image_height; p.W = s->image_width;
  p.gridx = tiles_across(p.W); p.gridy = tiles_across(p.H);
  p.tpv = p.gridx * p.gridy;                                           // tiles per view
  p.B = batch_views(f);
  p.Ppad = batch_pad(p.P, p.B);
  p.Pv = p.B > 1 ? p.B * p.Ppad : p.P;                                 // virtual Gaussians
  p.ntiles = p.B * p.tpv;                                              // virtual tiles
  p.HW = (size_t)p.H * p.W * (size_t)p.B;
  p.Pp = (size_t)std::max(p.Pv, 1);
  // Asynchronous pair count (GSR_FLAG_ASYNC_COUNT, or GSR_ASYNC_COUNT=1 in the environment): the host does not wait
  // for the pair count; buffers and grids are sized from the count an earlier forward of the same (P, H, W) saw, with
  // head-room.  Without such an entry this forward counts synchronously (and leaves the entry behind).
  static const int async_env = [] { const char* e = getenv("GSR_ASYNC_COUNT"); return e ? atoi(e) : 0; }();
  if (p.P > 0 && (async_env != 0 || (s->flags & GSR_FLAG_ASYNC_COUNT))) {
    unsigned long long seen = 0;
    if (cap_lookup(CapKey{dev, p.Pv, p.H, p.W}, seen)) {
      p.cap_pairs = std::min<unsigned long long>(seen + seen / 4 + 65536ull, MAX_PAIRS - 1);
      p.async_count = true;
    }
  }
  // the SH layouts the reference uses (and precomputed colours) take the lane-group kernels
  p.lanegroup = f.raw || (f.shs && p.K == 16) || f.colors_precomp != nullptr;
  p.want_D = p.lanegroup && f.shs != nullptr && f.ctx_out != nullptr && !f.fwd_only;
  p.needle_double = (s->flags & GSR_FLAG_NEEDLE_DOUBLE) != 0u;
  p.want_abc = p.needle_double && p.lanegroup && f.ctx_out != nullptr && !f.fwd_only;
  p.cull = (s->flags & GSR_FLAG_NO_CULL) ? 0 : 1;
  p.nbP = (uint32_t)((p.Pp + DCHUNK - 1) / DCHUNK);
  p.nk1 = (uint32_t)((p.Pp + PREG_BLOCK - 1) / PREG_BLOCK);
  p.nk1v = p.B > 1 ? (uint32_t)(p.Ppad / PREG_BLOCK) : p.nk1;
  p.nkc = (uint32_t)(((size_t)std::max(p.P, 1) + PREF_BLOCK - 1) / PREF_BLOCK);
  // the depth sort: three passes of <= 11 bits (a latency-bound million keys) or four of <= 8 (several million: throughput)
  static const int depth_passes_env = [] { const char* e = getenv("GSR_DEPTH_PASSES"); int v = e ? atoi(e) : 0; return (v == 3 || v == 4) ? v : 0; }();
  p.depth_passes = depth_passes_env ? depth_passes_env : (p.Pp >= (size_t(3) << 20) ? 4 : 3);
  p.group_sums = p.nk1 > K1_GROUP_MIN;
  p.ngroups = (p.nk1 + K1_GROUP - 1) / K1_GROUP;
  return p;
}

// ---- the forward's three slabs: each region list stands here once (see Slab) -------------------------------------
// the kept slab: what the context holds until gsr_ctx_free
static void keep_regions(Slab& s, const FwdPlan& p, GsrCtx* c) {
  c->G0 = s.take<float4>(REC * p.Pp);   // G records (storage order): interleaved, REC float4 apart
  c->G1 = c->G0 ? c->G0 + 1 : nullptr; c->G2 = c->G0 ? c->G0 + 2 : nullptr;
  c->order = s.take<uint32_t>(p.Pp); c->off = s.take<uint32_t>(p.Pp + 1); c->offg = s.take<uint32_t>(p.Pp + 1);
  c->ranges = s.take<uint2>(p.ntiles); c->final_T = s.take<float>(p.HW); c->n_contrib = s.take<uint32_t>(p.HW);
  c->dv = s.take<uint32_t>(DV_WORDS);
  c->sched = s.take<uint32_t>(p.ntiles);
  c->D = p.want_D ? s.take<float>(9 * p.Pp) : nullptr;
  c->abc = p.want_abc ? s.take<double>(p.Pp) : nullptr;
  c->vpack = p.B > 1 ? s.take<ViewDev>((size_t)p.B) : nullptr;
}

// the scratch slab: released at the end of the forward
struct FwdScratch {
  uint32_t *dkey = nullptr, *k1 = nullptr, *vtmp = nullptr, *v2 = nullptr, *tcnt = nullptr, *table = nullptr, *tsums = nullptr;
  uint4* bout = nullptr;
  uint32_t* psums = nullptr;
  uint4* gsum = nullptr;            // null unless FwdPlan::group_sums
  uint8_t* tcnt8 = nullptr;
};

static void scratch_regions(Slab& s, const FwdPlan& p, FwdScratch& w) {
  w.dkey = s.take<uint32_t>(p.Pp); w.k1 = s.take<uint32_t>(p.Pp); w.vtmp = s.take<uint32_t>(p.Pp);
  w.v2 = s.take<uint32_t>(p.Pp); w.tcnt = s.take<uint32_t>(p.Pp);
  w.table = s.take<uint32_t>((size_t)RS_BINS_DEV * p.nbP); w.tsums = s.take<uint32_t>(RS_BINS_DEV);
  w.bout = s.take<uint4>(p.nk1);
  w.psums = s.take<uint32_t>(p.nbP + 2);
  w.gsum = p.group_sums ? s.take<uint4>(p.ngroups) : nullptr;
  w.tcnt8 = s.take<uint8_t>(p.Pp);
}

// the segment slab: boundary records of split tiles, for c->rec_cap records (kept with the context)
static void seg_regions(Slab& s, GsrCtx* c) {
  c->bnd = s.take<float4>((size_t)c->rec_cap * PXL * 64); c->rec_item = s.take<uint2>(c->rec_cap);
  c->segoff = s.take<uint32_t>(c->ntiles);
}

// What one forward holds while it runs -- the context it is filling and everything transient -- and its stages, in the
// order forward_impl runs them.
struct FwdRun {
  const FwdCall& f;
  const FwdPlan& p;
  int dev;
  hipStream_t st;
  GsrCtx* c = nullptr;
  void* scratch_blk = nullptr;
  FwdScratch w;
  // The pair-proportional pool blocks of a forward with nbound > 0 pairs: (tile key, depth rank) arrays A and B for the
  // tile sort to alternate between -- the rank array it ends in stays with the context -- and the sort's table, which
  // also holds the sums and chunk_first (ngrain entries).
  uint32_t *tileA = nullptr, *rankA = nullptr, *tileB = nullptr, *rankB = nullptr, *tableN = nullptr;
  int rounds = 0, tile_bits = 0;
  uint32_t nbN = 0, ngrain = 0;
  uint32_t* tsumsN() const { return tableN + RS_BINS * nbN; }
  uint32_t* chunk_first() const { return tsumsN() + RS_BINS; }
  SideStream side{};
  bool side_used = false;

  int allocate();            // the context, its kept slab, the scratch slab
  int preprocess();          // P > 0: K1 (its colour half forked off: fork_color) and the storage scan
  int fork_color();
  int depth_sort();
  int pair_count();
  int empty_scene();         // P = 0, instead of the three above
  int take_pair_buffers();   // nbound > 0: these three
  int emit();
  int tile_sort();
  int render();              // joins the colour half; segments, tile schedule, K6
  // the forward failed with `code`: nothing of it may outlive its workspace
  int abandon(int code) {
    if (side_used) (void)hipStreamWaitEvent(st, side.join, 0);
    pool_free(dev, scratch_blk);
    for (void* b : {(void*)tableN, (void*)tileA, (void*)rankA, (void*)tileB, (void*)rankB})
      if (!(c && b == c->rank_blk)) pool_free(dev, b);
    gsr_ctx_free(c);
    return code;
  }
};

int FwdRun::allocate() {
  c = new (std::nothrow) GsrCtx();
  if (!c) return set_err(GSR_ERR_NOMEM, "gsr_forward: host allocation failed");
  c->dev = dev; c->st = *f.s; c->P = p.P; c->K = p.K; c->gridx = p.gridx; c->gridy = p.gridy; c->ntiles = p.ntiles;
  c->B = p.B; c->Ppad = p.Ppad; c->Pv = p.Pv; c->tpv = p.tpv;
  if (p.B > 1) c->views.assign(f.s, f.s + p.B);
  c->means3D = f.means3D; c->shs = f.shs; c->sh_objs = p.sh_objs; c->colors = f.colors_precomp; c->opac = f.opacities;
  c->scales = f.scales; c->rots = f.rotations; c->cov3d = f.cov3D_precomp;
  c->raw = f.raw; c->sh_dc = f.sh_dc;
  c->fwd_only = f.fwd_only; c->objects_out = f.out_objects != nullptr && p.sh_objs != nullptr;
  c->aux = f.out_depth != nullptr || f.out_alpha != nullptr; c->aux_depth_out = f.out_depth; c->aux_alpha_out = f.out_alpha;
  if (f.segb) { c->has_b = true; c->b = *f.segb; }
  c->lanegroup = p.lanegroup;
  c->depth_passes = p.depth_passes; c->group_sums = p.group_sums; c->scan_items = scan_items_for((uint32_t)p.Pv);
  Slab ksize, ssize;
  keep_regions(ksize, p, c);
  scratch_regions(ssize, p, w);
  c->keep_bytes = ksize.block_bytes();
  c->keep_blk = pool_alloc(dev, c->keep_bytes, st);
  scratch_blk = pool_alloc(dev, ssize.block_bytes(), st);
  if (!c->keep_blk || !scratch_blk)
    return set_err(GSR_ERR_NOMEM, "gsr_forward: workspace allocation failed (P=%d, %dx%d)", p.P, p.W, p.H);
  Slab ks(c->keep_blk, c->keep_bytes), ss(scratch_blk, ssize.block_bytes());
  keep_regions(ks, p, c);
  scratch_regions(ss, p, w);
  if (!ks.ok || !ss.ok) return set_err(GSR_ERR_STATE, "gsr_forward: a workspace region ends beyond its block");
  return GSR_OK;
}

// K1's colour half (SH -> RGB): on the side stream, beside the binning chain, unless the caller turned that off
// (GSR_FLAG_NO_SIDE_STREAM / GSR_SIDE_STREAM=0).  render() joins it.
int FwdRun::fork_color() {
  static const int side_env = [] { const char* e = getenv("GSR_SIDE_STREAM"); return e ? atoi(e) : 1; }();
  hipStream_t cs = st;
  if (side_env != 0 && !(f.s->flags & GSR_FLAG_NO_SIDE_STREAM) && side_stream_for(dev, st, side)) {
    HIP_TRY("side stream", hipEventRecord(side.fork, st));
    HIP_TRY("side stream", hipStreamWaitEvent(side.side, side.fork, 0));
    cs = side.side;
    side_used = true;
  }
  // beside the chain: a thin grid (COLOR_BLOCKS workgroups looping over the chunks); alone: one per chunk
  constexpr unsigned COLOR_BLOCKS = 512;
  const dim3 gridC(side_used ? std::min<unsigned>(p.nkc, COLOR_BLOCKS) : p.nkc), blkCol(PREF_BLOCK);
  // a batch of views: ONE launch reads every SH row once for all the views that see the Gaussian
  if (p.B > 1) hipLaunchKernelGGL(k_pre_color_batch, gridC, blkCol, 0, cs, color_batch_args(c, w.tcnt));
  else hipLaunchKernelGGL(f.raw ? k_pre_color<true> : k_pre_color<false>, gridC, blkCol, 0, cs, color_args(c, w.tcnt));
  if (side_used) HIP_TRY("side stream", hipEventRecord(side.join, side.side));
  return GSR_OK;
}

// K1 (geometry half, colour half forked off), then the storage scan: storage-order numbering of the pairs (where the
// backward puts its partial rows), the depth sort's digit width and first histogram, the device-side pair count --
// published to the host slot by the kernel itself: one launch
int FwdRun::preprocess() {
  const int ntiles = p.ntiles;
  StageTimer t(GSR_STAGE_PREPROCESS, st);
  PreBlockOut bo;
  bo.bout = w.bout;
  bo.ranges = p.P >= p.tpv ? c->ranges : nullptr;     // the tile ranges are cleared by K1's first threads
  bo.ntiles = p.tpv;
  if (!bo.ranges) {                                   // fewer Gaussians than tiles: spans (0xFFFFFFFF, 0) by two fills
    HIP_TRY("ranges", hipMemset2DAsync(c->ranges, sizeof(uint2), 0xFF, sizeof(uint32_t), ntiles, st));
    HIP_TRY("ranges", hipMemset2DAsync(reinterpret_cast<char*>(c->ranges) + sizeof(uint32_t), sizeof(uint2), 0, sizeof(uint32_t), ntiles, st));
  }
  if (p.B > 1) launch_pack_views(c, st);
  if (c->lanegroup) {
    // (a batch: ONE launch of the geometry kernel over the B views' padded ranges -- view = workgroup / workgroups per
    // view; everything behind K1 then runs once over the B * Ppad virtual Gaussians.)
    PreArgs pa = color_args(c, w.tcnt);      // what the colour half reads; the geometry half adds:
    pa.Pfill = p.B > 1 ? p.Ppad : p.P; pa.vpack = p.B > 1 ? c->vpack : nullptr; pa.bpv = (int)p.nk1v;
    pa.scales = f.scales; pa.rots = f.rotations; pa.cov3d = f.cov3D_precomp; pa.opac = f.opacities;
    pa.colors = f.colors_precomp; pa.radii = f.radii; pa.dkey = w.dkey; pa.tcnt8 = w.tcnt8; pa.abc = c->abc;
    pa.scales_b = f.segb ? f.segb->scaling : nullptr; pa.rots_b = f.segb ? f.segb->rotation : nullptr;
    pa.opac_b = f.segb ? f.segb->opacity : nullptr;
    pa.cull = p.cull; pa.bo = bo;
    hipLaunchKernelGGL(pick_pre_geom(f.raw, p.needle_double), dim3(p.nk1), dim3(PREG_BLOCK), 0, st, pa);
    if (!f.colors_precomp) { const int rcol = fork_color(); if (rcol != GSR_OK) return rcol; }
  } else {
    hipLaunchKernelGGL(k_preprocess, dim3(p.nk1v), dim3(PREG_BLOCK), 0, st, p.P, p.K, view_args(*f.s),
                       (p.cull ? 1 : 0) | (p.needle_double ? 2 : 0), f.means3D, f.scales, f.rotations, f.cov3D_precomp,
                       f.opacities, f.shs, f.colors_precomp, f.radii, c->G0, c->G1, c->G2, w.dkey, w.tcnt, bo);
  }
  // stream capture (hipGraph): the forward must not wait for anything, so the count has to be asynchronous, and it is
  // not published to the host at all (a replayed graph would keep writing into a slot that has long been recycled)
  hipStreamCaptureStatus cap_st = hipStreamCaptureStatusNone;
  const bool capturing = hipStreamIsCapturing(st, &cap_st) == hipSuccess && cap_st == hipStreamCaptureStatusActive;
  if (capturing && !p.async_count)
    return set_err(GSR_ERR_STATE, "gsr_forward: a stream capture needs GSR_FLAG_ASYNC_COUNT and an earlier forward of "
                   "the same (P, H, W) on this device (the pair count cannot be waited for while capturing)");
  if (!capturing && !slot_get(c->slot)) return set_err(GSR_ERR_NOMEM, "gsr_forward: pinned host slot allocation failed");
  c->fwd_stream = st;
  if (p.group_sums) hipLaunchKernelGGL(k_bout_group_sum, dim3(p.ngroups), dim3(K1_GROUP), 0, st, (const uint4*)w.bout, p.nk1, w.gsum);
  hipLaunchKernelGGL(k_storage_scan_hist, dim3(p.nbP), dim3(256), 0, st, (uint32_t)p.Pv, (const uint32_t*)w.tcnt, (const uint32_t*)w.dkey,
                     (const uint4*)w.bout, (const uint4*)w.gsum, c->offg, w.table, p.nbP, c->dv, p.cap_pairs, c->slot.dev, c->slot.token,
                     (uint32_t)p.depth_passes);
  LAUNCH_CHECK("preprocess");
  return GSR_OK;
}

// Stable argsort of the live depth keys in passes whose digit width the device chose from the keys' range:
// order[r] = Gaussian of depth rank r, r < V = dv[DV_V].  Pass 0 drops the Gaussians that emit nothing (its
// histogram came from k_storage_scan_hist), the last pass also gathers cnt[r] = tiles touched by rank r.
int FwdRun::depth_sort() {
  StageTimer t(GSR_STAGE_DEPTH_SORT, st);
  const uint32_t Pv = (uint32_t)p.Pv;
  const uint32_t* nV = c->dv + DV_V;
  uint8_t* const cnt8 = c->lanegroup ? w.tcnt8 : nullptr;
  DigitSpec d0{c->dv, 0, 0, 0u}, d1{c->dv, 1, 0, 0u}, d2{c->dv, 2, 0, 0u};
  if (p.depth_passes == 4) {
    // millions of keys (a batch of views, a large scene): four passes of <= 8 bits through the 256-bin kernels; passes
    // 1-3 in the chunk size the tile sort would pick for that many keys
    DigitSpec d3{c->dv, 3, 0, 0u};
    const int rn = radix_rounds_for(Pv);
    radix_pass<RS_BINS>(w.dkey, nullptr, w.k1, w.vtmp, Pv, nullptr, d0, DROUNDS, w.table, w.tsums, false, 1, 1,
                        c->dv + DV_V, nullptr, nullptr, st);
    radix_pass<RS_BINS>(w.k1, w.vtmp, w.dkey, w.v2, Pv, nV, d1, rn, w.table, w.tsums, true, 0, 0, nullptr, nullptr, nullptr, st);
    radix_pass<RS_BINS>(w.dkey, w.v2, w.k1, w.vtmp, Pv, nV, d2, rn, w.table, w.tsums, true, 0, 0, nullptr, nullptr, nullptr, st);
    radix_pass<RS_BINS>(w.k1, w.vtmp, nullptr, c->order, Pv, nV, d3, rn, w.table, w.tsums, true, 0, 0, nullptr, w.tcnt, w.v2, st,
                        nullptr, 0, cnt8);
  } else {
    radix_pass<RS_BINS_DEV>(w.dkey, nullptr, w.k1, w.vtmp, Pv, nullptr, d0, DROUNDS, w.table, w.tsums, false, 1, 1,
                            c->dv + DV_V, nullptr, nullptr, st);
    radix_pass<RS_BINS_DEV>(w.k1, w.vtmp, w.dkey, w.v2, Pv, nV, d1, DROUNDS, w.table, w.tsums, true, 0, 0, nullptr, nullptr,
                            nullptr, st);
    radix_pass<RS_BINS_DEV>(w.dkey, w.v2, nullptr, c->order, Pv, nV, d2, DROUNDS, w.table, w.tsums, true, 0, 0, nullptr,
                            w.tcnt, w.vtmp, st, nullptr, 0, cnt8);
  }
  LAUNCH_CHECK("depth sort");
  return GSR_OK;
}

// nbound: what every pair-proportional buffer and grid is sized for -- the exact count, waited for, or the guess
int FwdRun::pair_count() {
  uint32_t nbound = 0;
  if (!p.async_count) {
    // (the rank-order scan is enqueued after this wait: it records the owners of the emission chunks' first slots, an
    // array sized by N; the depth sort keeps the GPU busy well past the host's wake-up)
    if (ctx_resolve_count(c) != GSR_OK) return set_err(GSR_ERR_DEVICE, "gsr_forward: reading the pair count failed");
    if (c->n64 >= MAX_PAIRS)   // NSUB * N must stay below 2^32
      return set_err(GSR_ERR_NOMEM, "gsr_forward: %llu (tile, Gaussian) pairs exceed the supported %llu "
                     "(splats cover too many tiles: check scales / scale_modifier)", c->n64, MAX_PAIRS);
    nbound = (uint32_t)c->n64;
  } else {
    nbound = (uint32_t)p.cap_pairs;
  }
  c->nbound = nbound;
  c->async_count = p.async_count;
  if (nbound == 0) HIP_TRY("init", hipMemsetAsync(c->off, 0, sizeof(uint32_t), st));
  return GSR_OK;
}

// P = 0: no pairs, every tile's span empty; the compositor paints the background
int FwdRun::empty_scene() {
  const int ntiles = c->ntiles;
  HIP_TRY("init", hipMemsetAsync(c->off, 0, sizeof(uint32_t), st));
  HIP_TRY("init", hipMemsetAsync(c->offg, 0, sizeof(uint32_t), st));
  HIP_TRY("init", hipMemsetAsync(c->dv, 0, sizeof(uint32_t) * DV_WORDS, st));
  HIP_TRY("ranges", hipMemsetAsync(c->ranges, 0, sizeof(uint2) * ntiles, st));
  c->n_known = true;
  return GSR_OK;
}

int FwdRun::take_pair_buffers() {
  const uint32_t nbound = c->nbound;
  c->tile_rounds = rounds = radix_rounds_for(nbound);
  const uint32_t chunkN = (uint32_t)rs_chunk(rounds);
  nbN = (nbound + chunkN - 1) / chunkN;
  for (uint32_t** b : {&tileA, &rankA, &tileB, &rankB}) {
    *b = static_cast<uint32_t*>(pool_alloc(dev, sizeof(uint32_t) * (size_t)nbound, st));
    if (!*b) return set_err(GSR_ERR_NOMEM, "gsr_forward: pair buffers (N=%u) allocation failed", nbound);
  }
  ngrain = nbound / EMIT_GRAIN + 4;
  tableN = static_cast<uint32_t*>(pool_alloc(dev, sizeof(uint32_t) * ((size_t)(RS_BINS * nbN) + RS_BINS + ngrain), st));
  if (!tableN) return set_err(GSR_ERR_NOMEM, "gsr_forward: sort table allocation failed");
  tile_bits = ceil_log2((uint32_t)c->ntiles + 1);             // keys are 0..ntiles (ntiles = culled pair)
  return GSR_OK;
}

// The rank-order scan -- off[r] = pairs emitted by the ranks in front of r, off[V] = their total; chunk_first[c] = rank
// that owns slot c * EMIT_GRAIN -- and the emission of the (tile, rank) pairs.
int FwdRun::emit() {
  StageTimer t(GSR_STAGE_BIN, st);
  // (two launches: block sums, then carry + local scan.  Round 3's one-launch variant, in which a block waited for its
  // predecessors' published sums, saved 2.4 us and could, in principle, give up waiting with nothing but a poisoned
  // image to show for it: removed)
  scan_exclusive_u32(p.depth_passes == 4 ? w.v2 : w.vtmp, c->off, (uint32_t)p.Pv, c->dv + DV_V, w.psums, st, chunk_first(),
                     (uint32_t)EMIT_GRAIN, ngrain);
  LAUNCH_CHECK("rank scan");
  int sh0; uint32_t mask0;
  radix_first_digit(tile_bits, sh0, mask0);
  // a batch: the view of a virtual Gaussian is g / Ppad (one multiply by ceil(2^32 / Ppad) and one correction)
  const uint32_t e_ppad = p.B > 1 ? (uint32_t)p.Ppad : 0u;
  const uint32_t e_magic = p.B > 1 ? (uint32_t)(((1ull << 32) + (uint64_t)p.Ppad - 1ull) / (uint64_t)p.Ppad) : 0u;
  const bool rmin = rounds == RS_ROUNDS_MIN;
  hipLaunchKernelGGL(rmin ? k_emit<RS_ROUNDS_MIN> : k_emit<RS_ROUNDS_MAX>, dim3(nbN),
                     dim3(rs_chunk(rmin ? RS_ROUNDS_MIN : RS_ROUNDS_MAX) / EMIT_PER_THREAD), 0, st, (const uint32_t*)c->off, (const uint32_t*)c->order,
                     (const uint32_t*)chunk_first(), (const uint32_t*)c->dv, (const float4*)c->G0, (const float4*)c->G1, (const float4*)c->G2,
                     p.gridx, p.W, p.H, (uint32_t)p.ntiles, p.cull, tileA, rankA, tableN, nbN, mask0, e_ppad, e_magic,
                     (uint32_t)p.tpv);
  LAUNCH_CHECK("emit");
  return GSR_OK;
}

// The pairs sorted by tile (stable: depth order within a tile survives), the tiles' spans found on the way.  The rank
// array the sort ended in stays with the context; the other pair buffers and the table go back to the pool.
int FwdRun::tile_sort() {
  int res;
  {
    StageTimer t(GSR_STAGE_TILE_SORT, st);
    res = radix_sort_pairs(tileA, rankA, tileB, rankB, c->nbound, c->dv + DV_N, 0, tile_bits, false, tableN, tsumsN(), st, true,
                           reinterpret_cast<uint32_t*>(c->ranges), (uint32_t)c->ntiles);
    LAUNCH_CHECK("tile sort");
  }
  c->pair_rank = res ? rankB : rankA;
  c->rank_blk = c->pair_rank;
  pool_free(dev, tableN);
  for (uint32_t* k : {tileA, rankA, tileB, rankB}) if (k != c->pair_rank) pool_free(dev, k);
  tableN = tileA = rankA = tileB = rankB = nullptr;
  return GSR_OK;
}

// The boundary-record plan of split tiles, the tile schedule, K6.
int FwdRun::render() {
  if (side_used) HIP_TRY("side stream", hipStreamWaitEvent(st, side.join, 0));   // the colours are in place from here on
  StageTimer t(GSR_STAGE_RENDER_FWD, st);
  // Long tile lists are split into segments for the backward (gsr_kernels.hip.h, "Segments"): the forward stores the
  // per-pixel (T, C) at the segment boundaries -- with object channels too (round 5): a backward without dL/dobjects then
  // still walks segments; one WITH dL/dobjects ignores the records (the 16 running object sums are not stored).  Not
  // for a forward-only call, not under GSR_FLAG_NO_SEGMENTS.
  static const int seg_shift_env = [] { const char* e = getenv("GSR_SEG_SHIFT"); int v = e ? atoi(e) : 8; return (v >= 6 && v <= 16) ? v : 8; }();
  if (c->nbound > 0 && f.ctx_out && !f.fwd_only && !(f.s->flags & GSR_FLAG_NO_SEGMENTS)) {
    const uint32_t per = c->nbound >> seg_shift_env;
    c->seg_shift = (uint32_t)seg_shift_env;
    // sum over split tiles of ceil(len / seg) <= N / seg + min(T, N / seg): every split tile's records always fit
    c->rec_cap = per + std::min<uint32_t>((uint32_t)p.ntiles, per) + 1u;
    Slab gsize;
    seg_regions(gsize, c);
    c->seg_blk = pool_alloc(dev, gsize.block_bytes(), st);
    if (!c->seg_blk) return set_err(GSR_ERR_NOMEM, "gsr_forward: segment boundary buffer (N=%u) allocation failed", c->nbound);
    Slab gs(c->seg_blk, gsize.block_bytes());
    seg_regions(gs, c);
    if (!gs.ok) return set_err(GSR_ERR_STATE, "gsr_forward: a segment region ends beyond its block");
  }
  // always: it also turns the empty spans the tile sort left untouched into (0, 0)
  // (more than 64 KB of dynamic LDS at 4K: a single workgroup may use all of the CU's 160 KB on gfx950)
  // If the limit cannot be raised the lengths of the tiles beyond the default 64 KB's worth are read from HBM instead.
  static const int sched_lds_cap = [] {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_tile_schedule),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, 2 * SCHED_LDS_TILES);
    (void)hipGetLastError();
    return e == hipSuccess ? SCHED_LDS_TILES : SCHED_LDS_TILES_DEFAULT;
  }();
  static const int batch_sched_env = [] { const char* e = getenv("GSR_BATCH_SCHED"); return e ? atoi(e) : 0; }();
  hipLaunchKernelGGL(k_tile_schedule, dim3((c->segoff ? 2 : 1) * p.B), dim3(1024), sched_lds_bytes(p.tpv, sched_lds_cap), st, p.tpv,
                     sched_lds_cap, c->ranges, c->sched, c->seg_shift, c->segoff, c->rec_item, c->rec_cap, c->dv + DV_NREC, p.B,
                     batch_sched_env);
  LAUNCH_CHECK("tile schedule");
  const int rk6 = launch_render_fwd(c, f.out_color, f.out_objects, st);
  if (rk6 != GSR_OK) return rk6;
  c->aux_depth_out = nullptr; c->aux_alpha_out = nullptr;      // the caller's buffers: written once, by this launch
  return GSR_OK;
}

static int forward_impl(const FwdCall& f) {
  if (f.ctx_out) *f.ctx_out = nullptr;
  if (const int rc = check_forward(f)) return rc;
  const int dev = cur_dev();
  pending_harvest();
  const FwdPlan p = plan_forward(f, dev);
  FwdRun run{f, p, dev, static_cast<hipStream_t>(f.stream)};
  int r;
  if ((r = run.allocate()) != GSR_OK) return run.abandon(r);
  if (p.P > 0) {
    if ((r = run.preprocess()) != GSR_OK) return run.abandon(r);
    if ((r = run.depth_sort()) != GSR_OK) return run.abandon(r);
    if ((r = run.pair_count()) != GSR_OK) return run.abandon(r);
  } else {
    if ((r = run.empty_scene()) != GSR_OK) return run.abandon(r);
  }
  if (run.c->nbound > 0) {
    if ((r = run.take_pair_buffers()) != GSR_OK) return run.abandon(r);
    if ((r = run.emit()) != GSR_OK) return run.abandon(r);
    if ((r = run.tile_sort()) != GSR_OK) return run.abandon(r);
  }
  if ((r = run.render()) != GSR_OK) return run.abandon(r);
  GsrCtx* c = run.c;
  pool_free(dev, run.scratch_blk);
  if (f.num_rendered) *f.num_rendered = c->n_known ? (int64_t)c->n64 : (int64_t)-1;   // -1: not known yet (asynchronous count)
  if (f.ctx_out) *f.ctx_out = c; else gsr_ctx_free(c);
  return GSR_OK;
}

// The raw entry points name their inputs as the reference model does (RawSeg); this is where those names meet
// forward_impl's.  P: the Gaussians of the call (those of `a`, plus the second segment's when there is one).
static void set_raw_inputs(FwdCall& f, int32_t P, const RawSeg& a) {
  f.P = P; f.K = 16; f.raw = true;
  f.means3D = a.xyz; f.sh_dc = a.features_dc; f.shs = a.features_rest; f.sh_objs = a.objects_dc;
  f.opacities = a.opacity; f.scales = a.scaling; f.rotations = a.rotation;
}

static bool raw_seg_complete(const RawSeg& a) {
  return a.xyz && a.features_dc && a.features_rest && a.opacity && a.scaling && a.rotation;
}

// What a batch's views must look like: 1..MAX_BATCH of them, each with its device tensors, agreeing in image size, scale
// modifier, SH degree and flags (cameras, tan(fov / 2) and backgrounds are per view).  `fn` names the entry point.
static int check_batch_views(const char* fn, const GsrSettings* s, int32_t B) {
  if (!s || B < 1 || B > MAX_BATCH) return set_err(GSR_ERR_INVALID, "%s: 1..%d views, got %d", fn, MAX_BATCH, B);
  for (int v = 0; v < B; ++v) {
    if (!s[v].bg || !s[v].viewmatrix || !s[v].projmatrix || !s[v].campos)
      return set_err(GSR_ERR_INVALID, "%s: view %d: settings tensors (bg, viewmatrix, projmatrix, campos) must be device pointers", fn, v);
    if (s[v].image_height != s[0].image_height || s[v].image_width != s[0].image_width || s[v].scale_modifier != s[0].scale_modifier ||
        s[v].sh_degree != s[0].sh_degree || s[v].flags != s[0].flags)
      return set_err(GSR_ERR_INVALID, "%s: view %d differs from view 0 in image size, scale modifier, SH degree or "
                     "flags (a batch shares them)", fn, v);
  }
  if (s[0].flags & GSR_FLAG_NEEDLE_DOUBLE) return set_err(GSR_ERR_INVALID, "%s: GSR_FLAG_NEEDLE_DOUBLE is a single-view flag", fn);
  return GSR_OK;
}

// A batch of views of ONE set of raw parameters through one launch chain (include/gsraster.h).  `f`: the views' settings
// and their count, outputs, stream; `fn` names the entry point in the messages; with_obj: gsr_forward_raw_batch_obj
// (objects_dc required, out_objects [B,16,H,W] or null).
static int forward_raw_batch_impl(const char* fn, bool with_obj, FwdCall f, const RawSeg& a) {
  if (f.ctx_out) *f.ctx_out = nullptr;
  if (const int rc = check_batch_views(fn, f.s, f.nviews)) return rc;
  if (a.n > 0 && (!a.features_dc || !a.features_rest || !a.scaling || !a.rotation))
    return set_err(GSR_ERR_INVALID, "%s: null features_dc / features_rest / log_scaling / rotation_raw", fn);
  if (with_obj && a.n > 0 && !a.objects_dc) return set_err(GSR_ERR_INVALID, "%s: objects_dc is null", fn);
  if (!f.out_color) return set_err(GSR_ERR_INVALID, "%s: out_color is null", fn);
  set_raw_inputs(f, a.n, a);
  if (a.n == 0 && f.nviews > 1) {        // an empty scene: B backgrounds; the context (of view 0) has nothing to differentiate
    const size_t px = (size_t)f.s[0].image_height * (size_t)f.s[0].image_width;
    for (int v = 0; v < f.nviews; ++v) {
      FwdCall fv = f;                    // view v alone, its outputs at their place in the batch's
      fv.s = f.s + v; fv.nviews = 1; fv.sh_objs = nullptr;
      fv.out_color = f.out_color + (size_t)v * 3 * px;
      fv.out_objects = f.out_objects ? f.out_objects + (size_t)v * NUM_OBJ * px : nullptr;
      fv.out_depth = f.out_depth ? f.out_depth + (size_t)v * px : nullptr;
      fv.out_alpha = f.out_alpha ? f.out_alpha + (size_t)v * px : nullptr;
      fv.ctx_out = v == 0 ? f.ctx_out : nullptr;
      const int rc = forward_impl(fv);
      if (rc != GSR_OK) return rc;
    }
    return GSR_OK;
  }
  return forward_impl(f);
}

// gsr_forward_raw2_batch(_obj): TWO parameter sets as one scene per view, forward only (see below)
static int forward_raw2_batch_impl(const char* fn, bool with_obj, FwdCall f, const RawSeg& a, const RawSeg& b) {
  if (f.ctx_out) *f.ctx_out = nullptr;
  if (a.n <= 0 || b.n <= 0 || (long long)a.n + b.n > 0x7FFFFFFFll)
    return set_err(GSR_ERR_INVALID, "%s: both segments must hold Gaussians (Pa=%d Pb=%d)", fn, a.n, b.n);
  if (const int rc = check_batch_views(fn, f.s, f.nviews)) return rc;
  if (!raw_seg_complete(a) || !raw_seg_complete(b)) return set_err(GSR_ERR_INVALID, "%s: null parameter tensor", fn);
  if (with_obj && ((a.objects_dc == nullptr) != (b.objects_dc == nullptr)))
    return set_err(GSR_ERR_INVALID, "%s: objects_dc_a and objects_dc_b: both or neither", fn);
  if (!f.out_color) return set_err(GSR_ERR_INVALID, "%s: out_color is null", fn);
  set_raw_inputs(f, a.n + b.n, a);
  f.segb = &b; f.fwd_only = true;
  return forward_impl(f);
}

extern "C" {

// (The entry points that are another one with some arguments null -- gsr_forward, gsr_forward_raw, gsr_forward_raw2,
// gsr_forward_raw_batch -- call that one, argument for argument in the same order.)
int gsr_forward_aux(const GsrSettings* s, int32_t P, int32_t K, const float* means3D, const float* shs,
                    const float* sh_objs, const float* colors_precomp, const float* opacities, const float* scales,
                    const float* rotations, const float* cov3D_precomp, float* out_color, float* out_objects,
                    int32_t* radii, GsrCtx** ctx_out, int64_t* num_rendered, float* out_depth, float* out_alpha,
                    void* stream) {
  FwdCall f;
  f.s = s; f.P = P; f.K = K; f.means3D = means3D; f.shs = shs; f.sh_objs = sh_objs; f.colors_precomp = colors_precomp;
  f.opacities = opacities; f.scales = scales; f.rotations = rotations; f.cov3D_precomp = cov3D_precomp;
  f.out_color = out_color; f.out_objects = out_objects; f.radii = radii; f.ctx_out = ctx_out; f.num_rendered = num_rendered;
  f.out_depth = out_depth; f.out_alpha = out_alpha; f.stream = stream;
  return forward_impl(f);
}

int gsr_forward(const GsrSettings* s, int32_t P, int32_t K, const float* means3D, const float* shs,
                const float* sh_objs, const float* colors_precomp, const float* opacities, const float* scales,
                const float* rotations, const float* cov3D_precomp, float* out_color, float* out_objects,
                int32_t* radii, GsrCtx** ctx_out, int64_t* num_rendered, void* stream) {
  return gsr_forward_aux(s, P, K, means3D, shs, sh_objs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                         out_color, out_objects, radii, ctx_out, num_rendered, nullptr, nullptr, stream);
}

int gsr_forward_raw_aux(const GsrSettings* s, int32_t P, const float* xyz, const float* features_dc,
                        const float* features_rest, const float* objects_dc, const float* opacity_logit,
                        const float* log_scaling, const float* rotation_raw, float* out_color, float* out_objects,
                        int32_t* radii, GsrCtx** ctx_out, int64_t* num_rendered, float* out_depth, float* out_alpha,
                        void* stream) {
  if (P > 0 && (!features_dc || !features_rest || !log_scaling || !rotation_raw))
    return set_err(GSR_ERR_INVALID, "gsr_forward_raw: null features_dc / features_rest / log_scaling / rotation_raw");
  RawSeg a;
  a.n = P; a.xyz = xyz; a.features_dc = features_dc; a.features_rest = features_rest; a.objects_dc = objects_dc;
  a.opacity = opacity_logit; a.scaling = log_scaling; a.rotation = rotation_raw;
  FwdCall f;
  f.s = s; f.out_color = out_color; f.out_objects = out_objects; f.radii = radii; f.ctx_out = ctx_out;
  f.num_rendered = num_rendered; f.out_depth = out_depth; f.out_alpha = out_alpha; f.stream = stream;
  set_raw_inputs(f, P, a);
  return forward_impl(f);
}

int gsr_forward_raw(const GsrSettings* s, int32_t P, const float* xyz, const float* features_dc,
                    const float* features_rest, const float* objects_dc, const float* opacity_logit,
                    const float* log_scaling, const float* rotation_raw, float* out_color, float* out_objects,
                    int32_t* radii, GsrCtx** ctx_out, int64_t* num_rendered, void* stream) {
  return gsr_forward_raw_aux(s, P, xyz, features_dc, features_rest, objects_dc, opacity_logit, log_scaling, rotation_raw,
                             out_color, out_objects, radii, ctx_out, num_rendered, nullptr, nullptr, stream);
}

int gsr_forward_raw2_keep(const GsrSettings* s, int32_t Pa, const float* xyz_a, const float* features_dc_a,
                          const float* features_rest_a, const float* objects_dc_a, const float* opacity_logit_a,
                          const float* log_scaling_a, const float* rotation_raw_a, int32_t Pb, const float* xyz_b,
                          const float* features_dc_b, const float* features_rest_b, const float* objects_dc_b,
                          const float* opacity_logit_b, const float* log_scaling_b, const float* rotation_raw_b,
                          float* out_color, float* out_objects, int32_t* radii, GsrCtx** ctx_out, int64_t* num_rendered,
                          void* stream) {
  if (Pa < 0 || Pb < 0 || (long long)Pa + Pb > 0x7FFFFFFFll) return set_err(GSR_ERR_INVALID, "gsr_forward_raw2: bad sizes Pa=%d Pb=%d", Pa, Pb);
  RawSeg a, b;
  a.n = Pa; a.xyz = xyz_a; a.features_dc = features_dc_a; a.features_rest = features_rest_a; a.objects_dc = objects_dc_a;
  a.opacity = opacity_logit_a; a.scaling = log_scaling_a; a.rotation = rotation_raw_a;
  b.n = Pb; b.xyz = xyz_b; b.features_dc = features_dc_b; b.features_rest = features_rest_b; b.objects_dc = objects_dc_b;
  b.opacity = opacity_logit_b; b.scaling = log_scaling_b; b.rotation = rotation_raw_b;
  FwdCall f;
  f.s = s; f.fwd_only = true; f.out_color = out_color; f.out_objects = out_objects; f.radii = radii; f.ctx_out = ctx_out;
  f.num_rendered = num_rendered; f.stream = stream;
  if (Pa == 0 || Pb == 0) {              // one segment holds everything: an ordinary raw forward of that one
    set_raw_inputs(f, Pa + Pb, Pb == 0 ? a : b);
    return forward_impl(f);
  }
  if (!raw_seg_complete(a) || !raw_seg_complete(b)) return set_err(GSR_ERR_INVALID, "gsr_forward_raw2: null parameter tensor");
  if (out_objects && ((objects_dc_a == nullptr) != (objects_dc_b == nullptr)))
    return set_err(GSR_ERR_INVALID, "gsr_forward_raw2: object features must be given for both segments or for neither");
  set_raw_inputs(f, Pa + Pb, a);
  f.segb = &b;
  return forward_impl(f);
}

int gsr_forward_raw2(const GsrSettings* s, int32_t Pa, const float* xyz_a, const float* features_dc_a,
                     const float* features_rest_a, const float* objects_dc_a, const float* opacity_logit_a,
                     const float* log_scaling_a, const float* rotation_raw_a, int32_t Pb, const float* xyz_b,
                     const float* features_dc_b, const float* features_rest_b, const float* objects_dc_b,
                     const float* opacity_logit_b, const float* log_scaling_b, const float* rotation_raw_b,
                     float* out_color, float* out_objects, int32_t* radii, int64_t* num_rendered, void* stream) {
  return gsr_forward_raw2_keep(s, Pa, xyz_a, features_dc_a, features_rest_a, objects_dc_a, opacity_logit_a, log_scaling_a,
                               rotation_raw_a, Pb, xyz_b, features_dc_b, features_rest_b, objects_dc_b, opacity_logit_b,
                               log_scaling_b, rotation_raw_b, out_color, out_objects, radii, nullptr, num_rendered, stream);
}

int gsr_forward_raw_batch_aux(const GsrSettings* s, int32_t B, int32_t P, const float* xyz, const float* features_dc,
                              const float* features_rest, const float* opacity_logit, const float* log_scaling,
                              const float* rotation_raw, float* out_color, int32_t* radii, GsrCtx** ctx_out,
                              int64_t* num_rendered, float* out_depth, float* out_alpha, void* stream) {
  RawSeg a;
  a.n = P; a.xyz = xyz; a.features_dc = features_dc; a.features_rest = features_rest; a.opacity = opacity_logit;
  a.scaling = log_scaling; a.rotation = rotation_raw;
  FwdCall f;
  f.s = s; f.nviews = B; f.out_color = out_color; f.radii = radii; f.ctx_out = ctx_out; f.num_rendered = num_rendered;
  f.out_depth = out_depth; f.out_alpha = out_alpha; f.stream = stream;
  return forward_raw_batch_impl("gsr_forward_raw_batch", false, f, a);   // (the messages name the plain entry point)
}

int gsr_forward_raw_batch(const GsrSettings* s, int32_t B, int32_t P, const float* xyz, const float* features_dc,
                          const float* features_rest, const float* opacity_logit, const float* log_scaling,
                          const float* rotation_raw, float* out_color, int32_t* radii, GsrCtx** ctx_out, int64_t* num_rendered,
                          void* stream) {
  return gsr_forward_raw_batch_aux(s, B, P, xyz, features_dc, features_rest, opacity_logit, log_scaling, rotation_raw, out_color,
                                   radii, ctx_out, num_rendered, nullptr, nullptr, stream);
}

int gsr_forward_raw_batch_obj(const GsrSettings* s, int32_t B, int32_t P, const float* xyz, const float* features_dc,
                              const float* features_rest, const float* objects_dc, const float* opacity_logit,
                              const float* log_scaling, const float* rotation_raw, float* out_color, float* out_objects,
                              int32_t* radii, GsrCtx** ctx_out, int64_t* num_rendered, void* stream) {
  RawSeg a;
  a.n = P; a.xyz = xyz; a.features_dc = features_dc; a.features_rest = features_rest; a.objects_dc = objects_dc;
  a.opacity = opacity_logit; a.scaling = log_scaling; a.rotation = rotation_raw;
  FwdCall f;
  f.s = s; f.nviews = B; f.out_color = out_color; f.out_objects = out_objects; f.radii = radii; f.ctx_out = ctx_out;
  f.num_rendered = num_rendered; f.stream = stream;
  return forward_raw_batch_impl("gsr_forward_raw_batch_obj", true, f, a);
}

// gsr_forward_raw_batch for TWO parameter sets as one scene per view (the success renders of a batch, reference
// attack.py:513-530 inside the loop over the batch's cameras): forward only; a kept context is re-renderable, not differentiable.
int gsr_forward_raw2_batch(const GsrSettings* s, int32_t B, int32_t Pa, const float* xyz_a, const float* features_dc_a,
                           const float* features_rest_a, const float* opacity_logit_a, const float* log_scaling_a,
                           const float* rotation_raw_a, int32_t Pb, const float* xyz_b, const float* features_dc_b,
                           const float* features_rest_b, const float* opacity_logit_b, const float* log_scaling_b,
                           const float* rotation_raw_b, float* out_color, int32_t* radii, GsrCtx** ctx_out,
                           int64_t* num_rendered, void* stream) {
  RawSeg a, b;
  a.n = Pa; a.xyz = xyz_a; a.features_dc = features_dc_a; a.features_rest = features_rest_a; a.opacity = opacity_logit_a;
  a.scaling = log_scaling_a; a.rotation = rotation_raw_a;
  b.n = Pb; b.xyz = xyz_b; b.features_dc = features_dc_b; b.features_rest = features_rest_b; b.opacity = opacity_logit_b;
  b.scaling = log_scaling_b; b.rotation = rotation_raw_b;
  FwdCall f;
  f.s = s; f.nviews = B; f.out_color = out_color; f.radii = radii; f.ctx_out = ctx_out; f.num_rendered = num_rendered;
  f.stream = stream;
  return forward_raw2_batch_impl("gsr_forward_raw2_batch", false, f, a, b);
}

int gsr_forward_raw2_batch_obj(const GsrSettings* s, int32_t B, int32_t Pa, const float* xyz_a, const float* features_dc_a,
                               const float* features_rest_a, const float* objects_dc_a, const float* opacity_logit_a,
                               const float* log_scaling_a, const float* rotation_raw_a, int32_t Pb, const float* xyz_b,
                               const float* features_dc_b, const float* features_rest_b, const float* objects_dc_b,
                               const float* opacity_logit_b, const float* log_scaling_b, const float* rotation_raw_b,
                               float* out_color, float* out_objects, int32_t* radii, GsrCtx** ctx_out, int64_t* num_rendered,
                               void* stream) {
  RawSeg a, b;
  a.n = Pa; a.xyz = xyz_a; a.features_dc = features_dc_a; a.features_rest = features_rest_a; a.objects_dc = objects_dc_a;
  a.opacity = opacity_logit_a; a.scaling = log_scaling_a; a.rotation = rotation_raw_a;
  b.n = Pb; b.xyz = xyz_b; b.features_dc = features_dc_b; b.features_rest = features_rest_b; b.objects_dc = objects_dc_b;
  b.opacity = opacity_logit_b; b.scaling = log_scaling_b; b.rotation = rotation_raw_b;
  FwdCall f;
  f.s = s; f.nviews = B; f.out_color = out_color; f.out_objects = out_objects; f.radii = radii; f.ctx_out = ctx_out;
  f.num_rendered = num_rendered; f.stream = stream;
  return forward_raw2_batch_impl("gsr_forward_raw2_batch_obj", true, f, a, b);
}

// Re-render of a kept context whose colour inputs (SH coefficients) may have changed and nothing else has: the colour
// half of K1 over the Gaussians that emit pairs, then K6 over the kept lists.  include/gsraster.h has the contract.
int gsr_ctx_rerender(GsrCtx* c, const float* features_dc, const float* features_rest, const float* features_dc_b,
                     const float* features_rest_b, const float* bg, float* out_color, float* out_objects, uint32_t flags,
                     void* stream) {
  if (!c) return set_err(GSR_ERR_STATE, "gsr_ctx_rerender: null context");
  if (!out_color) return set_err(GSR_ERR_INVALID, "gsr_ctx_rerender: out_color is null");
  if (c->aux)
    return set_err(GSR_ERR_STATE, "gsr_ctx_rerender: the context's forward produced depth / alpha maps (gsr_forward*_aux); "
                   "such a context is not re-rendered");
  // a batch context (gsr_forward_raw_batch / gsr_forward_raw2_batch and their _obj forms): out_color [B,3,H,W], bg [B,3] or
  // null; out_objects [B,16,H,W] only if the batch's forward composited object channels
  if (c->B > 1 && out_objects && !c->objects_out)
    return set_err(GSR_ERR_INVALID, "gsr_ctx_rerender: a batch context (%d views) has no object channels", c->B);
  if (c->P > 0 && (!c->lanegroup || !c->shs))
    return set_err(GSR_ERR_INVALID, "gsr_ctx_rerender: the context was not rendered from SH coefficients (raw parameters, "
                   "or shs with K = 16): there is no colour stage to run again");
  if (out_objects && !c->objects_out)
    return set_err(GSR_ERR_INVALID, "gsr_ctx_rerender: the context's forward did not composite object features");
  if (!c->raw && features_dc)
    return set_err(GSR_ERR_INVALID, "gsr_ctx_rerender: a gsr_forward context takes its [P,16,3] coefficients in `features_rest`");
  if (!c->has_b && (features_dc_b || features_rest_b))
    return set_err(GSR_ERR_INVALID, "gsr_ctx_rerender: the context has one attribute segment");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (ctx_resolve_count(c) != GSR_OK) return set_err(GSR_ERR_DEVICE, "gsr_ctx_rerender: reading the forward's pair count failed");
  if (c->overflow)
    return set_err(GSR_ERR_OVERFLOW, "gsr_ctx_rerender: the context's forward overflowed its pair capacity (%llu pairs, "
                   "capacity %u): render again with gsr_forward", c->n64, c->nbound);
  if ((flags & GSR_RERENDER_FIRST_SEGMENT_ONLY) && (features_dc_b || features_rest_b))
    return set_err(GSR_ERR_INVALID, "gsr_ctx_rerender: GSR_RERENDER_FIRST_SEGMENT_ONLY with new second-segment coefficients");
  // every argument check has passed: only now does the kept context take the call's pointers and follow its stream (a
  // rejected call leaves the context exactly as it was)
  pool_retag(c->dev, c->keep_blk, st); pool_retag(c->dev, c->rank_blk, st); pool_retag(c->dev, c->seg_blk, st);
  c->sumsq_out = nullptr;                // a request armed for a backward of the previous render does not carry over
  if (features_rest) c->shs = features_rest;
  if (features_dc) c->sh_dc = features_dc;
  if (features_rest_b) c->b.features_rest = features_rest_b;
  if (features_dc_b) c->b.features_dc = features_dc_b;
  if (bg && c->B > 1) {
    for (int v = 0; v < c->B; ++v) c->views[v].bg = bg + 3 * (size_t)v;
    c->st.bg = bg;
  } else if (bg) {
    c->st.bg = bg;
  }
  if (c->P > 0) {
    StageTimer t(GSR_STAGE_PREPROCESS, st);
    const bool skip_D = (flags & GSR_RERENDER_COLOR_GRADS_ONLY) != 0u;
    c->D_stale = c->D != nullptr && skip_D;
    // two segments, the second one's coefficients untouched since the last render: its colour words are still right
    const bool first_only = c->has_b && (flags & GSR_RERENDER_FIRST_SEGMENT_ONLY);
    const dim3 blkC(PREF_BLOCK);
    if (c->B > 1) {
      // the batch's colour kernel over the Gaussians that emit pairs in ANY view (every SH row read once), the views' constants
      // packed again first: the CONTENTS of a background tensor may have changed, and the compositors read it from there
      launch_pack_views(c, st);
      PreColorBatchArgs ca = color_batch_args(c, nullptr);
      if (first_only) ca.P = ca.Pa;
      if (skip_D) ca.D = nullptr;
      hipLaunchKernelGGL(k_pre_color_batch, dim3((unsigned)((ca.P + PREF_BLOCK - 1) / PREF_BLOCK)), blkC, 0, st, ca);
    } else {
      PreArgs pa = color_args(c, nullptr);
      if (first_only) pa.P = pa.Pa;
      if (skip_D) pa.D = nullptr;
      hipLaunchKernelGGL(c->raw ? k_pre_color<true> : k_pre_color<false>, dim3((unsigned)((pa.P + PREF_BLOCK - 1) / PREF_BLOCK)), blkC, 0, st, pa);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
      return set_err(GSR_ERR_DEVICE, "rerender colours%s: launch failed: %s", c->B > 1 ? " (batch)" : "", hipGetErrorString(e));
  }
  StageTimer t(GSR_STAGE_RENDER_FWD, st);
  return launch_render_fwd(c, out_color, out_objects, st);
}

}  // extern "C"

static bool batch_k9_fused() {
  static const int env = [] { const char* e = getenv("GSR_BATCH_K9"); return e ? atoi(e) : 1; }();
  return env != 0;
}

// where a backward leaves its gradients (null: not wanted), under forward_impl's names of the inputs
struct GradOut {
  float *means3D = nullptr, *means2D = nullptr, *shs = nullptr, *sh_dc = nullptr, *sh_objs = nullptr,
        *colors_precomp = nullptr, *opacities = nullptr, *scales = nullptr, *rotations = nullptr, *cov3D = nullptr;
};

// One backward, as every backward entry point hands it to backward_impl.
struct BwdCall {
  const float *grad_color = nullptr, *grad_objects = nullptr;
  GradOut d;
  bool accumulate = false;
  int nchunks = 1;                  // gsr_backward_raw_chunked: ranges of the per-Gaussian stage, the caller told after each
  gsr_chunk_fn chunk_done = nullptr;
  void* chunk_user = nullptr;
  // != 0 (gsr_backward_raw_batch_views): a batch context's PER-VIEW gradients -- the attribute-gradient pointers are
  // view 0's buffers, view v's lie v * view_stride floats further; every view's buffers are overwritten
  int64_t view_stride = 0;
  void* stream = nullptr;
};

// An entry point serves the contexts of gsr_forward (want_raw false) or those of the raw forwards, not both.  (A null
// context is backward_impl's to refuse.)
static int check_ctx_kind(const char* fn, const GsrCtx* c, bool want_raw) {
  if (!c || c->raw == want_raw) return GSR_OK;
  if (!want_raw) return set_err(GSR_ERR_STATE, "%s: context came from gsr_forward_raw; use gsr_backward_raw", fn);
  return set_err(GSR_ERR_STATE, "%s: context came from gsr_forward; use gsr_backward", fn);
}

// ---------------------------------------------------------------------------------------------
// The backward.  backward_impl (at the end of this section) refuses what it has to before anything is allocated or
// launched, then runs K7 (render_bwd) and the per-Gaussian stage K8+K9 (pre_bwd).
// ---------------------------------------------------------------------------------------------
// What one backward holds while it runs.
struct BwdRun {
  GsrCtx* c;
  const BwdCall& b;
  hipStream_t st;
  // the context's one-shot requests, taken (and the context disarmed) when the call starts
  double* ss_out = nullptr;                           // gsr_ctx_request_sumsq
  const float *aux_gd = nullptr, *aux_ga = nullptr;   // gsr_ctx_set_aux_grads
  bool aux = false;                                   // ... either of them
  bool obj = false;                 // dL/d object channels comes in and the context has object features
  bool geom = false;                // a geometry-side gradient is wanted
  int nchunks = 1;                  // ranges of the per-Gaussian stage
  bool batch_fused = false;         // a batch's per-Gaussian stage is ONE k_pre_bwd_batch launch per range
  bool segs_on = false;             // K7 walks the long lists as segments
  int bwd_npx = 4;                  // pixels per lane of K7
  uint32_t nsub = 1;                // K7's partial rows per pair: PXL / bwd_npx
  uint32_t tag_lo = 0, tag_hi = 0;  // 64-bit tag of this call: K7 stamps it into every partial row it writes, K8/K9 ignores rows without it
  float4 *part = nullptr, *part_obj = nullptr;   // K7's partial rows (pool blocks)
  int finish(int code) { pool_free(c->dev, part); pool_free(c->dev, part_obj); return code; }

  int check_aux_grads() const;
  int check_pre_bwd();
  int take_partial_rows();
  int render_bwd();                                   // K7
  int pre_bwd();                                      // K8+K9, through one of the three launch forms per range:
  PreBwdArgs shared_args() const;
  void launch_batch(const PreBwdArgs& sh, int gb, int ge) const;
  void launch_views(PreBwdArgs pa, int gb, int ge) const;
  void launch_view(PreBwdArgs pa, int v, int gb, int ge) const;
};

// what a backward with depth / alpha gradients armed (gsr_ctx_set_aux_grads) cannot be
int BwdRun::check_aux_grads() const {
  if (b.view_stride != 0)
    return set_err(GSR_ERR_INVALID, "gsr_ctx_set_aux_grads: the per-view batch backward (gsr_backward_raw_batch_views / _obj_views) "
                   "does not take depth / alpha gradients");
  if (b.nchunks > 1)
    return set_err(GSR_ERR_INVALID, "gsr_ctx_set_aux_grads: gsr_backward_raw_chunked with more than one range does not take "
                   "depth / alpha gradients");
  if (b.grad_objects != nullptr)
    return set_err(GSR_ERR_INVALID, "gsr_ctx_set_aux_grads: depth / alpha gradients and grad_objects in one backward are not supported");
  if (!geom)
    return set_err(GSR_ERR_INVALID, "gsr_ctx_set_aux_grads: depth / alpha gradients reach geometry and opacity only, and this "
                   "backward asks for no such gradient");
  if (!c->lanegroup)
    return set_err(GSR_ERR_INVALID, "gsr_ctx_set_aux_grads: a gsr_forward context with K != 16 SH coefficients does not take "
                   "depth / alpha gradients");
  if (c->st.flags & GSR_FLAG_NEEDLE_DOUBLE)
    return set_err(GSR_ERR_INVALID, "gsr_ctx_set_aux_grads: not available under GSR_FLAG_NEEDLE_DOUBLE");
  return GSR_OK;
}

// What the per-Gaussian stage cannot serve: asked before K7 is launched, so that a refused backward launches nothing.
// Also settles how that stage will run (nchunks, batch_fused).
int BwdRun::check_pre_bwd() {
  const float* const dsh = c->shs ? b.d.shs : nullptr;
  if (c->raw && ((dsh == nullptr) != (b.d.sh_dc == nullptr)))
    return set_err(GSR_ERR_INVALID, "gsr_backward_raw: dfeatures_dc and dfeatures_rest must both be given");
  if (c->lanegroup && c->shs && geom && !c->D)
    return set_err(GSR_ERR_STATE, "gsr_backward: the forward of this context was run without its backward state");
  if (c->lanegroup && c->shs && geom && c->D_stale)
    return set_err(GSR_ERR_STATE, "gsr_backward: geometry gradients asked of a context whose last gsr_ctx_rerender was "
                   "told GSR_RERENDER_COLOR_GRADS_ONLY");
  // The per-Gaussian stage covers the Gaussians in `nchunks` ranges (multiples of 64), one launch each; after a
  // range's launch is enqueued the caller is told (chunk_done): its gradients are complete in stream order, so a
  // collective over that range can be issued while the next range is still being computed.
  nchunks = std::max(1, std::min(b.nchunks, (c->P + 63) / 64));
  // a batch of views: ONE launch of k_pre_bwd_batch per range walks the B views and writes the gradients once
  // (GSR_BATCH_K9=0: one k_pre_bwd launch per view instead, the others in accumulate mode -- the A/B and the bit-exact form)
  batch_fused = c->B > 1 && c->raw && c->lanegroup && batch_k9_fused() && b.view_stride == 0;
  if (ss_out && (!(c->lanegroup && c->raw) || b.accumulate || nchunks != 1 || (c->B > 1 && !batch_fused)))
    return set_err(GSR_ERR_INVALID, "gsr_ctx_request_sumsq: served by an overwriting gsr_backward_raw* over one range only");
  return GSR_OK;
}

// K7's partial rows (one per list entry and tile part), and the tag that tells this call's rows from stale ones
int BwdRun::take_partial_rows() {
  const uint32_t N = c->nbound;
  // K7 runs one wave per 16x(4*npx) part of a tile; each writes its own partial row per list entry (4 pixels per lane:
  // one wave per tile; 2: two, and K8/K9 then sums twice the rows).  With long lists walked as segments every work item
  // is short whatever the tile count, so one wave per tile it is (S-hydrant-full, 2500 tiles: K7 0.169 -> 0.194 ms but
  // K8+K9 0.141 -> 0.084 ms, 2563 -> 2811 views/s); only without segments (object channels, GSR_FLAG_NO_SEGMENTS) an
  // image with fewer tiles than the chip has wave slots is split in two.  GSR_FLAG_BWD_SPLIT(n) overrides.
  // (The rule looks at the tiles of ONE view, also for a batch: the split decides how many partial rows K9 adds up per
  // pair -- the float32 association of the sums -- and a batch's per-view gradients are the single-view call's bit for bit.
  // Found by tests/diag_fuzz_batch.py with GSR_FLAG_NO_SEGMENTS on batches of >= 4096 tiles of views with fewer.)
  segs_on = c->bnd != nullptr && !obj && aux_gd == nullptr;   // (dL/ddepth walks whole lists: no running depth in the records)
  bwd_npx = flag_bwd_npx(c->st.flags) ? flag_bwd_npx(c->st.flags) : ((c->tpv < 4096 && !segs_on) ? 2 : 4);
  nsub = (uint32_t)(PXL / bwd_npx);
  if (N > 0) {
    part = static_cast<float4*>(pool_alloc(c->dev, sizeof(float4) * PART_F4 * (size_t)N * nsub, st));
    if (obj) part_obj = static_cast<float4*>(pool_alloc(c->dev, sizeof(float4) * 4 * (size_t)N * nsub, st));
    if (!part || (obj && !part_obj))
      return set_err(GSR_ERR_NOMEM, "gsr_backward: partial-gradient buffer (N=%u) allocation failed", N);
  }
  static std::atomic<uint64_t> tag_counter{0x243F6A8885A308D3ull};
  uint64_t z = tag_counter.fetch_add(0x9E3779B97F4A7C15ull) + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
  tag_lo = (uint32_t)z; tag_hi = (uint32_t)(z >> 32);
  return GSR_OK;
}

// K7: the backward compositor (a context with pairs only)
int BwdRun::render_bwd() {
  StageTimer t(GSR_STAGE_RENDER_BWD, st, true);
  RenderBwdArgs ra;
  ra.tag_lo = tag_lo; ra.tag_hi = tag_hi;
  ra.ranges = c->ranges; ra.pair_rank = c->pair_rank; ra.offg = c->offg; ra.R0 = c->G0; ra.R1 = c->G1; ra.R2 = c->G2;
  ra.sh_objs = c->sh_objs; ra.bg = c->st.bg; ra.W = c->st.image_width; ra.H = c->st.image_height;
  ra.map_mode = flag_tile_map(c->st.flags);
  ra.sched = c->sched;
  ra.wave_clock = g_wave_clock.load();
  ra.gridx = c->gridx; ra.ntiles = c->ntiles; ra.final_T = c->final_T; ra.n_contrib = c->n_contrib;
  ra.grad_color = b.grad_color; ra.grad_objects = obj ? b.grad_objects : nullptr; ra.part = part; ra.part_obj = part_obj;
  // split tiles: one extra work item per boundary record, in front of the per-tile items
  ra.grad_depth = aux_gd; ra.grad_alpha = aux_ga;
  ra.bnd = segs_on ? c->bnd : nullptr; ra.segoff = c->segoff; ra.rec_item = c->rec_item; ra.nrec = c->dv + DV_NREC;
  ra.seg_shift = c->seg_shift; ra.extra_blocks = segs_on ? c->rec_cap * nsub : 0u;
  ra.tpv = c->tpv; ra.vpack = c->vpack; ra.Ppad = c->Ppad;
  const dim3 gridT(ra.extra_blocks + (unsigned)render_grid(c->ntiles * (int)nsub)), blk(64);
  const Kern<RenderBwdArgs> k7 = pick_render_bwd(obj, bwd_npx, geom, aux);
  if (t.on) hipExtLaunchKernelGGL(k7, gridT, blk, 0, st, t.a, t.b, 0, ra);
  else hipLaunchKernelGGL(k7, gridT, blk, 0, st, ra);
  LAUNCH_CHECK("render backward");
  return GSR_OK;
}

// what every launch form of the per-Gaussian stage shares: one view (view 0 of a batch) over all its Gaussians
PreBwdArgs BwdRun::shared_args() const {
  const GradOut& g = b.d;
  PreBwdArgs pa;
  pa.P = c->P; pa.g0 = 0; pa.K = c->K; pa.va = view_args(c->st);
  pa.offg = c->offg; pa.G0 = c->G0; pa.G1 = c->G1; pa.G2 = c->G2;
  pa.part = part; pa.part_obj = obj ? part_obj : nullptr;
  pa.tag_lo = tag_lo; pa.tag_hi = tag_hi; pa.nsub = nsub;
  pa.means = c->means3D; pa.scales = c->scales; pa.rots = c->rots; pa.cov3d = c->cov3d; pa.sh = c->shs;
  pa.sh_dc = c->sh_dc; pa.D = c->D; pa.abc = c->abc;
  pa.needle_double = (c->st.flags & GSR_FLAG_NEEDLE_DOUBLE) != 0u ? 1 : 0;
  // (a batch: the object-feature gradient is k_obj_grad_batch's, the per-Gaussian kernels leave it alone)
  pa.dmeans3D = g.means3D; pa.dmeans2D = g.means2D; pa.dsh = c->shs ? g.shs : nullptr; pa.dsh_dc = g.sh_dc;
  pa.dsh_objs = c->B > 1 ? nullptr : g.sh_objs; pa.dcolors = c->colors ? g.colors_precomp : nullptr; pa.dopac = g.opacities;
  pa.dscales = c->cov3d ? nullptr : g.scales; pa.drots = c->cov3d ? nullptr : g.rotations;
  pa.dcov3d = c->cov3d ? g.cov3D : nullptr;
  pa.accumulate = b.accumulate ? 1 : 0;
  pa.vpack = nullptr; pa.Ppad = 0; pa.Pscene = c->P; pa.vstride = 0;
  pa.sumsq = nullptr;
  return pa;
}

// Gaussians [gb, ge) of a batch, its views summed: ONE launch of k_pre_bwd_batch walks the B views and writes the gradients once
void BwdRun::launch_batch(const PreBwdArgs& sh, int gb, int ge) const {
  const GradOut& d = b.d;
  PreBwdBatchArgs ba;
  ba.P = ge; ba.g0 = gb; ba.B = c->B; ba.Ppad = c->Ppad; ba.Pscene = c->P; ba.vpack = c->vpack;
  ba.H = c->st.image_height; ba.W = c->st.image_width; ba.deg = c->st.sh_degree; ba.mod = c->st.scale_modifier;
  ba.offg = c->offg; ba.G0 = c->G0; ba.G1 = c->G1; ba.G2 = c->G2; ba.part = part;
  ba.tag_lo = tag_lo; ba.tag_hi = tag_hi; ba.nsub = nsub;
  ba.means = c->means3D; ba.scales = c->scales; ba.rots = c->rots; ba.D = c->D;
  ba.dmeans3D = d.means3D; ba.dmeans2D = d.means2D; ba.dsh = d.shs; ba.dsh_dc = d.sh_dc; ba.dopac = d.opacities;
  ba.dscales = d.scales; ba.drots = d.rotations; ba.sumsq = sh.sumsq;
  const dim3 gridB((unsigned)((ge - gb + 63) / 64)), blkB(64 * BATCH_K9_WAVES);
  const size_t lds = sizeof(float) * 3 * 64 * (size_t)c->B;
  hipLaunchKernelGGL(pick_pre_bwd_batch(geom, b.accumulate, aux), gridB, blkB, lds, st, ba);
}

// Gaussians [gb, ge) of a batch, per-view gradients (gsr_backward_raw_batch_views): ONE launch whose grid.y is the view --
// the B per-view launches' ramp-ups and tails happen once.  View v's buffers lie v * view_stride floats behind view 0's.
void BwdRun::launch_views(PreBwdArgs pa, int gb, int ge) const {
  pa.vpack = c->vpack; pa.Ppad = c->Ppad; pa.Pscene = c->P; pa.vstride = (long long)b.view_stride;
  pa.accumulate = 0; pa.abc = nullptr;
  pa.g0 = gb; pa.P = ge;
  const dim3 gridV((unsigned)((ge - gb + PRE_BLOCK - 1) / PRE_BLOCK), (unsigned)c->B);
  hipLaunchKernelGGL(pick_pre_bwd(true, geom, false, false, false), gridV, dim3(PRE_BLOCK), 0, st, pa);
}

// Gaussians [gb, ge) of one view: the only view, or view v of a batch under GSR_BATCH_K9=0 -- one launch per view over
// the same range, the first overwriting (unless the caller asked for accumulation) and the others adding; the per-view
// arrays of the virtual scene are offset by v * Ppad
void BwdRun::launch_view(PreBwdArgs pa, int v, int gb, int ge) const {
  const GradOut& d = b.d;
  const bool acc_v = b.view_stride == 0 && (b.accumulate || v > 0);
  if (c->B > 1) {
    const size_t o = (size_t)v * (size_t)c->Ppad;
    pa.va = view_args(c->views[v]);
    pa.offg = c->offg + o; pa.G0 = c->G0 + REC * o; pa.G1 = c->G1 + REC * o; pa.G2 = c->G2 + REC * o;
    pa.D = c->D ? c->D + 9 * o : nullptr; pa.abc = c->abc ? c->abc + o : nullptr;
    pa.dmeans2D = d.means2D ? d.means2D + 3 * (size_t)v * (size_t)c->P : nullptr;
    pa.accumulate = acc_v ? 1 : 0;
  }
  pa.g0 = gb; pa.P = ge;
  const dim3 gridK9((unsigned)((ge - gb + PRE_BLOCK - 1) / PRE_BLOCK));
  if (c->lanegroup) {
    const bool ndl = pa.needle_double != 0 && pa.abc != nullptr;
    hipLaunchKernelGGL(pick_pre_bwd(c->raw, geom, acc_v, ndl, aux), gridK9, dim3(PRE_BLOCK), 0, st, pa);
  } else {
    if (geom && pa.needle_double) hipLaunchKernelGGL((k_preprocess_bwd<true, true>), gridK9, dim3(PRE_BLOCK), 0, st, pa);
    else if (geom) hipLaunchKernelGGL((k_preprocess_bwd<true>), gridK9, dim3(PRE_BLOCK), 0, st, pa);
    else hipLaunchKernelGGL((k_preprocess_bwd<false>), gridK9, dim3(PRE_BLOCK), 0, st, pa);
  }
}

// K8+K9: the partial rows summed per Gaussian, and the chain rule down to the caller's parameters
int BwdRun::pre_bwd() {
  const int P = c->P, dev = c->dev;
  StageTimer t(GSR_STAGE_PREPROCESS_BWD, st);
  PreBwdArgs pa = shared_args();
  if (c->B > 1 && b.d.sh_objs) {
    // dL/d object features of a batch: view by view as k_pre_bwd forms them, summed in view order (or per view)
    ObjGradBatchArgs oa;
    oa.P = P; oa.B = c->B; oa.Ppad = c->Ppad; oa.nsub = nsub; oa.tag_lo = tag_lo; oa.tag_hi = tag_hi;
    oa.offg = c->offg; oa.part = part; oa.part_obj = (obj && c->nbound > 0) ? part_obj : nullptr; oa.dobj = b.d.sh_objs;
    oa.vstride = b.view_stride != 0 ? (long long)P * NUM_OBJ : 0;
    hipLaunchKernelGGL(k_obj_grad_batch, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, oa);
  }
  // gsr_ctx_request_sumsq (one-shot): the overwriting raw-parameter kernel also leaves per-workgroup sums of squares of
  // what it writes; one small launch behind it adds them up per tensor (fixed order) into the caller's six doubles
  void* ss_blk = nullptr;
  const int ss_blocks = batch_fused ? ((P + 63) / 64) * BATCH_K9_WAVES : (P + PRE_BLOCK - 1) / PRE_BLOCK;
  if (ss_out) {
    ss_blk = pool_alloc(dev, sizeof(float) * SUMSQ_W * (size_t)ss_blocks * PRE_WAVES, st);
    if (!ss_blk) return set_err(GSR_ERR_NOMEM, "gsr_backward_raw: sum-of-squares partials allocation failed");
    pa.sumsq = static_cast<float*>(ss_blk);
  }
  const bool views_fused = !batch_fused && b.view_stride != 0 && c->B > 1;
  const int per = (((P + nchunks - 1) / nchunks) + 63) / 64 * 64;
  for (int ck = 0; ck < nchunks; ++ck) {
    const int gb = std::min(ck * per, P), ge = (ck == nchunks - 1) ? P : std::min((ck + 1) * per, P);
    if (ge > gb) {
      if (batch_fused) launch_batch(pa, gb, ge);
      else if (views_fused) launch_views(pa, gb, ge);
      else for (int v = 0; v < c->B; ++v) launch_view(pa, v, gb, ge);
    }
    if (b.chunk_done) b.chunk_done(b.chunk_user, ck, (int64_t)gb, (int64_t)ge);
  }
  if (ss_out) {
    hipLaunchKernelGGL(k_sumsq_reduce, dim3(6), dim3(256), 0, st, pa.sumsq, ss_blocks * PRE_WAVES, ss_out);
    pool_free(dev, ss_blk);
  }
  LAUNCH_CHECK("preprocess backward");
  return GSR_OK;
}

static int backward_impl(GsrCtx* c, const BwdCall& b) {
  if (!c) return set_err(GSR_ERR_STATE, "gsr_backward: null context");
  BwdRun r{c, b, static_cast<hipStream_t>(b.stream)};
  // gsr_ctx_request_sumsq is one-shot: the request is taken (and the context disarmed) here, whatever this call's fate --
  // a backward that fails early must not leave the next one writing six doubles to a buffer that may be gone by then
  r.ss_out = c->sumsq_out;
  c->sumsq_out = nullptr;
  // gsr_ctx_set_aux_grads is one-shot in the same way
  r.aux_gd = c->aux_gd; r.aux_ga = c->aux_ga;
  c->aux_gd = nullptr; c->aux_ga = nullptr;
  r.aux = r.aux_gd != nullptr || r.aux_ga != nullptr;
  if (!b.grad_color) return set_err(GSR_ERR_INVALID, "gsr_backward: grad_color is null");
  if (c->fwd_only)
    return set_err(GSR_ERR_STATE, "gsr_backward: the context was kept by gsr_forward_raw2_keep (re-render only, no backward state)");
  if (c->P == 0) return GSR_OK;
  const GradOut& d = b.d;
  r.obj = b.grad_objects != nullptr && c->sh_objs != nullptr;
  // Only colour-side gradients wanted (SH / precomputed colours / object features): K7 and K8+K9 drop the geometry
  // sums and the projection chain rule (the colour attack; BASELINE configs 2 and 3).
  r.geom = d.means3D || d.means2D || d.opacities || d.scales || d.rotations || d.cov3D;
  if (r.aux) { if (const int rc = r.check_aux_grads()) return rc; }
  // an asynchronous-count forward: its pair count must have fitted the capacity guess (else the image it produced was
  // poisoned with NaN and nothing downstream of it is meaningful).  (A forward recorded into a hipGraph publishes
  // nothing to the host: c->slot is empty and this is a no-op.)
  if (ctx_resolve_count(c) != GSR_OK) return set_err(GSR_ERR_DEVICE, "gsr_backward: reading the forward's pair count failed");
  if (c->overflow)
    return set_err(GSR_ERR_OVERFLOW, "gsr_backward: the forward emitted %llu (tile, Gaussian) pairs, more than the capacity "
                   "%u guessed from earlier views (GSR_FLAG_ASYNC_COUNT); its image was filled with NaN -- render again",
                   c->n64, c->nbound);
  if (const int rc = r.check_pre_bwd()) return rc;
  // every refusal has passed.  The context's blocks are read here, on this stream: whoever takes them over after
  // gsr_ctx_free orders behind it
  pool_retag(c->dev, c->keep_blk, r.st); pool_retag(c->dev, c->rank_blk, r.st); pool_retag(c->dev, c->seg_blk, r.st);
  int rc;
  if ((rc = r.take_partial_rows()) != GSR_OK) return r.finish(rc);
  if (c->nbound > 0 && (rc = r.render_bwd()) != GSR_OK) return r.finish(rc);
  if ((rc = r.pre_bwd()) != GSR_OK) return r.finish(rc);
  return r.finish(GSR_OK);
}

// ---- what the five detector stages' entries (further down) share.  A stage states the regions of its workspace once, as a run of take()
// calls on a Carve: with no base that run is the sizing pass (off ends as the bytes needed), with the caller's workspace
// it hands out the pointers -- so *_workspace_bytes and the entry point cannot drift apart.
static inline size_t det_round(size_t v) { return (v + 255) & ~(size_t)255; }

struct Carve {
  char* base;
  size_t off = 0;
  explicit Carve(void* ws = nullptr) : base(static_cast<char*>(ws)) {}
  template <class T>
  T* take(size_t count) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off += det_round(count * sizeof(T));
    return p;
  }
};

// the caller's workspace holds `need` bytes and starts on an `align`-byte boundary; sizer: the call that gives `need`
static int check_workspace(const char* fn, const void* ws, int64_t ws_bytes, size_t need, unsigned align, const char* sizer) {
  if (ws_bytes < (int64_t)need)
    return set_err(GSR_ERR_INVALID, "%s: workspace of %lld bytes, %zu needed (%s)", fn, (long long)ws_bytes, need, sizer);
  if (((uintptr_t)ws & (uintptr_t)(align - 1)) != 0)
    return set_err(GSR_ERR_INVALID, "%s: the workspace must be %u-byte aligned", fn, align);
  return GSR_OK;
}

// null pointers (optional tensors) pass
template <class... P>
static int check_aligned4(const char* fn, const P*... p) {
  if (((... | (uintptr_t)p) & 3) != 0) return set_err(GSR_ERR_INVALID, "%s: every tensor must be 4-byte aligned", fn);
  return GSR_OK;
}

static bool finite_pos(float v) { return v > 0.0f && v <= 3.0e38f; }       // false for a NaN
static bool finite_nonneg(float v) { return v >= 0.0f && v <= 3.0e38f; }
static bool all_finite_nonneg(std::initializer_list<float> v) { return std::all_of(v.begin(), v.end(), finite_nonneg); }

struct DetWs {
  float* score;
  int32_t *cls, *order, *ncand;
};

static DetWs det_regions(Carve& c, long long B, long long A, long long maxc) {
  DetWs w;
  w.score = c.take<float>((size_t)(B * A));
  w.cls = c.take<int32_t>((size_t)(B * A));
  w.order = c.take<int32_t>((size_t)(B * maxc));
  w.ncand = c.take<int32_t>((size_t)B);
  return w;
}

// The NMS walk over B rows of n boxes (x1 y1 x2 y2): the select-sort by score of the rows below n_valid[b] (NULL: all n),
// then the greedy walk writes keep [B, max_det] and counts.  w: det_regions(B, n, n); fn: the entry, for the error text.
static int launch_nms_walk(const char* fn, int32_t B, int32_t n, const float* boxes, const float* scores, const int32_t* classes,
                           const int32_t* n_valid, float iou_thr, int32_t max_det, const DetWs& w, int32_t* keep, int32_t* counts,
                           hipStream_t st) {
  char stage[64];
  hipLaunchKernelGGL(gsr_detect::k_det_select_sort, dim3((unsigned)B), dim3(gsr_detect::SEL_THREADS), 0, st, n, n, scores, 0, 0.0f,
                     n_valid, w.order, w.ncand, (int32_t*)nullptr, 0);
  snprintf(stage, sizeof(stage), "%s (select)", fn);
  LAUNCH_CHECK(stage);
  gsr_detect::NmsArgs na;
  na.sp = gsr_detect::Spec{};
  na.sp.B = B; na.sp.A = n; na.sp.C = 1; na.sp.box_format = 1; na.sp.iou_thr = iou_thr; na.sp.max_candidates = n; na.sp.max_det = max_det;
  na.sp.flags = classes ? 0u : gsr_detect::CLASS_AGNOSTIC;
  na.pred = nullptr; na.score = scores; na.cls = classes; na.boxes = boxes; na.order = w.order; na.ncand = w.ncand;
  na.dets = nullptr; na.keep = keep; na.counts = counts;
  hipLaunchKernelGGL((gsr_detect::k_det_nms<false>), dim3((unsigned)B), dim3(gsr_detect::NMS_THREADS), 0, st, na);
  snprintf(stage, sizeof(stage), "%s (nms)", fn);
  LAUNCH_CHECK(stage);
  return GSR_OK;
}

extern "C" {

int gsr_backward(GsrCtx* c, const float* grad_color, const float* grad_objects, float* dmeans3D, float* dmeans2D,
                 float* dshs, float* dsh_objs, float* dcolors_precomp, float* dopacities, float* dscales,
                 float* drotations, float* dcov3D, void* stream) {
  if (const int rc = check_ctx_kind("gsr_backward", c, false)) return rc;
  BwdCall b;
  b.grad_color = grad_color; b.grad_objects = grad_objects; b.stream = stream;
  b.d.means3D = dmeans3D; b.d.means2D = dmeans2D; b.d.shs = dshs; b.d.sh_objs = dsh_objs; b.d.colors_precomp = dcolors_precomp;
  b.d.opacities = dopacities; b.d.scales = dscales; b.d.rotations = drotations; b.d.cov3D = dcov3D;
  return backward_impl(c, b);
}

// (The raw backwards that are gsr_backward_raw_chunked with one range, or gsr_backward_raw_batch_obj_views without object
// channels, call that one -- behind their own refusal, which names them -- argument for argument in the same order.)
int gsr_backward_raw_chunked(GsrCtx* c, const float* grad_color, const float* grad_objects, float* dxyz, float* dmeans2D,
                             float* dfeatures_dc, float* dfeatures_rest, float* dobjects_dc, float* dopacity_logit,
                             float* dlog_scaling, float* drotation_raw, int32_t accumulate, int32_t nchunks,
                             gsr_chunk_fn chunk_done, void* user, void* stream) {
  if (const int rc = check_ctx_kind("gsr_backward_raw_chunked", c, true)) return rc;
  BwdCall b;
  b.grad_color = grad_color; b.grad_objects = grad_objects; b.stream = stream;
  b.d.means3D = dxyz; b.d.means2D = dmeans2D; b.d.sh_dc = dfeatures_dc; b.d.shs = dfeatures_rest; b.d.sh_objs = dobjects_dc;
  b.d.opacities = dopacity_logit; b.d.scales = dlog_scaling; b.d.rotations = drotation_raw;
  b.accumulate = accumulate != 0; b.nchunks = nchunks; b.chunk_done = chunk_done; b.chunk_user = user;
  return backward_impl(c, b);
}

int gsr_backward_raw(GsrCtx* c, const float* grad_color, const float* grad_objects, float* dxyz, float* dmeans2D,
                     float* dfeatures_dc, float* dfeatures_rest, float* dobjects_dc, float* dopacity_logit,
                     float* dlog_scaling, float* drotation_raw, void* stream) {
  if (const int rc = check_ctx_kind("gsr_backward_raw", c, true)) return rc;
  return gsr_backward_raw_chunked(c, grad_color, grad_objects, dxyz, dmeans2D, dfeatures_dc, dfeatures_rest, dobjects_dc,
                                  dopacity_logit, dlog_scaling, drotation_raw, 0, 1, nullptr, nullptr, stream);
}

int gsr_backward_raw_into(GsrCtx* c, const float* grad_color, const float* grad_objects, float* dxyz, float* dmeans2D,
                          float* dfeatures_dc, float* dfeatures_rest, float* dobjects_dc, float* dopacity_logit,
                          float* dlog_scaling, float* drotation_raw, int32_t accumulate, void* stream) {
  if (const int rc = check_ctx_kind("gsr_backward_raw_into", c, true)) return rc;
  return gsr_backward_raw_chunked(c, grad_color, grad_objects, dxyz, dmeans2D, dfeatures_dc, dfeatures_rest, dobjects_dc,
                                  dopacity_logit, dlog_scaling, drotation_raw, accumulate, 1, nullptr, nullptr, stream);
}

int gsr_backward_raw_batch_obj_into(GsrCtx* c, const float* grad_color, const float* grad_objects, float* dxyz, float* dmeans2D,
                                    float* dfeatures_dc, float* dfeatures_rest, float* dobjects_dc, float* dopacity_logit,
                                    float* dlog_scaling, float* drotation_raw, int32_t accumulate, void* stream) {
  if (const int rc = check_ctx_kind("gsr_backward_raw_batch_obj_into", c, true)) return rc;
  return gsr_backward_raw_chunked(c, grad_color, grad_objects, dxyz, dmeans2D, dfeatures_dc, dfeatures_rest, dobjects_dc,
                                  dopacity_logit, dlog_scaling, drotation_raw, accumulate, 1, nullptr, nullptr, stream);
}

int gsr_backward_raw_batch_into(GsrCtx* c, const float* grad_color, float* dxyz, float* dmeans2D, float* dfeatures_dc,
                                float* dfeatures_rest, float* dopacity_logit, float* dlog_scaling, float* drotation_raw,
                                int32_t accumulate, void* stream) {
  if (const int rc = check_ctx_kind("gsr_backward_raw_batch_into", c, true)) return rc;
  return gsr_backward_raw_chunked(c, grad_color, nullptr, dxyz, dmeans2D, dfeatures_dc, dfeatures_rest, nullptr, dopacity_logit,
                                  dlog_scaling, drotation_raw, accumulate, 1, nullptr, nullptr, stream);
}

int gsr_backward_raw_batch_obj_views(GsrCtx* c, const float* grad_color, const float* grad_objects, float* dxyz, float* dmeans2D,
                                     float* dfeatures_dc, float* dfeatures_rest, float* dobjects_dc, float* dopacity_logit,
                                     float* dlog_scaling, float* drotation_raw, int64_t view_stride, void* stream) {
  if (const int rc = check_ctx_kind("gsr_backward_raw_batch_obj_views", c, true)) return rc;
  if (view_stride <= 0) return set_err(GSR_ERR_INVALID, "gsr_backward_raw_batch_obj_views: view_stride must be positive (floats between two views' buffers)");
  BwdCall b;
  b.grad_color = grad_color; b.grad_objects = grad_objects; b.stream = stream;
  b.d.means3D = dxyz; b.d.means2D = dmeans2D; b.d.sh_dc = dfeatures_dc; b.d.shs = dfeatures_rest; b.d.sh_objs = dobjects_dc;
  b.d.opacities = dopacity_logit; b.d.scales = dlog_scaling; b.d.rotations = drotation_raw;
  b.view_stride = view_stride;
  return backward_impl(c, b);
}

int gsr_backward_raw_batch_views(GsrCtx* c, const float* grad_color, float* dxyz, float* dmeans2D, float* dfeatures_dc,
                                 float* dfeatures_rest, float* dopacity_logit, float* dlog_scaling, float* drotation_raw,
                                 int64_t view_stride, void* stream) {
  if (const int rc = check_ctx_kind("gsr_backward_raw_batch_views", c, true)) return rc;
  if (view_stride <= 0) return set_err(GSR_ERR_INVALID, "gsr_backward_raw_batch_views: view_stride must be positive (floats between two views' buffers)");
  return gsr_backward_raw_batch_obj_views(c, grad_color, nullptr, dxyz, dmeans2D, dfeatures_dc, dfeatures_rest, nullptr,
                                          dopacity_logit, dlog_scaling, drotation_raw, view_stride, stream);
}

int gsr_mark_visible(const GsrSettings* s, int32_t P, const float* means3D, uint8_t* present, void* stream) {
  if (!s || !s->viewmatrix || !means3D || !present) return set_err(GSR_ERR_INVALID, "gsr_mark_visible: null argument");
  if (P <= 0) return GSR_OK;
  hipLaunchKernelGGL(k_mark_visible, dim3((P + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), P,
                     s->viewmatrix, means3D, present);
  LAUNCH_CHECK("mark_visible");
  return GSR_OK;
}

int gsr_query(int32_t what, int64_t* out) {
  if (!out) return set_err(GSR_ERR_INVALID, "gsr_query: null out");
  switch (what) {
    case 0: *out = GSR_VERSION; return GSR_OK;
    case 1: {
      Pool& pl = g_pool[cur_dev()];
      std::lock_guard<std::mutex> lk(pl.mu);
      *out = (int64_t)pl.total;
      return GSR_OK;
    }
    case 3: *out = GSR_CAP_IMAGE | GSR_CAP_DETECT | GSR_CAP_DETLOSS | GSR_CAP_SETDET; return GSR_OK;     // capability bits 0..3: closed
    case 4: *out = GSR_CAP_IMAGE | GSR_CAP_DETECT | GSR_CAP_DETLOSS | GSR_CAP_SETDET | GSR_CAP_RCNN; return GSR_OK;     // bits 0..4: closed
    case 5: *out = GSR_CAP_IMAGE | GSR_CAP_DETECT | GSR_CAP_DETLOSS | GSR_CAP_SETDET | GSR_CAP_RCNN | GSR_CAP_RPN; return GSR_OK;     // every capability bit
    default: return set_err(GSR_ERR_INVALID, "gsr_query: unknown item %d", what);
  }
}

int gsr_ctx_info(const GsrCtx* c, int32_t what, int64_t* out) {
  if (!c || !out) return set_err(GSR_ERR_INVALID, "gsr_ctx_info: null argument");
  switch (what) {
    case 0:
      if (ctx_resolve_count(const_cast<GsrCtx*>(c)) != GSR_OK) return set_err(GSR_ERR_DEVICE, "gsr_ctx_info: reading the pair count failed");
      *out = (int64_t)c->n64;
      return GSR_OK;
    case 1: *out = -1; return GSR_OK;
    case 2: *out = (int64_t)(c->keep_bytes + sizeof(uint32_t) * (size_t)c->nbound); return GSR_OK;
    case 3: *out = (int64_t)c->nbound; return GSR_OK;
    case 4: *out = (int64_t)c->B; return GSR_OK;
    case 5: *out = (int64_t)c->Ppad; return GSR_OK;
    case 6: *out = (int64_t)c->depth_passes; return GSR_OK;
    case 7: *out = (int64_t)c->tile_rounds; return GSR_OK;
    case 8: *out = (int64_t)c->scan_items; return GSR_OK;
    case 9: *out = c->group_sums ? 1 : 0; return GSR_OK;
    default: return set_err(GSR_ERR_INVALID, "gsr_ctx_info: unknown item %d", what);
  }
}

int gsr_ctx_export(const GsrCtx* c, int32_t what, void* dst, int64_t dst_bytes, void* stream) {
  if (!c || !dst) return set_err(GSR_ERR_INVALID, "gsr_ctx_export: null argument");
  const size_t HW = (size_t)c->st.image_height * c->st.image_width * (size_t)c->B;   // (a batch: the B views one after another)
  const size_t PV = (size_t)c->Pv;                                                    // (... B * Ppad virtual Gaussians)
  const void* src = nullptr;
  size_t bytes = 0;
  switch (what) {
    case 0: src = c->ranges; bytes = sizeof(uint2) * (size_t)c->ntiles; break;
    case 1:
      if (ctx_resolve_count(const_cast<GsrCtx*>(c)) != GSR_OK) return set_err(GSR_ERR_DEVICE, "gsr_ctx_export: reading the pair count failed");
      src = c->pair_rank; bytes = sizeof(uint32_t) * (size_t)(c->overflow ? 0 : c->n64);
      break;
    case 2: src = c->n_contrib; bytes = sizeof(uint32_t) * HW; break;
    case 3: src = c->final_T; bytes = sizeof(float) * HW; break;
    case 4: src = c->order; bytes = sizeof(uint32_t) * PV; break;
    case 5: src = c->off; bytes = sizeof(uint32_t) * (PV + 1); break;
    case 6:                                                                   // (kept for old callers: same as 7)
    case 7: {                                                                 // splat records [P][3] float4, storage order
      const size_t need = sizeof(float4) * 3 * PV;
      if ((int64_t)need > dst_bytes)
        return set_err(GSR_ERR_INVALID, "gsr_ctx_export: item %d needs %zu bytes, buffer has %lld", what, need, (long long)dst_bytes);
      if (PV == 0) return GSR_OK;
      // the records sit REC float4 apart in the workspace: copied out packed, 48 bytes each
      HIP_TRY("ctx export", hipMemcpy2DAsync(dst, sizeof(float4) * 3, c->G0, sizeof(float4) * REC, sizeof(float4) * 3,
                                             PV, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
      return GSR_OK;
    }
    case 8: src = c->dv; bytes = sizeof(uint32_t) * DV_WORDS; break;          // device-side scalars (DV_*)
    case 9: src = c->offg; bytes = sizeof(uint32_t) * (PV + 1); break;
    default: return set_err(GSR_ERR_INVALID, "gsr_ctx_export: unknown item %d", what);
  }
  if ((int64_t)bytes > dst_bytes)
    return set_err(GSR_ERR_INVALID, "gsr_ctx_export: item %d needs %zu bytes, buffer has %lld", what, bytes, (long long)dst_bytes);
  if (bytes == 0) return GSR_OK;
  HIP_TRY("ctx export", hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
  return GSR_OK;
}

void gsr_trim_pool(void) {
  const int dev = cur_dev();
  (void)hipDeviceSynchronize();
  Pool& pl = g_pool[dev];
  std::lock_guard<std::mutex> lk(pl.mu);
  std::vector<Block> keep;
  for (Block& b : pl.blocks) {
    if (b.used) keep.push_back(b);
    else { (void)hipFree(b.p); pl.total -= b.bytes; }
  }
  pl.blocks.swap(keep);
}

int gsr_ctx_set_aux_grads(GsrCtx* c, const float* grad_depth, const float* grad_alpha) {
  if (!c) return set_err(GSR_ERR_STATE, "gsr_ctx_set_aux_grads: null context");
  if (!c->aux)
    return set_err(GSR_ERR_STATE, "gsr_ctx_set_aux_grads: the context's forward did not produce depth / alpha maps (use gsr_forward*_aux)");
  if (c->fwd_only) return set_err(GSR_ERR_STATE, "gsr_ctx_set_aux_grads: the context has no backward state");
  c->aux_gd = grad_depth; c->aux_ga = grad_alpha;
  return GSR_OK;
}

int gsr_ctx_request_sumsq(GsrCtx* c, double* out6) {
  if (!c) return set_err(GSR_ERR_STATE, "gsr_ctx_request_sumsq: null context");
  if (!c->raw || !c->lanegroup)
    return set_err(GSR_ERR_INVALID, "gsr_ctx_request_sumsq: only contexts of gsr_forward_raw (raw parameters) produce the sums");
  if (c->B > 1 && !batch_k9_fused())
    return set_err(GSR_ERR_INVALID, "gsr_ctx_request_sumsq: a batch context under GSR_BATCH_K9=0 runs one accumulating launch per view");
  c->sumsq_out = out6;
  return GSR_OK;
}

int gsr_pgd_step_normed(float* x, const float* grad, const float* x0, int64_t rows, int32_t cols, float alpha, float epsilon,
                        const double* sumsq, void* stream) {
  if (rows < 0 || cols < 1 || cols > PGD_MAX_COLS)
    return set_err(GSR_ERR_INVALID, "gsr_pgd_step_normed: rows=%lld cols=%d (1..%d columns)", (long long)rows, cols, PGD_MAX_COLS);
  if (rows == 0) return GSR_OK;
  if (!x || !grad || !x0 || !sumsq) return set_err(GSR_ERR_INVALID, "gsr_pgd_step_normed: null argument");
  const int64_t rpw = pgd_rows_per_wave(cols);
  hipLaunchKernelGGL((k_pgd_step<true>), dim3((unsigned)((rows + rpw - 1) / rpw)), dim3(64), 0, static_cast<hipStream_t>(stream), x, grad,
                     x0, (size_t)rows, cols, alpha, epsilon, sumsq, 1);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_err(GSR_ERR_DEVICE, "gsr_pgd_step_normed: launch failed: %s", hipGetErrorString(e));
  return GSR_OK;
}

int gsr_pgd_step(float* x, const float* grad, const float* x0, int64_t rows, int32_t cols, float alpha, float epsilon,
                 int32_t l2, void* stream) {
  if (rows < 0 || cols < 1 || cols > PGD_MAX_COLS)
    return set_err(GSR_ERR_INVALID, "gsr_pgd_step: rows=%lld cols=%d (1..%d columns)", (long long)rows, cols, PGD_MAX_COLS);
  if (rows == 0) return GSR_OK;
  if (!x || !grad || !x0) return set_err(GSR_ERR_INVALID, "gsr_pgd_step: null argument");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int dev = cur_dev();
  const size_t n = (size_t)rows * (size_t)cols;
  const int64_t rpw = pgd_rows_per_wave(cols);
  const unsigned blocks = (unsigned)((rows + rpw - 1) / rpw);
  if (!l2) {
    hipLaunchKernelGGL((k_pgd_step<false>), dim3(blocks), dim3(64), 0, st, x, grad, x0, (size_t)rows, cols, alpha, epsilon,
                       (const double*)nullptr, 0);
  } else {
    const int nb = pgd_sumsq_blocks(n);
    void* blk = pool_alloc(dev, sizeof(double) * (size_t)nb, st);
    if (!blk) return set_err(GSR_ERR_NOMEM, "gsr_pgd_step: allocation failed");
    double* partial = static_cast<double*>(blk);
    hipLaunchKernelGGL(k_pgd_sumsq, dim3(nb), dim3(256), 0, st, grad, n, partial);
    hipLaunchKernelGGL((k_pgd_step<true>), dim3(blocks), dim3(64), 0, st, x, grad, x0, (size_t)rows, cols, alpha, epsilon,
                       partial, nb);
    pool_free(dev, blk);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_err(GSR_ERR_DEVICE, "gsr_pgd_step: launch failed: %s", hipGetErrorString(e));
  return GSR_OK;
}

int gsr_pgd_step_multi(int32_t n, float* const* x, const float* const* grad, const float* const* x0, const int64_t* rows,
                       const int32_t* cols, const float* alpha, const float* epsilon, int32_t l2, const double* const* sumsq,
                       void* stream) {
  if (n < 0 || n > PGD_MAX_TENSORS) return set_err(GSR_ERR_INVALID, "gsr_pgd_step_multi: n=%d (0..%d tensors)", n, PGD_MAX_TENSORS);
  if (n == 0) return GSR_OK;
  if (!x || !grad || !x0 || !rows || !cols || !alpha || !epsilon) return set_err(GSR_ERR_INVALID, "gsr_pgd_step_multi: null argument");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int dev = cur_dev();
  PgdMulti m;
  memset(&m, 0, sizeof(m));
  unsigned long long blocks = 0;
  size_t need = 0;                                       // doubles of partial sums this call has to make itself
  for (int t = 0; t < n; ++t) {
    if (rows[t] < 0 || cols[t] < 1 || cols[t] > PGD_MAX_COLS)
      return set_err(GSR_ERR_INVALID, "gsr_pgd_step_multi: tensor %d: rows=%lld cols=%d (1..%d columns)", t, (long long)rows[t], cols[t],
                     PGD_MAX_COLS);
    if (rows[t] > 0 && (!x[t] || !grad[t] || !x0[t])) return set_err(GSR_ERR_INVALID, "gsr_pgd_step_multi: tensor %d: null pointer", t);
    m.x[t] = x[t]; m.g[t] = grad[t]; m.x0[t] = x0[t];
    m.rows[t] = (unsigned long long)rows[t]; m.cols[t] = cols[t]; m.alpha[t] = alpha[t]; m.eps[t] = epsilon[t];
    m.first[t] = (unsigned)blocks;
    blocks += (unsigned long long)((rows[t] + pgd_rows_per_wave(cols[t]) - 1) / pgd_rows_per_wave(cols[t]));
    if (blocks > 0x7fffffffull) return set_err(GSR_ERR_INVALID, "gsr_pgd_step_multi: too many rows for one launch");
    if (l2 && rows[t] > 0) {
      if (sumsq && sumsq[t]) { m.partial[t] = sumsq[t]; m.nb[t] = 1; }
      else {
        m.nb[t] = pgd_sumsq_blocks((size_t)rows[t] * (size_t)cols[t]);
        need += (size_t)m.nb[t];
      }
    }
  }
  for (int t = n; t <= PGD_MAX_TENSORS; ++t) m.first[t] = (unsigned)blocks;
  m.n = n;
  if (blocks == 0) return GSR_OK;
  void* blk = nullptr;
  if (need) {
    blk = pool_alloc(dev, sizeof(double) * need, st);
    if (!blk) return set_err(GSR_ERR_NOMEM, "gsr_pgd_step_multi: allocation failed");
    double* partial = static_cast<double*>(blk);
    for (int t = 0; t < n; ++t) {
      if (!l2 || rows[t] == 0 || m.partial[t]) continue;
      hipLaunchKernelGGL(k_pgd_sumsq, dim3(m.nb[t]), dim3(256), 0, st, grad[t], (size_t)rows[t] * (size_t)cols[t], partial);
      m.partial[t] = partial;
      partial += m.nb[t];
    }
  }
  if (l2) hipLaunchKernelGGL((k_pgd_step_multi<true>), dim3((unsigned)blocks), dim3(64), 0, st, m);
  else hipLaunchKernelGGL((k_pgd_step_multi<false>), dim3((unsigned)blocks), dim3(64), 0, st, m);
  if (blk) pool_free(dev, blk);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_err(GSR_ERR_DEVICE, "gsr_pgd_step_multi: launch failed: %s", hipGetErrorString(e));
  return GSR_OK;
}

int gsr_adam_step_multi(int32_t n, void* const* x, const void* const* g, void* const* m, void* const* v, const int64_t* rows,
                        const int32_t* cols, const float* lr, const float* beta1, const float* beta2, const float* eps,
                        int64_t step, const uint8_t* row_mask, int64_t row_begin, int64_t row_end, void* stream) {
  if (n < 1 || n > ADAM_MAX_TENSORS) return set_err(GSR_ERR_INVALID, "gsr_adam_step_multi: n=%d (1..%d tensors)", n, ADAM_MAX_TENSORS);
  if (step < 1) return set_err(GSR_ERR_INVALID, "gsr_adam_step_multi: step=%lld (the count of this step, >= 1)", (long long)step);
  if (!x || !g || !m || !v || !rows || !cols || !lr || !beta1 || !beta2 || !eps)
    return set_err(GSR_ERR_INVALID, "gsr_adam_step_multi: null argument");
  const bool selected = row_mask != nullptr || row_begin != 0 || row_end != -1;
  AdamMulti a;
  memset(&a, 0, sizeof(a));
  unsigned long long blocks = 0;
  for (int t = 0; t < n; ++t) {
    if (rows[t] < 0 || cols[t] < 1 || cols[t] > ADAM_MAX_COLS)
      return set_err(GSR_ERR_INVALID, "gsr_adam_step_multi: tensor %d: rows=%lld cols=%d (1..%d columns)", t, (long long)rows[t], cols[t],
                     ADAM_MAX_COLS);
    if (rows[t] > 0 && (!x[t] || !g[t] || !m[t] || !v[t])) return set_err(GSR_ERR_INVALID, "gsr_adam_step_multi: tensor %d: null pointer", t);
    if (selected && rows[t] != rows[0])
      return set_err(GSR_ERR_INVALID, "gsr_adam_step_multi: tensor %d has %lld rows, tensor 0 has %lld: a row mask or a row range needs equal row counts",
                     t, (long long)rows[t], (long long)rows[0]);
    if (!std::isfinite(lr[t]) || !std::isfinite(beta1[t]) || !std::isfinite(beta2[t]) || !std::isfinite(eps[t]))
      return set_err(GSR_ERR_INVALID, "gsr_adam_step_multi: tensor %d: lr, beta1, beta2 and eps must be finite", t);
    if (!(beta1[t] >= 0.f && beta1[t] < 1.f) || !(beta2[t] >= 0.f && beta2[t] < 1.f) || eps[t] < 0.f)
      return set_err(GSR_ERR_INVALID, "gsr_adam_step_multi: tensor %d: beta1=%g beta2=%g (both in [0, 1)) eps=%g (>= 0)", t, (double)beta1[t],
                     (double)beta2[t], (double)eps[t]);
    a.x[t] = static_cast<float*>(x[t]); a.g[t] = static_cast<const float*>(g[t]);
    a.m[t] = static_cast<float*>(m[t]); a.v[t] = static_cast<float*>(v[t]);
    a.rows[t] = (unsigned long long)rows[t]; a.cols[t] = cols[t];
    adam_bias_corrections((double)lr[t], (double)beta1[t], (double)beta2[t], (long long)step, &a.step_size[t], &a.sqrt_bc2[t]);
    a.b1[t] = beta1[t]; a.b2[t] = beta2[t]; a.eps[t] = eps[t];
    a.first[t] = (unsigned)blocks;
    blocks += adam_blocks((unsigned long long)rows[t] * (unsigned long long)cols[t]);
    if (blocks > 0x7fffffffull) return set_err(GSR_ERR_INVALID, "gsr_adam_step_multi: too many elements for one launch");
  }
  if (selected) {
    if (row_end == -1) row_end = rows[0];
    if (row_begin < 0 || row_begin > row_end || row_end > rows[0])
      return set_err(GSR_ERR_INVALID, "gsr_adam_step_multi: row range [%lld, %lld) of %lld rows", (long long)row_begin, (long long)row_end,
                     (long long)rows[0]);
    a.row_mask = row_mask; a.row_begin = (unsigned long long)row_begin; a.row_end = (unsigned long long)row_end;
  }
  for (int t = n; t <= ADAM_MAX_TENSORS; ++t) a.first[t] = (unsigned)blocks;
  a.n = n;
  if (blocks == 0 || (selected && row_begin == row_end)) return GSR_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (selected) hipLaunchKernelGGL((k_adam_step_multi<true>), dim3((unsigned)blocks), dim3(ADAM_BLOCK), 0, st, a);
  else hipLaunchKernelGGL((k_adam_step_multi<false>), dim3((unsigned)blocks), dim3(ADAM_BLOCK), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return set_err(GSR_ERR_DEVICE, "gsr_adam_step_multi: launch failed: %s", hipGetErrorString(e));
  return GSR_OK;
}

// ---- adaptive density control (gsr_densify.h / gsr_densify.hip.h): the plan's workspace is the caller's; one read-back (the
// three totals) in gsr_densify_plan, none elsewhere.  Every check is made on the host before the first launch.
struct DensWs {
  uint8_t* code;
  uint32_t *off_keep, *off_clone, *off_split, *sums, *totals;
};

// the workspace's regions: the class codes, the three 0/1 counts (scanned in place, P + 1 words each), the scan's block sums,
// the three totals
static DensWs dens_regions(Carve& c, long long P) {
  DensWs w;
  w.code = c.take<uint8_t>((size_t)P + 1);
  w.off_keep = c.take<uint32_t>((size_t)P + 1);
  w.off_clone = c.take<uint32_t>((size_t)P + 1);
  w.off_split = c.take<uint32_t>((size_t)P + 1);
  w.sums = c.take<uint32_t>((size_t)P / 2048 + 2);
  w.totals = c.take<uint32_t>(4);
  return w;
}

int gsr_densify_plan_bytes(int64_t P, int64_t* bytes) {
  if (P < 0 || P > DENS_MAX_ROWS) return set_err(GSR_ERR_INVALID, "gsr_densify_plan_bytes: P=%lld (0..2^28 rows)", (long long)P);
  if (!bytes) return set_err(GSR_ERR_INVALID, "gsr_densify_plan_bytes: null bytes");
  Carve c;
  dens_regions(c, P);
  *bytes = (int64_t)c.off;
  return GSR_OK;
}

int gsr_densify_stats(const float* grad, const int32_t* radii, const uint8_t* filter, int32_t B, int64_t P, float* accum,
                      float* denom, float* max_radii, void* stream) {
  const char* fn = "gsr_densify_stats";
  if (B < 0 || P < 0 || P > DENS_MAX_ROWS) return set_err(GSR_ERR_INVALID, "%s: B=%d P=%lld (B >= 0, 0..2^28 rows)", fn, B, (long long)P);
  if ((long long)B * (long long)P > 0x7fffffffll) return set_err(GSR_ERR_INVALID, "%s: B * P = %lld beyond 2^31 - 1", fn, (long long)B * (long long)P);
  if (B == 0 || P == 0) return GSR_OK;
  if (!grad || !accum || !denom) return set_err(GSR_ERR_INVALID, "%s: null argument", fn);
  if (!radii && !filter) return set_err(GSR_ERR_INVALID, "%s: neither radii nor a filter: nothing says which Gaussians a view saw", fn);
  if (max_radii && !radii) return set_err(GSR_ERR_INVALID, "%s: max_radii2D needs the radii", fn);
  if (int rc = check_aligned4(fn, grad, radii, accum, denom, max_radii)) return rc;
  hipLaunchKernelGGL(k_densify_stats, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), grad, radii,
                     filter, B, (unsigned)P, accum, denom, max_radii);
  LAUNCH_CHECK(fn);
  return GSR_OK;
}

// the three 0/1 counts scanned in place into exclusive offsets, and the totals read back: the plan's one wait for the device
static int dens_scan_counts(const char* fn, const DensWs& w, uint32_t n, int64_t* counts, hipStream_t st) {
  uint32_t* offs[3] = {w.off_keep, w.off_clone, w.off_split};
  hipError_t e = hipSuccess;
  for (int k = 0; k < 3 && e == hipSuccess; ++k) {
    scan_exclusive_u32(offs[k], offs[k], n, nullptr, w.sums, st);         // in place; offs[k][n] = the total
    e = hipMemcpyAsync(w.totals + k, offs[k] + n, sizeof(uint32_t), hipMemcpyDeviceToDevice, st);
  }
  uint32_t host[3] = {0, 0, 0};
  if (e == hipSuccess) e = hipMemcpyAsync(host, w.totals, sizeof(host), hipMemcpyDeviceToHost, st);   // the call's one read-back
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) return set_err(GSR_ERR_DEVICE, "%s: %s", fn, hipGetErrorString(e));
  for (int k = 0; k < 3; ++k) counts[k] = (int64_t)host[k];
  return GSR_OK;
}

static int dens_params(const char* fn, double max_grad, double min_opacity, double extent, double percent_dense, double max_screen_size,
                       int32_t N, uint32_t flags, DensParams* p) {
  if (flags & ~(DENS_WORLD_PRUNE | DENS_SCREEN_PRUNE)) return set_err(GSR_ERR_INVALID, "%s: unknown flags 0x%x", fn, flags);
  switch (dens_thresholds(max_grad, min_opacity, extent, percent_dense, max_screen_size, N, flags, p)) {
    case 0: return GSR_OK;
    case 1: return set_err(GSR_ERR_INVALID, "%s: max_grad=%g is not a finite float32", fn, max_grad);
    case 2: return set_err(GSR_ERR_INVALID, "%s: extent=%g with percent_dense=%g: log(percent_dense extent) or log(0.1 extent) is not finite", fn,
                           extent, percent_dense);
    case 3: return set_err(GSR_ERR_INVALID, "%s: min_opacity=%g: logit(min_opacity) is not finite (0 < min_opacity < 1)", fn, min_opacity);
    case 4: return set_err(GSR_ERR_INVALID, "%s: N=%d (1..%d children)", fn, N, DENS_MAX_N);
    default: return set_err(GSR_ERR_INVALID, "%s: max_screen_size=%g is not a finite float32", fn, max_screen_size);
  }
}

int gsr_densify_plan(const float* accum, const float* denom, const float* scaling, const float* opacity, const float* max_radii,
                     int64_t P, double max_grad, double min_opacity, double extent, double percent_dense, double max_screen_size,
                     int32_t N, uint32_t flags, void* ws, int64_t ws_bytes, int64_t* counts, void* stream) {
  const char* fn = "gsr_densify_plan";
  if (P < 0 || P > DENS_MAX_ROWS) return set_err(GSR_ERR_INVALID, "%s: P=%lld (0..2^28 rows)", fn, (long long)P);
  if (!counts) return set_err(GSR_ERR_INVALID, "%s: null counts", fn);
  DensParams p;
  if (int rc = dens_params(fn, max_grad, min_opacity, extent, percent_dense, max_screen_size, N, flags, &p)) return rc;
  counts[0] = counts[1] = counts[2] = 0;
  if (P == 0) return GSR_OK;
  if (!accum || !denom || !scaling || !opacity) return set_err(GSR_ERR_INVALID, "%s: null argument", fn);
  if ((flags & DENS_SCREEN_PRUNE) && !max_radii) return set_err(GSR_ERR_INVALID, "%s: screen_prune needs max_radii2D", fn);
  if (int rc = check_aligned4(fn, accum, denom, scaling, opacity, max_radii)) return rc;
  Carve c(ws);
  DensWs w = dens_regions(c, P);
  if (!ws) return set_err(GSR_ERR_INVALID, "%s: null workspace", fn);
  if (int rc = check_workspace(fn, ws, ws_bytes, c.off, 16, "gsr_densify_plan_bytes")) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uint32_t n = (uint32_t)P;
  hipLaunchKernelGGL(k_densify_classify, dim3((n + 255) / 256), dim3(256), 0, st, accum, denom, scaling, opacity, max_radii, n, p, w.code,
                     w.off_keep, w.off_clone, w.off_split);
  return dens_scan_counts(fn, w, n, counts, st);
}

int gsr_densify_plan_prune(const uint8_t* prune_mask, int64_t P, void* ws, int64_t ws_bytes, int64_t* counts, void* stream) {
  const char* fn = "gsr_densify_plan_prune";
  if (P < 0 || P > DENS_MAX_ROWS) return set_err(GSR_ERR_INVALID, "%s: P=%lld (0..2^28 rows)", fn, (long long)P);
  if (!counts) return set_err(GSR_ERR_INVALID, "%s: null counts", fn);
  counts[0] = counts[1] = counts[2] = 0;
  if (P == 0) return GSR_OK;
  if (!prune_mask) return set_err(GSR_ERR_INVALID, "%s: null mask", fn);
  Carve c(ws);
  DensWs w = dens_regions(c, P);
  if (!ws) return set_err(GSR_ERR_INVALID, "%s: null workspace", fn);
  if (int rc = check_workspace(fn, ws, ws_bytes, c.off, 16, "gsr_densify_plan_bytes")) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uint32_t n = (uint32_t)P;
  hipLaunchKernelGGL(k_densify_classify_mask, dim3((n + 255) / 256), dim3(256), 0, st, prune_mask, n, w.code, w.off_keep, w.off_clone, w.off_split);
  return dens_scan_counts(fn, w, n, counts, st);
}

static bool dens_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a && b && na && nb && a0 < b0 + nb && b0 < a0 + na;
}

int gsr_densify_apply(const void* ws, int64_t ws_bytes, int64_t P, const int64_t* counts, int32_t n, const void* const* src,
                      void* const* dst, const void* const* m_src, const void* const* v_src, void* const* m_dst, void* const* v_dst,
                      const int32_t* cols, const int32_t* roles, const float* rotation, int32_t N, uint32_t seed, const float* normals,
                      const uint8_t* mask_in, uint8_t* mask_out, int32_t* origin, int32_t* kind, void* stream) {
  const char* fn = "gsr_densify_apply";
  if (N < 1 || N > DENS_MAX_N) return set_err(GSR_ERR_INVALID, "%s: N=%d (1..%d children)", fn, N, DENS_MAX_N);
  if (n < 0 || n > DENS_MAX_TENSORS) return set_err(GSR_ERR_INVALID, "%s: n=%d (0..%d tensors)", fn, n, DENS_MAX_TENSORS);
  if (P < 0 || P > DENS_MAX_ROWS) return set_err(GSR_ERR_INVALID, "%s: P=%lld (0..2^28 rows)", fn, (long long)P);
  if (!counts || (n > 0 && (!src || !dst || !cols || !roles))) return set_err(GSR_ERR_INVALID, "%s: null argument", fn);
  if ((m_src || v_src || m_dst || v_dst) && !(m_src && v_src && m_dst && v_dst))
    return set_err(GSR_ERR_INVALID, "%s: the four moment tables come together", fn);
  if ((origin != nullptr) != (kind != nullptr)) return set_err(GSR_ERR_INVALID, "%s: origin and kind come together", fn);
  if (mask_in && !mask_out) return set_err(GSR_ERR_INVALID, "%s: a row mask in needs a row mask out", fn);
  for (int k = 0; k < 3; ++k)
    if (counts[k] < 0 || counts[k] > P) return set_err(GSR_ERR_INVALID, "%s: counts[%d]=%lld of P=%lld rows", fn, k, (long long)counts[k], (long long)P);
  const long long Pn = (long long)counts[0] + (long long)counts[1] + (long long)N * (long long)counts[2];
  if (Pn > DENS_MAX_ROWS) return set_err(GSR_ERR_INVALID, "%s: P'=%lld rows (at most 2^28)", fn, Pn);
  DensMove a;
  memset(&a, 0, sizeof(a));
  unsigned long long blocks = 0;
  int t_xyz = -1, t_scale = -1;
  for (int t = 0; t < n; ++t) {
    if (cols[t] < 1 || cols[t] > DENS_MAX_COLS) return set_err(GSR_ERR_INVALID, "%s: tensor %d: cols=%d (1..%d columns)", fn, t, cols[t], DENS_MAX_COLS);
    if (roles[t] != DENS_COPY && roles[t] != DENS_XYZ && roles[t] != DENS_SCALE) return set_err(GSR_ERR_INVALID, "%s: tensor %d: role %d", fn, t, roles[t]);
    if ((roles[t] == DENS_XYZ || roles[t] == DENS_SCALE) && cols[t] != 3)
      return set_err(GSR_ERR_INVALID, "%s: tensor %d: the XYZ and SCALE tensors have 3 columns, not %d", fn, t, cols[t]);
    if (roles[t] == DENS_XYZ) { if (t_xyz >= 0) return set_err(GSR_ERR_INVALID, "%s: two XYZ tensors", fn); t_xyz = t; }
    if (roles[t] == DENS_SCALE) { if (t_scale >= 0) return set_err(GSR_ERR_INVALID, "%s: two SCALE tensors", fn); t_scale = t; }
    if ((P > 0 && !src[t]) || (Pn > 0 && !dst[t])) return set_err(GSR_ERR_INVALID, "%s: tensor %d: null pointer", fn, t);
    const bool state = m_src && m_src[t];
    if (m_src && (state != (v_src[t] != nullptr) || (Pn > 0 && state != (m_dst[t] != nullptr)) || (Pn > 0 && state != (v_dst[t] != nullptr))))
      return set_err(GSR_ERR_INVALID, "%s: tensor %d: a moment pair needs all of m, v in and out", fn, t);
    a.src[t] = static_cast<const float*>(src[t]); a.dst[t] = static_cast<float*>(dst[t]);
    if (state) {
      a.m_src[t] = static_cast<const float*>(m_src[t]); a.v_src[t] = static_cast<const float*>(v_src[t]);
      a.m_dst[t] = static_cast<float*>(m_dst[t]); a.v_dst[t] = static_cast<float*>(v_dst[t]);
    }
    if (((uintptr_t)a.src[t] | (uintptr_t)a.dst[t] | (uintptr_t)a.m_src[t] | (uintptr_t)a.v_src[t] | (uintptr_t)a.m_dst[t] | (uintptr_t)a.v_dst[t]) & 3)
      return set_err(GSR_ERR_INVALID, "%s: tensor %d: every tensor must be 4-byte aligned", fn, t);
    a.cols[t] = cols[t]; a.role[t] = roles[t];
    a.first[t] = (unsigned)blocks;
    blocks += dens_blocks((unsigned long long)P * (unsigned long long)cols[t]);
  }
  if (counts[2] > 0 && t_xyz >= 0 && (t_scale < 0 || !rotation))
    return set_err(GSR_ERR_INVALID, "%s: the XYZ tensor's children need the SCALE tensor and the rotation", fn);
  if (int rc = check_aligned4(fn, rotation, normals, origin, kind)) return rc;
  // nothing that is written may overlap anything that is read (the move is not in place): every source, moment, the rotation,
  // the normals, the row mask and the plan's workspace against every destination, moment, mask_out, origin and kind
  {
    struct Span { const void* p; size_t n; const char* what; };
    std::vector<Span> rd, wr;
    for (int t = 0; t < n; ++t) {
      const size_t sb = (size_t)P * cols[t] * 4, db = (size_t)Pn * cols[t] * 4;
      rd.push_back({a.src[t], sb, "a source tensor"}); rd.push_back({a.m_src[t], sb, "a source moment"}); rd.push_back({a.v_src[t], sb, "a source moment"});
      wr.push_back({a.dst[t], db, "a destination tensor"}); wr.push_back({a.m_dst[t], db, "a destination moment"});
      wr.push_back({a.v_dst[t], db, "a destination moment"});
    }
    rd.push_back({rotation, (size_t)P * 16, "the rotation"});
    rd.push_back({normals, (size_t)P * (size_t)N * 12, "the normals"});
    rd.push_back({mask_in, (size_t)P, "the row mask"});
    if (ws && ws_bytes > 0) rd.push_back({ws, (size_t)ws_bytes, "the workspace"});
    wr.push_back({mask_out, (size_t)Pn, "the row mask out"});
    wr.push_back({origin, (size_t)Pn * 4, "origin"});
    wr.push_back({kind, (size_t)Pn * 4, "kind"});
    for (const Span& w : wr)
      for (const Span& r : rd)
        if (dens_overlap(r.p, r.n, w.p, w.n))
          return set_err(GSR_ERR_INVALID, "%s: %s overlaps %s: the move is not in place", fn, w.what, r.what);
    for (size_t i = 0; i < wr.size(); ++i)
      for (size_t j = i + 1; j < wr.size(); ++j)
        if (dens_overlap(wr[i].p, wr[i].n, wr[j].p, wr[j].n))
          return set_err(GSR_ERR_INVALID, "%s: %s overlaps %s: two outputs share memory", fn, wr[i].what, wr[j].what);
  }
  if (Pn == 0 || P == 0) return GSR_OK;
  Carve c(const_cast<void*>(ws));
  DensWs w = dens_regions(c, P);
  if (!ws) return set_err(GSR_ERR_INVALID, "%s: null workspace", fn);
  if (int rc = check_workspace(fn, ws, ws_bytes, c.off, 16, "gsr_densify_plan_bytes")) return rc;
  const bool table = mask_out || origin;
  const unsigned long long grid = blocks + (table ? ((unsigned long long)P + DENS_SPAN - 1) / DENS_SPAN : 0ull);
  if (grid > 0x7fffffffull) return set_err(GSR_ERR_INVALID, "%s: too many elements for one launch", fn);
  for (int t = n; t <= DENS_MAX_TENSORS; ++t) a.first[t] = (unsigned)blocks;
  a.n = n; a.P = (unsigned)P;
  a.n_keep = (unsigned)counts[0]; a.n_clone = (unsigned)counts[1]; a.n_split = (unsigned)counts[2];
  a.code = w.code; a.off_keep = w.off_keep; a.off_clone = w.off_clone; a.off_split = w.off_split;
  a.xyz = t_xyz >= 0 ? a.src[t_xyz] : nullptr; a.scale = t_scale >= 0 ? a.src[t_scale] : nullptr; a.rot = rotation;
  a.normals = normals; a.seed = seed; a.N = N;
  a.c = (float)log(0.8 * (double)N);
  a.mask_in = mask_in; a.mask_out = mask_out; a.origin = origin; a.kind = kind;
  if (grid == 0) return GSR_OK;
  hipLaunchKernelGGL(k_densify_move, dim3((unsigned)grid), dim3(DENS_BLOCK), 0, static_cast<hipStream_t>(stream), a);
  LAUNCH_CHECK(fn);
  return GSR_OK;
}

// ---- detection metrics (gsr_deteval.h / gsr_deteval.hip.h): no allocation, no copy, no host wait; every check is made on
// the host before the first device call.
static int deteval_spec(const char* fn, const GsrDetEvalSpec* spec, gsr_de::Spec* s) {
  static_assert(sizeof(GsrDetEvalSpec) == sizeof(gsr_de::Spec), "GsrDetEvalSpec and gsr_de::Spec are one layout");
  if (!spec) return set_err(GSR_ERR_INVALID, "%s: null spec", fn);
  memcpy(s, spec, sizeof(*s));
  if (const char* why = gsr_de::spec_error(*s)) return set_err(GSR_ERR_INVALID, "%s: bad spec: %s", fn, why);
  return GSR_OK;
}

struct DeWs {
  uint32_t *k0, *v0, *k1, *v1, *cls, *table, *sums, *count, *off, *scan_sums;
};

static DeWs deteval_regions(Carve& c, const gsr_de::Spec& s, long long N) {
  const size_t n = (size_t)N * (size_t)s.D;
  DeWs w;
  w.k0 = c.take<uint32_t>(n);
  w.v0 = c.take<uint32_t>(n);
  w.k1 = c.take<uint32_t>(n);
  w.v1 = c.take<uint32_t>(n);
  w.cls = c.take<uint32_t>(n);
  w.table = c.take<uint32_t>(radix_table_words((uint32_t)n));
  w.sums = c.take<uint32_t>(RS_BINS);
  w.count = c.take<uint32_t>((size_t)s.K + 2);
  w.off = c.take<uint32_t>((size_t)s.K + 2);
  w.scan_sums = c.take<uint32_t>((size_t)(s.K + 1) / 2048 + 2);
  return w;
}

static int deteval_rows(const char* fn, const gsr_de::Spec& s, int64_t N) {
  if (N < 1 || N * (int64_t)s.D > gsr_de::MAX_ROWS)
    return set_err(GSR_ERR_INVALID, "%s: N=%lld images of D=%d detections (N >= 1, N * D <= 2^20)", fn, (long long)N, s.D);
  return GSR_OK;
}

int gsr_deteval_workspace_bytes(const GsrDetEvalSpec* spec, int64_t N, int64_t* bytes) {
  const char* fn = "gsr_deteval_workspace_bytes";
  gsr_de::Spec s;
  if (int rc = deteval_spec(fn, spec, &s)) return rc;
  if (int rc = deteval_rows(fn, s, N)) return rc;
  if (!bytes) return set_err(GSR_ERR_INVALID, "%s: null bytes", fn);
  Carve c;
  deteval_regions(c, s, N);
  *bytes = (int64_t)c.off;
  return GSR_OK;
}

int gsr_deteval_match(const GsrDetEvalSpec* spec, int32_t B, const float* dets, const int32_t* counts, const float* gt_boxes,
                      const int32_t* gt_cls, int32_t* dt_order, int32_t* dt_rank, int32_t* dt_match, uint8_t* dt_ignore,
                      uint8_t* gt_ignore, int32_t* gt_match, void* stream) {
  const char* fn = "gsr_deteval_match";
  gsr_de::Spec s;
  if (int rc = deteval_spec(fn, spec, &s)) return rc;
  if (B < 1 || (long long)B * s.D > gsr_de::MAX_ROWS) return set_err(GSR_ERR_INVALID, "%s: B=%d images of D=%d detections (B >= 1, B * D <= 2^20)", fn, B, s.D);
  if (!dets || !counts || !dt_order || !dt_rank || !dt_match || !dt_ignore) return set_err(GSR_ERR_INVALID, "%s: null dets / counts / dt_order / dt_rank / dt_match / dt_ignore", fn);
  if (s.M > 0 && (!gt_boxes || !gt_cls || !gt_ignore || !gt_match)) return set_err(GSR_ERR_INVALID, "%s: null gt_boxes / gt_cls / gt_ignore / gt_match with M=%d", fn, s.M);
  if (int rc = check_aligned4(fn, dets, counts, gt_boxes, gt_cls, dt_order, dt_rank, dt_match, gt_match)) return rc;
  int P = 2;                                                // the sort's width: the power of two at or above D
  while (P < s.D) P <<= 1;
  hipLaunchKernelGGL(gsr_de::k_de_match, dim3((unsigned)B), dim3(gsr_de::MATCH_THREADS), (size_t)P * 10, static_cast<hipStream_t>(stream), s, P,
                     dets, counts, gt_boxes, gt_cls, dt_order, dt_rank, dt_match, dt_ignore, gt_ignore, gt_match);
  LAUNCH_CHECK(fn);
  return GSR_OK;
}

int gsr_deteval_accumulate(const GsrDetEvalSpec* spec, int64_t N, const float* dets, const int32_t* dt_order, const int32_t* dt_rank,
                           const int32_t* dt_match, const uint8_t* dt_ignore, const int32_t* gt_cls, const uint8_t* gt_ignore,
                           const double* rec_thrs, void* ws, int64_t ws_bytes, double* precision, double* scores, double* recall,
                           int32_t* npig, void* stream) {
  const char* fn = "gsr_deteval_accumulate";
  gsr_de::Spec s;
  if (int rc = deteval_spec(fn, spec, &s)) return rc;
  if (int rc = deteval_rows(fn, s, N)) return rc;
  if (!dets || !dt_order || !dt_rank || !dt_match || !dt_ignore || !rec_thrs || !precision || !scores || !recall || !npig)
    return set_err(GSR_ERR_INVALID, "%s: null dets / dt_order / dt_rank / dt_match / dt_ignore / rec_thrs / precision / scores / recall / npig", fn);
  if (s.M > 0 && (!gt_cls || !gt_ignore)) return set_err(GSR_ERR_INVALID, "%s: null gt_cls / gt_ignore with M=%d", fn, s.M);
  if (int rc = check_aligned4(fn, dets, dt_order, dt_rank, dt_match, gt_cls, npig)) return rc;
  if ((((uintptr_t)rec_thrs | (uintptr_t)precision | (uintptr_t)scores | (uintptr_t)recall) & 7) != 0)
    return set_err(GSR_ERR_INVALID, "%s: rec_thrs, precision, scores and recall must be 8-byte aligned", fn);
  if (!ws) return set_err(GSR_ERR_INVALID, "%s: null workspace", fn);
  Carve c(ws);
  DeWs w = deteval_regions(c, s, N);
  if (int rc = check_workspace(fn, ws, ws_bytes, c.off, 16, "gsr_deteval_workspace_bytes")) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uint32_t n = (uint32_t)(N * s.D);
  HIP_TRY(fn, hipMemsetAsync(w.count, 0, sizeof(uint32_t) * ((size_t)s.K + 2), st));
  HIP_TRY(fn, hipMemsetAsync(npig, 0, sizeof(int32_t) * (size_t)s.K * (size_t)s.A, st));
  hipLaunchKernelGGL(gsr_de::k_de_keys, dim3((n + 255) / 256), dim3(256), 0, st, dets, dt_order, n, s.D, s.K, w.k0, w.cls, w.count);
  // two stable sorts: by score descending (the values start as image * D + position, so equal scores stay in image, then rank
  // order), then by class
  const int r1 = radix_sort_pairs(w.k0, w.v0, w.k1, w.v1, n, nullptr, 0, 32, true, w.table, w.sums, st);
  uint32_t *ka = r1 ? w.k1 : w.k0, *va = r1 ? w.v1 : w.v0, *kb = r1 ? w.k0 : w.k1, *vb = r1 ? w.v0 : w.v1;
  hipLaunchKernelGGL(gsr_de::k_de_classes, dim3((n + 255) / 256), dim3(256), 0, st, (const uint32_t*)va, (const uint32_t*)w.cls, n, ka);
  int class_bits = 1;
  while ((s.K >> class_bits) != 0) ++class_bits;             // the keys are 0 .. K
  const int r2 = radix_sort_pairs(ka, va, kb, vb, n, nullptr, 0, class_bits, false, w.table, w.sums, st);
  scan_exclusive_u32(w.count, w.off, (uint32_t)s.K + 1u, nullptr, w.scan_sums, st);
  if (s.M > 0) {
    const uint32_t total = (uint32_t)(N * s.A * s.M);
    hipLaunchKernelGGL(gsr_de::k_de_npig, dim3((total + 255) / 256), dim3(256), 0, st, gt_cls, gt_ignore, total, s.A, s.M, s.K, npig);
  }
  gsr_de::CurveArgs a;
  a.dets = dets; a.dt_order = dt_order; a.dt_rank = dt_rank; a.dt_match = dt_match; a.dt_ignore = dt_ignore;
  a.vals = r2 ? vb : va; a.off = w.off; a.npig = npig; a.rec_thrs = rec_thrs;
  a.precision = precision; a.scores = scores; a.recall = recall;
  hipLaunchKernelGGL(gsr_de::k_de_curve, dim3((unsigned)s.K * (unsigned)(s.A * s.n_caps * s.T)), dim3(gsr_de::ACC_CHUNK), sizeof(double) * 2 * (size_t)s.R, st, s, a);
  LAUNCH_CHECK(fn);
  return GSR_OK;
}

int gsr_deteval_summarize(const GsrDetEvalSpec* spec, const double* precision, const double* recall, double* stats, void* stream) {
  const char* fn = "gsr_deteval_summarize";
  gsr_de::Spec s;
  if (int rc = deteval_spec(fn, spec, &s)) return rc;
  if (!precision || !recall || !stats) return set_err(GSR_ERR_INVALID, "%s: null precision / recall / stats", fn);
  if ((((uintptr_t)precision | (uintptr_t)recall | (uintptr_t)stats) & 7) != 0)
    return set_err(GSR_ERR_INVALID, "%s: precision, recall and stats must be 8-byte aligned", fn);
  hipLaunchKernelGGL(gsr_de::k_de_summarize, dim3(1), dim3(gsr_de::N_STATS * 64), 0, static_cast<hipStream_t>(stream), s, precision, recall, stats);
  LAUNCH_CHECK(fn);
  return GSR_OK;
}

int gsr_knn_dist2(const float* points, int32_t P, float* mean_dist2, void* stream) {
  if (P < 0 || (P > 0 && (!points || !mean_dist2))) return set_err(GSR_ERR_INVALID, "gsr_knn_dist2: null argument");
  if (P == 0) return GSR_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int dev = cur_dev();
  const uint32_t n = (uint32_t)P;
  const uint32_t tbl = radix_table_words(n);
  // ---- bounding box (one small read-back: this routine is scene set-up, not the per-view path) ----------------
  float host_bb[6] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
  void* bb_blk = pool_alloc(dev, 256, st);
  if (!bb_blk) return set_err(GSR_ERR_NOMEM, "gsr_knn_dist2: allocation failed");
  float* bbox = static_cast<float*>(bb_blk);
  hipError_t e = hipMemcpyAsync(bbox, host_bb, sizeof(host_bb), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_knn_bbox, dim3(std::min<uint32_t>((n + 255) / 256, 1024u)), dim3(256), 0, st, points, P, bbox);
    e = hipMemcpyAsync(host_bb, bbox, sizeof(host_bb), hipMemcpyDeviceToHost, st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  pool_free(dev, bb_blk);
  if (e != hipSuccess) return set_err(GSR_ERR_DEVICE, "gsr_knn_dist2: bounding box: %s", hipGetErrorString(e));
  // ---- grid: about three points per cell, at most 256 cells per axis ---------------------------------------------
  const KnnGrid g = knn_make_grid(host_bb, P);   // gsr_knn.h
  const uint32_t ncells = (uint32_t)g.dx * g.dy * g.dz;
  // ---- workspace -----------------------------------------------------------------------------------------------
  const size_t words = (size_t)4 * n + tbl + RS_BINS + 2 * (size_t)ncells + 64;
  void* blk = pool_alloc(dev, sizeof(uint32_t) * words, st);
  if (!blk) return set_err(GSR_ERR_NOMEM, "gsr_knn_dist2: workspace allocation failed");
  uint32_t* k0 = static_cast<uint32_t*>(blk);
  uint32_t* v0 = k0 + n; uint32_t* k1 = v0 + n; uint32_t* v1 = k1 + n;
  uint32_t* table = v1 + n; uint32_t* sums = table + tbl;
  uint2* cell_range = reinterpret_cast<uint2*>(sums + RS_BINS + (((uintptr_t)(sums + RS_BINS) & 4) ? 1 : 0));
  hipLaunchKernelGGL(k_knn_cells, dim3((n + 255) / 256), dim3(256), 0, st, points, P, g, k0);
  const int res = radix_sort_pairs(k0, v0, k1, v1, n, nullptr, 0, ceil_log2(ncells), true, table, sums, st);
  const uint32_t* skeys = res ? k1 : k0;
  const uint32_t* sidx = res ? v1 : v0;
  if (ceil_log2(ncells) == 0) {   // a single cell: no pass ran, build the identity permutation by hand
    std::vector<uint32_t> iota(n);
    for (uint32_t i = 0; i < n; ++i) iota[i] = i;
    (void)hipMemcpyAsync(v0, iota.data(), sizeof(uint32_t) * n, hipMemcpyHostToDevice, st);
    (void)hipStreamSynchronize(st);
  }
  (void)hipMemsetAsync(cell_range, 0, sizeof(uint2) * ncells, st);
  hipLaunchKernelGGL(k_knn_ranges, dim3((n + 255) / 256), dim3(256), 0, st, n, skeys, cell_range);
  hipLaunchKernelGGL(k_knn_search, dim3((n + 255) / 256), dim3(256), 0, st, points, P, g, sidx, cell_range, mean_dist2);
  pool_free(dev, blk);
  LAUNCH_CHECK("knn");
  return GSR_OK;
}

int gsr_knn_query(const float* ref, int32_t R, const float* qry, int32_t Q, int32_t k, uint32_t flags, int32_t* out_idx,
                  float* out_d2, void* stream) {
  if (k < 1 || k > KNNQ_MAX_K) return set_err(GSR_ERR_INVALID, "gsr_knn_query: k=%d (1..%d)", k, KNNQ_MAX_K);
  if (R < 0 || Q < 0) return set_err(GSR_ERR_INVALID, "gsr_knn_query: R=%d Q=%d", R, Q);
  if (flags & ~KNNQ_EXCLUDE_SAME_INDEX) return set_err(GSR_ERR_INVALID, "gsr_knn_query: unknown flags 0x%x", flags);
  if ((flags & KNNQ_EXCLUDE_SAME_INDEX) && Q != R)
    return set_err(GSR_ERR_INVALID, "gsr_knn_query: EXCLUDE_SAME_INDEX is the self-query, Q=%d must equal R=%d", Q, R);
  if ((R > 0 && !ref) || (Q > 0 && (!qry || !out_idx))) return set_err(GSR_ERR_INVALID, "gsr_knn_query: null argument");
  if (Q == 0) return GSR_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uint32_t nq = (uint32_t)Q, nr = (uint32_t)R;
  if (R == 0) {   // no reference: every slot is missing, no grid
    const size_t n = (size_t)Q * (size_t)k;
    hipLaunchKernelGGL(k_knnq_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, out_idx, out_d2);
    LAUNCH_CHECK("gsr_knn_query");
    return GSR_OK;
  }
  const int dev = cur_dev();
  // ---- the references' bounding box, as gsr_knn_dist2 reads it (the one wait for the device) --------------------------
  float host_bb[6] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
  void* bb_blk = pool_alloc(dev, 256, st);
  if (!bb_blk) return set_err(GSR_ERR_NOMEM, "gsr_knn_query: allocation failed");
  float* bbox = static_cast<float*>(bb_blk);
  hipError_t e = hipMemcpyAsync(bbox, host_bb, sizeof(host_bb), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_knn_bbox, dim3(std::min<uint32_t>((nr + 255) / 256, 1024u)), dim3(256), 0, st, ref, R, bbox);
    e = hipMemcpyAsync(host_bb, bbox, sizeof(host_bb), hipMemcpyDeviceToHost, st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  pool_free(dev, bb_blk);
  if (e != hipSuccess) return set_err(GSR_ERR_DEVICE, "gsr_knn_query: bounding box: %s", hipGetErrorString(e));
  const KnnGrid g = knn_make_grid(host_bb, R);   // gsr_knn.h
  const uint32_t ncells = (uint32_t)g.dx * g.dy * g.dz;
  const int bits = ceil_log2(ncells);
  // ---- workspace: staged references | cell ranges | 4 sort arrays of R | 4 sort arrays of Q | table | sums -----------
  const uint32_t tbl = radix_table_words(std::max(nr, nq));
  const size_t words = (size_t)4 * nr + 2 * (size_t)ncells + (size_t)4 * nr + (size_t)4 * nq + tbl + RS_BINS;
  void* blk = pool_alloc(dev, sizeof(uint32_t) * words, st);
  if (!blk) return set_err(GSR_ERR_NOMEM, "gsr_knn_query: workspace allocation failed");
  KnnqRef* staged = static_cast<KnnqRef*>(blk);                               // 16 bytes each, the block is 256-byte aligned
  uint2* cell_range = reinterpret_cast<uint2*>(staged + nr);
  uint32_t* k0 = reinterpret_cast<uint32_t*>(cell_range + ncells);
  uint32_t* v0 = k0 + nr; uint32_t* k1 = v0 + nr; uint32_t* v1 = k1 + nr;
  uint32_t* qk0 = v1 + nr; uint32_t* qv0 = qk0 + nq; uint32_t* qk1 = qv0 + nq; uint32_t* qv1 = qk1 + nq;
  uint32_t* table = qv1 + nq; uint32_t* sums = table + tbl;
  // ---- references: cell keys, sort, ranges, cell-sorted copy ----------------------------------------------------------
  hipLaunchKernelGGL(k_knn_cells, dim3((nr + 255) / 256), dim3(256), 0, st, ref, R, g, k0);
  const int res = radix_sort_pairs(k0, v0, k1, v1, nr, nullptr, 0, bits, true, table, sums, st);
  const uint32_t* skeys = res ? k1 : k0;
  const uint32_t* sidx = res ? v1 : v0;
  if (bits == 0) hipLaunchKernelGGL(k_knnq_iota, dim3((nr + 255) / 256), dim3(256), 0, st, nr, v0);   // one cell: no pass ran
  (void)hipMemsetAsync(cell_range, 0, sizeof(uint2) * ncells, st);
  hipLaunchKernelGGL(k_knn_ranges, dim3((nr + 255) / 256), dim3(256), 0, st, nr, skeys, cell_range);
  hipLaunchKernelGGL(k_knnq_stage, dim3((nr + 255) / 256), dim3(256), 0, st, ref, nr, sidx, staged);
  // ---- queries: their cell keys in the REFERENCE grid, sorted, so that neighbouring lanes scan the same cells ---------
  hipLaunchKernelGGL(k_knn_cells, dim3((nq + 255) / 256), dim3(256), 0, st, qry, Q, g, qk0);
  const int qres = radix_sort_pairs(qk0, qv0, qk1, qv1, nq, nullptr, 0, bits, true, table, sums, st);
  const uint32_t* qsidx = qres ? qv1 : qv0;
  if (bits == 0) hipLaunchKernelGGL(k_knnq_iota, dim3((nq + 255) / 256), dim3(256), 0, st, nq, qv0);
  const uint32_t qb = (nq + 255) / 256;
  const int excl = (flags & KNNQ_EXCLUDE_SAME_INDEX) ? 1 : 0;
  switch (k) {
    case 1: launch_knnq_query<1>(qb, st, staged, R, g, cell_range, qry, Q, qsidx, excl, out_idx, out_d2); break;
    case 2: launch_knnq_query<2>(qb, st, staged, R, g, cell_range, qry, Q, qsidx, excl, out_idx, out_d2); break;
    case 3: launch_knnq_query<3>(qb, st, staged, R, g, cell_range, qry, Q, qsidx, excl, out_idx, out_d2); break;
    case 4: launch_knnq_query<4>(qb, st, staged, R, g, cell_range, qry, Q, qsidx, excl, out_idx, out_d2); break;
    case 5: launch_knnq_query<5>(qb, st, staged, R, g, cell_range, qry, Q, qsidx, excl, out_idx, out_d2); break;
    case 6: launch_knnq_query<6>(qb, st, staged, R, g, cell_range, qry, Q, qsidx, excl, out_idx, out_d2); break;
    case 7: launch_knnq_query<7>(qb, st, staged, R, g, cell_range, qry, Q, qsidx, excl, out_idx, out_d2); break;
    default: launch_knnq_query<8>(qb, st, staged, R, g, cell_range, qry, Q, qsidx, excl, out_idx, out_d2); break;
  }
  pool_free(dev, blk);
  LAUNCH_CHECK("gsr_knn_query");
  return GSR_OK;
}

int gsr_knn_gather_mean(const int32_t* idx, int32_t Q, int32_t k, int32_t R, int32_t n_tensors, const float* const* src,
                        const int32_t* cols, float* const* dst, void* stream) {
  if (k < 1 || k > KNNQ_MAX_K) return set_err(GSR_ERR_INVALID, "gsr_knn_gather_mean: k=%d (1..%d)", k, KNNQ_MAX_K);
  if (R < 0 || Q < 0) return set_err(GSR_ERR_INVALID, "gsr_knn_gather_mean: R=%d Q=%d", R, Q);
  if (n_tensors < 1 || n_tensors > KNNQ_MAX_TENSORS)
    return set_err(GSR_ERR_INVALID, "gsr_knn_gather_mean: %d tensors (1..%d)", n_tensors, KNNQ_MAX_TENSORS);
  if (!src || !cols || !dst) return set_err(GSR_ERR_INVALID, "gsr_knn_gather_mean: null argument");
  KnnqGather a;
  memset(&a, 0, sizeof(a));
  int total = 0;
  for (int t = 0; t < n_tensors; ++t) {
    if (cols[t] < 1 || cols[t] > KNNQ_MAX_COLS)
      return set_err(GSR_ERR_INVALID, "gsr_knn_gather_mean: tensor %d: %d columns (1..%d)", t, cols[t], KNNQ_MAX_COLS);
    a.first[t] = total;
    total += cols[t];
    if (total > KNNQ_MAX_COLS) return set_err(GSR_ERR_INVALID, "gsr_knn_gather_mean: more than %d columns in all", KNNQ_MAX_COLS);
    a.cols[t] = cols[t];
  }
  for (int t = n_tensors; t <= KNNQ_MAX_TENSORS; ++t) a.first[t] = total;
  a.total = total;
  if (Q > 0) {
    if (!idx) return set_err(GSR_ERR_INVALID, "gsr_knn_gather_mean: null idx");
    for (int t = 0; t < n_tensors; ++t) {
      if (!dst[t] || (R > 0 && !src[t])) return set_err(GSR_ERR_INVALID, "gsr_knn_gather_mean: tensor %d: null pointer", t);
      a.src[t] = src[t]; a.dst[t] = dst[t];
    }
  }
  if (Q == 0) return GSR_OK;
  const size_t n = (size_t)Q * (size_t)total;
  hipLaunchKernelGGL(k_knnq_gather_mean, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), idx,
                     (size_t)Q, k, R, a);
  LAUNCH_CHECK("gsr_knn_gather_mean");
  return GSR_OK;
}

int gsr_group_classify(const float* objects, int32_t P, const float* W, const float* b, int32_t C, const int32_t* ids,
                       int32_t nids, float thresh, float* psel, uint8_t* mask, void* stream) {
  if (P < 0) return set_err(GSR_ERR_INVALID, "gsr_group_classify: P=%d", P);
  if (C < 1 || C > GROUP_MAX_CLASSES) return set_err(GSR_ERR_INVALID, "gsr_group_classify: C=%d classes (1..%d)", C, GROUP_MAX_CLASSES);
  if (!ids || nids < 1 || nids > C) return set_err(GSR_ERR_INVALID, "gsr_group_classify: %d selected ids (1..C=%d, host array)", nids, C);
  if (!std::isfinite(thresh)) return set_err(GSR_ERR_INVALID, "gsr_group_classify: threshold is not finite");
  GroupSel sel;
  memset(&sel, 0, sizeof(sel));
  for (int32_t k = 0; k < nids; ++k) {
    const int32_t c = ids[k];
    if (c < 0 || c >= C) return set_err(GSR_ERR_INVALID, "gsr_group_classify: id %d outside [0, %d)", c, C);
    if ((sel.bits[c >> 5] >> (c & 31)) & 1u) return set_err(GSR_ERR_INVALID, "gsr_group_classify: duplicate id %d", c);
    sel.bits[c >> 5] |= 1u << (c & 31);
  }
  if (P == 0) return GSR_OK;
  if (!objects || !W || !b || !psel || !mask) return set_err(GSR_ERR_INVALID, "gsr_group_classify: null argument");
  if (((uintptr_t)objects & 15) != 0) return set_err(GSR_ERR_INVALID, "gsr_group_classify: objects must be 16-byte aligned");
  hipLaunchKernelGGL(k_group_classify, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     objects, P, W, b, C, sel, thresh, psel, mask);
  LAUNCH_CHECK("gsr_group_classify");
  return GSR_OK;
}

int gsr_convex_hull_planes(const double* pts, int64_t M, double* planes, int64_t max_facets, int64_t* nfacets, double* bbox) {
  if (!nfacets || !bbox) return set_err(GSR_ERR_INVALID, "gsr_convex_hull_planes: null nfacets / bbox");
  *nfacets = 0;
  for (int a = 0; a < 6; ++a) bbox[a] = 0.0;
  if (M < 0 || max_facets < 0) return set_err(GSR_ERR_INVALID, "gsr_convex_hull_planes: M=%lld max_facets=%lld", (long long)M,
                                              (long long)max_facets);
  if (M > 0 && !pts) return set_err(GSR_ERR_INVALID, "gsr_convex_hull_planes: null points");
  if (max_facets > 0 && !planes) return set_err(GSR_ERR_INVALID, "gsr_convex_hull_planes: null planes");
  gsr_hull::Result r;
  try {
    r = gsr_hull::convex_hull(pts, M);
  } catch (const std::bad_alloc&) {
    return set_err(GSR_ERR_NOMEM, "gsr_convex_hull_planes: host allocation failed (M=%lld)", (long long)M);
  }
  if (M > 0)
    for (int a = 0; a < 6; ++a) bbox[a] = r.bbox[a];
  switch (r.status) {
    case gsr_hull::HULL_DEGENERATE: set_err(GSR_OK, "gsr_convex_hull_planes: degenerate point set (M=%lld)", (long long)M); return GSR_OK;
    case gsr_hull::HULL_CHECK_FAILED:
      return set_err(GSR_ERR_HULL, "gsr_convex_hull_planes: self-check failed: a point lies %.3e beyond a plane, tau %.3e",
                     r.worst, r.tau);
    case gsr_hull::HULL_OK: break;
    default: return set_err(GSR_ERR_HULL, "gsr_convex_hull_planes: the construction lost its topology (M=%lld)", (long long)M);
  }
  *nfacets = (int64_t)r.planes.size();
  if (*nfacets > max_facets)
    return set_err(GSR_ERR_NOMEM, "gsr_convex_hull_planes: %lld facets, room for %lld", (long long)*nfacets, (long long)max_facets);
  for (size_t f = 0; f < r.planes.size(); ++f) {
    planes[4 * f] = r.planes[f].nx; planes[4 * f + 1] = r.planes[f].ny;
    planes[4 * f + 2] = r.planes[f].nz; planes[4 * f + 3] = r.planes[f].c;
  }
  return GSR_OK;
}

int gsr_points_in_hull(const float* xyz, int32_t P, const double* planes, int32_t F, const double* bbox, double tau,
                       const uint8_t* mask_in, uint8_t* out, void* stream) {
  if (P < 0 || F < 0) return set_err(GSR_ERR_INVALID, "gsr_points_in_hull: P=%d F=%d", P, F);
  if (!(tau >= 0.0) || !std::isfinite(tau)) return set_err(GSR_ERR_INVALID, "gsr_points_in_hull: tau must be finite and >= 0");
  if (P == 0) return GSR_OK;
  if (!xyz || !out || !bbox || (F > 0 && !planes)) return set_err(GSR_ERR_INVALID, "gsr_points_in_hull: null argument");
  if (F > 0 && ((uintptr_t)planes & 31) != 0) return set_err(GSR_ERR_INVALID, "gsr_points_in_hull: planes must be 32-byte aligned");
  hipLaunchKernelGGL(k_points_in_hull, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     xyz, P, reinterpret_cast<const double4*>(planes), F, bbox, tau, mask_in, out);
  LAUNCH_CHECK("gsr_points_in_hull");
  return GSR_OK;
}

// ---- image front end (gsr_image.h / gsr_image.hip.h): no allocation, no copy, no host wait; the spec and the
// per-channel affine travel by value in the kernel arguments, so the calls are capturable and never touch the pool ----
static int image_spec(const char* fn, const GsrResample* r, gsr_image::Spec& sp) {
  if (!r) return set_err(GSR_ERR_INVALID, "%s: null spec", fn);
  if (r->B < 1 || r->C < 1 || r->H < 1 || r->W < 1 || r->out_h < 1 || r->out_w < 1 || r->rh < 1 || r->rw < 1)
    return set_err(GSR_ERR_INVALID, "%s: sizes must be >= 1 (B=%d C=%d H=%d W=%d out=%dx%d resized=%dx%d)", fn, r->B, r->C, r->H,
                   r->W, r->out_h, r->out_w, r->rh, r->rw);
  if (r->C > gsr_image::MAX_C) return set_err(GSR_ERR_INVALID, "%s: C=%d channels (1..%d)", fn, r->C, gsr_image::MAX_C);
  if (r->top < 0 || r->left < 0) return set_err(GSR_ERR_INVALID, "%s: negative offset top=%d left=%d", fn, r->top, r->left);
  if ((long long)r->top + r->rh > r->out_h || (long long)r->left + r->rw > r->out_w)
    return set_err(GSR_ERR_INVALID, "%s: the resized image %dx%d at (top=%d, left=%d) does not fit the destination %dx%d", fn,
                   r->rh, r->rw, r->top, r->left, r->out_h, r->out_w);
  const unsigned long long lim = 0x7fffffffull, bc = (unsigned long long)r->B * (unsigned long long)r->C;
  const unsigned long long sp_px = (unsigned long long)r->H * (unsigned long long)r->W;
  const unsigned long long op_px = (unsigned long long)r->out_h * (unsigned long long)r->out_w;
  if (sp_px > lim || op_px > lim || bc * sp_px > lim || bc * op_px > lim)
    return set_err(GSR_ERR_INVALID, "%s: more than 2^31 - 1 elements in the source or the destination", fn);
  if (r->flags & ~GSR_RESAMPLE_CLAMP01) return set_err(GSR_ERR_INVALID, "%s: unknown flags 0x%x", fn, r->flags);
  sp.C = r->C; sp.H = r->H; sp.W = r->W; sp.out_h = r->out_h; sp.out_w = r->out_w;
  sp.rh = r->rh; sp.rw = r->rw; sp.top = r->top; sp.left = r->left;
  sp.pad_value = r->pad_value;
  sp.sy = gsr_image::axis_scale(r->H, r->rh);
  sp.sx = gsr_image::axis_scale(r->W, r->rw);
  sp.flags = r->flags;
  sp.affine = (r->mean || r->inv_std) ? 1 : 0;
  for (int c = 0; c < gsr_image::MAX_C; ++c) {
    sp.mean[c] = (r->mean && c < r->C) ? r->mean[c] : 0.0f;
    sp.inv_std[c] = (r->inv_std && c < r->C) ? r->inv_std[c] : 1.0f;
  }
  return GSR_OK;
}

int gsr_image_resample(const GsrResample* r, const float* src, float* dst, void* stream) {
  gsr_image::Spec sp;
  if (int rc = image_spec("gsr_image_resample", r, sp)) return rc;
  if (!src || !dst) return set_err(GSR_ERR_INVALID, "gsr_image_resample: null src / dst");
  const unsigned nbx = (unsigned)((sp.out_w + gsr_image::IMG_BX - 1) / gsr_image::IMG_BX);
  const unsigned nby = (unsigned)((sp.out_h + gsr_image::IMG_BY - 1) / gsr_image::IMG_BY);
  const unsigned long long blocks = (unsigned long long)nbx * nby * (unsigned long long)r->B;
  if (blocks > 0x7fffffffull) return set_err(GSR_ERR_INVALID, "gsr_image_resample: too many workgroups for one launch");
  hipLaunchKernelGGL(gsr_image::k_image_resample, dim3((unsigned)blocks), dim3(gsr_image::IMG_BX, gsr_image::IMG_BY), 0,
                     static_cast<hipStream_t>(stream), sp, src, dst, nbx, nby);
  LAUNCH_CHECK("gsr_image_resample");
  return GSR_OK;
}

int gsr_image_resample_backward(const GsrResample* r, const float* src, const float* grad_dst, float* grad_src,
                                int32_t accumulate, void* stream) {
  gsr_image::Spec sp;
  if (int rc = image_spec("gsr_image_resample_backward", r, sp)) return rc;
  if (!grad_dst || !grad_src) return set_err(GSR_ERR_INVALID, "gsr_image_resample_backward: null grad_dst / grad_src");
  if ((sp.flags & GSR_RESAMPLE_CLAMP01) && !src)
    return set_err(GSR_ERR_INVALID, "gsr_image_resample_backward: GSR_RESAMPLE_CLAMP01 needs src (the clamp's mask)");
  const unsigned nbx = (unsigned)((sp.W + gsr_image::IMG_BX * 4 - 1) / (gsr_image::IMG_BX * 4));
  const unsigned nby = (unsigned)((sp.H + gsr_image::IMG_BY - 1) / gsr_image::IMG_BY);
  const unsigned long long blocks = (unsigned long long)nbx * nby * (unsigned long long)r->B;
  if (blocks > 0x7fffffffull) return set_err(GSR_ERR_INVALID, "gsr_image_resample_backward: too many workgroups for one launch");
  const bool vec = (sp.W & 3) == 0 && ((uintptr_t)grad_src & 15) == 0 && (!(sp.flags & GSR_RESAMPLE_CLAMP01) || ((uintptr_t)src & 15) == 0);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)blocks), block(gsr_image::IMG_BX, gsr_image::IMG_BY);
  if (vec) hipLaunchKernelGGL((gsr_image::k_image_resample_bwd<true>), grid, block, 0, st, sp, src, grad_dst, grad_src, (int)accumulate, nbx, nby);
  else hipLaunchKernelGGL((gsr_image::k_image_resample_bwd<false>), grid, block, 0, st, sp, src, grad_dst, grad_src, (int)accumulate, nbx, nby);
  LAUNCH_CHECK("gsr_image_resample_backward");
  return GSR_OK;
}

int gsr_image_to_u8(const float* src, int32_t B, int32_t H, int32_t W, uint8_t* dst, void* stream) {
  if (B < 1 || H < 1 || W < 1) return set_err(GSR_ERR_INVALID, "gsr_image_to_u8: sizes must be >= 1 (B=%d H=%d W=%d)", B, H, W);
  const unsigned long long plane = (unsigned long long)H * (unsigned long long)W;
  if (plane > 0x7fffffffull || 3ull * (unsigned long long)B * plane > 0x7fffffffull)
    return set_err(GSR_ERR_INVALID, "gsr_image_to_u8: more than 2^31 - 1 elements");
  if (!src || !dst) return set_err(GSR_ERR_INVALID, "gsr_image_to_u8: null src / dst");
  const unsigned nbx = (unsigned)((plane + 1023) / 1024);
  const int aligned = (plane & 3) == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 3) == 0;
  hipLaunchKernelGGL(gsr_image::k_image_to_u8, dim3(nbx * (unsigned)B), dim3(256), 0, static_cast<hipStream_t>(stream), src,
                     (size_t)plane, dst, nbx, aligned);
  LAUNCH_CHECK("gsr_image_to_u8");
  return GSR_OK;
}

// ---- detector output stage (gsr_detect.h / gsr_detect.hip.h): no allocation, no copy, no host wait; everything is
// checked on the host before the first launch.  Workspace: [score B*A f32][class B*A i32][order B*maxc i32][ncand B i32],
// each region rounded up to 256 bytes.
static int det_spec(const char* fn, const GsrDetSpec* d, gsr_detect::Spec& sp) {
  if (!d) return set_err(GSR_ERR_INVALID, "%s: null spec", fn);
  if (d->B < 1 || d->A < 1 || d->C < 1) return set_err(GSR_ERR_INVALID, "%s: sizes must be >= 1 (B=%d A=%d C=%d)", fn, d->B, d->A, d->C);
  if ((d->layout != 0 && d->layout != 1) || (d->has_obj != 0 && d->has_obj != 1) || (d->box_format != 0 && d->box_format != 1))
    return set_err(GSR_ERR_INVALID, "%s: layout, has_obj and box_format are 0 or 1 (got %d, %d, %d)", fn, d->layout, d->has_obj, d->box_format);
  if (d->max_candidates < 1 || d->max_candidates > gsr_detect::MAX_CAND)
    return set_err(GSR_ERR_INVALID, "%s: max_candidates=%d (1..%d)", fn, d->max_candidates, gsr_detect::MAX_CAND);
  if (d->max_det < 1 || d->max_det > d->max_candidates)
    return set_err(GSR_ERR_INVALID, "%s: max_det=%d (1..max_candidates=%d)", fn, d->max_det, d->max_candidates);
  if (d->flags & ~GSR_DET_CLASS_AGNOSTIC) return set_err(GSR_ERR_INVALID, "%s: unknown flags 0x%x", fn, d->flags);
  const unsigned long long K = 4ull + (unsigned long long)d->has_obj + (unsigned long long)d->C;
  if ((unsigned long long)d->B * (unsigned long long)d->A > 0x7fffffffull ||
      (unsigned long long)d->B * (unsigned long long)d->A * K > 0x7fffffffull ||
      (unsigned long long)d->B * (unsigned long long)d->max_det * 6ull > 0x7fffffffull)
    return set_err(GSR_ERR_INVALID, "%s: more than 2^31 - 1 elements in pred or dets", fn);
  sp.B = d->B; sp.A = d->A; sp.C = d->C; sp.layout = d->layout; sp.has_obj = d->has_obj; sp.box_format = d->box_format;
  sp.conf_thr = d->conf_thr; sp.iou_thr = d->iou_thr; sp.max_candidates = d->max_candidates; sp.max_det = d->max_det;
  sp.flags = d->flags; sp.ox = d->ox; sp.oy = d->oy; sp.sx = d->sx; sp.sy = d->sy;
  return GSR_OK;
}

int gsr_det_workspace_bytes(const GsrDetSpec* d, int64_t* bytes) {
  gsr_detect::Spec sp;
  if (int rc = det_spec("gsr_det_workspace_bytes", d, sp)) return rc;
  if (!bytes) return set_err(GSR_ERR_INVALID, "gsr_det_workspace_bytes: null bytes");
  Carve c;
  det_regions(c, sp.B, sp.A, sp.max_candidates);
  *bytes = (int64_t)c.off;
  return GSR_OK;
}

int gsr_det_postprocess(const GsrDetSpec* d, const float* pred, void* ws, int64_t ws_bytes, float* dets, int32_t* counts,
                        void* stream) {
  gsr_detect::Spec sp;
  if (int rc = det_spec("gsr_det_postprocess", d, sp)) return rc;
  if (!pred || !ws || !dets || !counts) return set_err(GSR_ERR_INVALID, "gsr_det_postprocess: null pred / ws / dets / counts");
  Carve c(ws);
  const DetWs w = det_regions(c, sp.B, sp.A, sp.max_candidates);
  if (int rc = check_workspace("gsr_det_postprocess", ws, ws_bytes, c.off, 8, "gsr_det_workspace_bytes")) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const unsigned long long anchors = (unsigned long long)sp.B * (unsigned long long)sp.A;
  if (sp.layout == 1) {
    const unsigned blocks = (unsigned)((anchors + gsr_detect::SCORE_THREADS - 1) / gsr_detect::SCORE_THREADS);
    hipLaunchKernelGGL((gsr_detect::k_det_score<1>), dim3(blocks), dim3(gsr_detect::SCORE_THREADS), 0, st, sp, pred, w.score, w.cls);
  } else {
    const unsigned per = gsr_detect::SCORE_THREADS / 16;
    const unsigned blocks = (unsigned)((anchors + per - 1) / per);
    hipLaunchKernelGGL((gsr_detect::k_det_score<0>), dim3(blocks), dim3(gsr_detect::SCORE_THREADS), 0, st, sp, pred, w.score, w.cls);
  }
  LAUNCH_CHECK("gsr_det_postprocess (score)");
  hipLaunchKernelGGL(gsr_detect::k_det_select_sort, dim3((unsigned)sp.B), dim3(gsr_detect::SEL_THREADS), 0, st, sp.A,
                     sp.max_candidates, (const float*)w.score, 1, sp.conf_thr, (const int32_t*)nullptr, w.order, w.ncand, counts + 1, 2);
  LAUNCH_CHECK("gsr_det_postprocess (select)");
  gsr_detect::NmsArgs na;
  na.sp = sp; na.pred = pred; na.score = w.score; na.cls = w.cls; na.boxes = nullptr; na.order = w.order; na.ncand = w.ncand;
  na.dets = dets; na.keep = nullptr; na.counts = counts;
  hipLaunchKernelGGL((gsr_detect::k_det_nms<true>), dim3((unsigned)sp.B), dim3(gsr_detect::NMS_THREADS), 0, st, na);
  LAUNCH_CHECK("gsr_det_postprocess (nms)");
  return GSR_OK;
}

int gsr_det_nms(int32_t B, int32_t n, const float* boxes, const float* scores, const int32_t* classes, const int32_t* n_valid,
                float iou_thr, int32_t max_det, void* ws, int64_t ws_bytes, int32_t* keep, int32_t* counts, void* stream) {
  if (B < 1 || n < 1 || n > gsr_detect::MAX_CAND)
    return set_err(GSR_ERR_INVALID, "gsr_det_nms: B=%d (>= 1), n=%d (1..%d)", B, n, gsr_detect::MAX_CAND);
  if (max_det < 1 || max_det > n) return set_err(GSR_ERR_INVALID, "gsr_det_nms: max_det=%d (1..n=%d)", max_det, n);
  if ((unsigned long long)B * (unsigned long long)n * 4ull > 0x7fffffffull)
    return set_err(GSR_ERR_INVALID, "gsr_det_nms: more than 2^31 - 1 elements in boxes");
  if (!boxes || !scores || !ws || !keep || !counts) return set_err(GSR_ERR_INVALID, "gsr_det_nms: null boxes / scores / ws / keep / counts");
  Carve c(ws);
  const DetWs w = det_regions(c, B, n, n);
  if (int rc = check_workspace("gsr_det_nms", ws, ws_bytes, c.off, 8, "gsr_det_workspace_bytes with A = max_candidates = n")) return rc;
  return launch_nms_walk("gsr_det_nms", B, n, boxes, scores, classes, n_valid, iou_thr, max_det, w, keep, counts,
                         static_cast<hipStream_t>(stream));
}

int gsr_det_box_iou(const float* a, int32_t n, const float* b, int32_t m, float* iou, void* stream) {
  if (n < 1 || m < 1) return set_err(GSR_ERR_INVALID, "gsr_det_box_iou: sizes must be >= 1 (n=%d m=%d)", n, m);
  const unsigned long long total = (unsigned long long)n * (unsigned long long)m;
  if (total > 0x7fffffffull) return set_err(GSR_ERR_INVALID, "gsr_det_box_iou: more than 2^31 - 1 elements");
  if (!a || !b || !iou) return set_err(GSR_ERR_INVALID, "gsr_det_box_iou: null a / b / iou");
  hipLaunchKernelGGL(gsr_detect::k_det_box_iou, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                     a, n, b, m, iou);
  LAUNCH_CHECK("gsr_det_box_iou");
  return GSR_OK;
}

int gsr_det_verdict(const float* dets, const int32_t* counts, int32_t B, int32_t max_det, const float* gt, int32_t target,
                    int32_t untarget, int32_t is_targeted, float iou_match, int32_t* verdict, float* best, void* stream) {
  if (B < 1 || max_det < 1) return set_err(GSR_ERR_INVALID, "gsr_det_verdict: sizes must be >= 1 (B=%d max_det=%d)", B, max_det);
  if ((unsigned long long)B * (unsigned long long)max_det * 6ull > 0x7fffffffull)
    return set_err(GSR_ERR_INVALID, "gsr_det_verdict: more than 2^31 - 1 elements in dets");
  if (!dets || !counts || !verdict || !best) return set_err(GSR_ERR_INVALID, "gsr_det_verdict: null dets / counts / verdict / best");
  hipLaunchKernelGGL(gsr_detect::k_det_verdict, dim3((unsigned)B), dim3(64), 0, static_cast<hipStream_t>(stream), dets, counts,
                     max_det, gt, target, untarget < 0 ? -1 : untarget, is_targeted != 0 ? 1 : 0, iou_match, verdict, best);
  LAUNCH_CHECK("gsr_det_verdict");
  return GSR_OK;
}

// ---- detector loss stage (gsr_detloss.h / gsr_detloss.hip.h): four launches, no allocation, no copy, no host wait;
// everything is checked on the host before the first launch.  Workspace: [ov B*M*A f32][metric B*M*A f32][tgt B*A i32]
// [ts B*A f32][ts_sum B f32][slab blocks*3 f32], each region rounded up to 256 bytes; the slab is sized for one anchor
// per lane (the most blocks either path launches).
static unsigned detloss_tiles(long long A, int v) {
  const long long per = (long long)gsr_dloss::TERM_THREADS * v;
  return (unsigned)((A + per - 1) / per);
}

static unsigned detloss_chunks(int C) { return 1u + (unsigned)((C + gsr_dloss::CLS_CHUNK - 1) / gsr_dloss::CLS_CHUNK); }

static void detloss_regions(Carve& c, gsr_dloss::Args& ar) {
  const gsr_dloss::Spec& sp = ar.sp;
  const size_t BA = (size_t)sp.B * (size_t)sp.A, BMA = BA * (size_t)sp.M;
  const size_t blocks = (size_t)detloss_tiles(sp.A, 1) * (size_t)detloss_chunks(sp.C) * (size_t)sp.B;
  ar.ov = c.take<float>(BMA);
  ar.metric = c.take<float>(BMA);
  ar.tgt = c.take<int32_t>(BA);
  ar.ts = c.take<float>(BA);
  ar.ts_sum = c.take<float>((size_t)sp.B);
  ar.slab = c.take<float>(blocks * 3);
}

static int detloss_spec(const char* fn, const GsrDetLossSpec* d, gsr_dloss::Spec& sp) {
  if (!d) return set_err(GSR_ERR_INVALID, "%s: null spec", fn);
  if (d->B < 1 || d->A < 1 || d->C < 1) return set_err(GSR_ERR_INVALID, "%s: sizes must be >= 1 (B=%d A=%d C=%d)", fn, d->B, d->A, d->C);
  if (d->M < 1 || d->M > gsr_dloss::MAX_ROWS) return set_err(GSR_ERR_INVALID, "%s: M=%d gt rows per image (1..%d)", fn, d->M, gsr_dloss::MAX_ROWS);
  if (d->nl < 1 || d->nl > gsr_dloss::MAX_LEVELS) return set_err(GSR_ERR_INVALID, "%s: nl=%d levels (1..%d)", fn, d->nl, gsr_dloss::MAX_LEVELS);
  if (d->reg_max != gsr_dloss::REG_MAX) return set_err(GSR_ERR_INVALID, "%s: reg_max=%d (only %d is built)", fn, d->reg_max, gsr_dloss::REG_MAX);
  if (d->topk < 1 || d->topk > gsr_dloss::MAX_TOPK) return set_err(GSR_ERR_INVALID, "%s: topk=%d (1..%d)", fn, d->topk, gsr_dloss::MAX_TOPK);
  if (d->flags != 0u) return set_err(GSR_ERR_INVALID, "%s: unknown flags 0x%x", fn, d->flags);
  if (!all_finite_nonneg({d->alpha, d->beta, d->w_box, d->w_cls, d->w_dfl}))
    return set_err(GSR_ERR_INVALID, "%s: alpha, beta, w_box, w_cls, w_dfl must be finite and >= 0", fn);
  unsigned long long total = 0;
  for (int i = 0; i < d->nl; ++i) {
    if (d->level_h[i] < 1 || d->level_w[i] < 1 || !finite_pos(d->level_stride[i]))
      return set_err(GSR_ERR_INVALID, "%s: level %d is %d x %d with stride %g (sizes >= 1, a finite stride > 0)", fn, i,
                     d->level_h[i], d->level_w[i], (double)d->level_stride[i]);
    sp.h[i] = d->level_h[i]; sp.w[i] = d->level_w[i]; sp.stride[i] = d->level_stride[i];
    sp.start[i] = (int32_t)(total > 0x7fffffffull ? 0x7fffffffull : total);
    total += (unsigned long long)d->level_h[i] * (unsigned long long)d->level_w[i];
    if (total > 0x7fffffffull) return set_err(GSR_ERR_INVALID, "%s: the levels hold more than 2^31 - 1 anchors", fn);
  }
  for (int i = d->nl; i < gsr_dloss::MAX_LEVELS; ++i) { sp.h[i] = 1; sp.w[i] = 1; sp.stride[i] = 1.0f; sp.start[i] = 0x7fffffff; }
  if (total != (unsigned long long)d->A)
    return set_err(GSR_ERR_INVALID, "%s: the levels hold %llu anchors, A=%d", fn, total, d->A);
  const unsigned long long K = 64ull + (unsigned long long)d->C;
  if ((unsigned long long)d->B * (unsigned long long)d->A * K > 0x7fffffffull ||
      (unsigned long long)d->B * (unsigned long long)d->A * (unsigned long long)d->M > 0x7fffffffull)
    return set_err(GSR_ERR_INVALID, "%s: more than 2^31 - 1 elements in pred or in the workspace's [B,M,A] arrays", fn);
  if (d->B > 65535 || detloss_chunks(d->C) > 65535u)
    return set_err(GSR_ERR_INVALID, "%s: B=%d (<= 65535), C=%d (<= %d)", fn, d->B, d->C, 65534 * gsr_dloss::CLS_CHUNK);
  sp.B = d->B; sp.A = d->A; sp.C = d->C; sp.M = d->M; sp.nl = d->nl; sp.topk = d->topk;
  sp.alpha = d->alpha; sp.beta = d->beta; sp.w_box = d->w_box; sp.w_cls = d->w_cls; sp.w_dfl = d->w_dfl;
  return GSR_OK;
}

int gsr_detloss_workspace_bytes(const GsrDetLossSpec* d, int64_t* bytes) {
  gsr_dloss::Args ar;
  if (int rc = detloss_spec("gsr_detloss_workspace_bytes", d, ar.sp)) return rc;
  if (!bytes) return set_err(GSR_ERR_INVALID, "gsr_detloss_workspace_bytes: null bytes");
  Carve c;
  detloss_regions(c, ar);
  *bytes = (int64_t)c.off;
  return GSR_OK;
}

int gsr_detloss(const GsrDetLossSpec* d, const float* pred, const float* gt_boxes, const int32_t* gt_cls, void* ws,
                int64_t ws_bytes, float* loss, float* grad_pred, int32_t* tgt, float* ts, void* stream) {
  gsr_dloss::Args ar;
  if (int rc = detloss_spec("gsr_detloss", d, ar.sp)) return rc;
  const gsr_dloss::Spec& sp = ar.sp;
  if (!pred || !gt_boxes || !gt_cls || !ws || !loss)
    return set_err(GSR_ERR_INVALID, "gsr_detloss: null pred / gt_boxes / gt_cls / ws / loss");
  Carve c(ws);
  detloss_regions(c, ar);
  if (int rc = check_workspace("gsr_detloss", ws, ws_bytes, c.off, 16, "gsr_detloss_workspace_bytes")) return rc;
  if (int rc = check_aligned4("gsr_detloss", pred, gt_boxes, gt_cls, loss, grad_pred, tgt, ts)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ar.pred = pred; ar.gt_boxes = gt_boxes; ar.gt_cls = gt_cls;
  ar.loss = loss; ar.grad_pred = grad_pred; ar.tgt_out = tgt; ar.ts_out = ts;
  const unsigned long long anchors = (unsigned long long)sp.B * (unsigned long long)sp.A;
  hipLaunchKernelGGL(gsr_dloss::k_detloss_metrics, dim3((unsigned)((anchors + gsr_dloss::MET_THREADS - 1) / gsr_dloss::MET_THREADS)),
                     dim3(gsr_dloss::MET_THREADS), 0, st, ar);
  LAUNCH_CHECK("gsr_detloss (metrics)");
  hipLaunchKernelGGL(gsr_dloss::k_detloss_assign, dim3((unsigned)sp.B), dim3(gsr_dloss::ASG_THREADS), 0, st, ar);
  LAUNCH_CHECK("gsr_detloss (assign)");
  const bool vec = (sp.A & 3) == 0 && ((uintptr_t)pred & 15) == 0 && ((uintptr_t)grad_pred & 15) == 0;
  const unsigned tiles = detloss_tiles(sp.A, vec ? 4 : 1), chunks = detloss_chunks(sp.C);
  const dim3 grid(tiles, chunks, (unsigned)sp.B);
  if (vec)
    hipLaunchKernelGGL((gsr_dloss::k_detloss_terms<4>), grid, dim3(gsr_dloss::TERM_THREADS), 0, st, ar);
  else
    hipLaunchKernelGGL((gsr_dloss::k_detloss_terms<1>), grid, dim3(gsr_dloss::TERM_THREADS), 0, st, ar);
  LAUNCH_CHECK("gsr_detloss (terms)");
  hipLaunchKernelGGL(gsr_dloss::k_detloss_final, dim3(1), dim3(gsr_dloss::FIN_THREADS), 0, st, ar, tiles * chunks * (unsigned)sp.B);
  LAUNCH_CHECK("gsr_detloss (final)");
  return GSR_OK;
}

// ---- set-prediction detector stage (gsr_setdet.h / gsr_setdet.hip.h): four launches for the loss, one for the output
// stage; no allocation, no copy, no host wait; everything is checked on the host before the first launch.  Workspace:
// [stats B*Q*2 f32][cost B*M*Q f32][tgt B*Q i32][nmatch B i32][slab blocks*3 f32], each region rounded up to 256 bytes.
static unsigned setdet_term_blocks(const gsr_setdet::Spec& sp) {
  const unsigned long long total = (unsigned long long)sp.B * (unsigned long long)sp.Q * (unsigned long long)(sp.C + 1);
  return (unsigned)((total + gsr_setdet::TERM_TILE - 1) / gsr_setdet::TERM_TILE);
}

static void setdet_regions(Carve& c, gsr_setdet::Args& ar) {
  const gsr_setdet::Spec& sp = ar.sp;
  const size_t BQ = (size_t)sp.B * (size_t)sp.Q;
  ar.stats = c.take<float>(BQ * 2);
  ar.cost = c.take<float>(BQ * (size_t)sp.M);
  ar.tgt = c.take<int32_t>(BQ);
  ar.nmatch = c.take<int32_t>((size_t)sp.B);
  ar.slab = c.take<float>((size_t)setdet_term_blocks(sp) * 3);
}

static int setdet_spec(const char* fn, const GsrSetDetSpec* d, gsr_setdet::Spec& sp) {
  if (!d) return set_err(GSR_ERR_INVALID, "%s: null spec", fn);
  if (d->B < 1 || d->B > 65535) return set_err(GSR_ERR_INVALID, "%s: B=%d images (1..65535)", fn, d->B);
  if (d->Q < 1 || d->Q > gsr_setdet::MAX_QUERIES) return set_err(GSR_ERR_INVALID, "%s: Q=%d queries (1..%d)", fn, d->Q, gsr_setdet::MAX_QUERIES);
  if (d->C < 1 || d->C > gsr_setdet::MAX_CLASSES) return set_err(GSR_ERR_INVALID, "%s: C=%d classes (1..%d)", fn, d->C, gsr_setdet::MAX_CLASSES);
  if (d->M < 1 || d->M > gsr_setdet::MAX_ROWS) return set_err(GSR_ERR_INVALID, "%s: M=%d gt rows per image (1..%d)", fn, d->M, gsr_setdet::MAX_ROWS);
  if (d->Q < d->M) return set_err(GSR_ERR_INVALID, "%s: Q=%d queries cannot take M=%d rows (Q >= M)", fn, d->Q, d->M);
  if (d->max_det < 1 || d->max_det > gsr_setdet::MAX_QUERIES)
    return set_err(GSR_ERR_INVALID, "%s: max_det=%d (1..%d)", fn, d->max_det, gsr_setdet::MAX_QUERIES);
  if (d->flags != 0u) return set_err(GSR_ERR_INVALID, "%s: unknown flags 0x%x", fn, d->flags);
  if (!all_finite_nonneg({d->c_class, d->c_l1, d->c_giou, d->w_ce, d->w_l1, d->w_giou, d->eos_coef}))
    return set_err(GSR_ERR_INVALID, "%s: c_class, c_l1, c_giou, w_ce, w_l1, w_giou, eos_coef must be finite and >= 0", fn);
  if (!finite_pos(d->img_w) || !finite_pos(d->img_h))
    return set_err(GSR_ERR_INVALID, "%s: the frame is %g x %g (finite sizes > 0)", fn, (double)d->img_w, (double)d->img_h);
  if ((unsigned long long)d->B * (unsigned long long)d->Q * (unsigned long long)(d->C + 1) > 0x7fffffffull)
    return set_err(GSR_ERR_INVALID, "%s: more than 2^31 - 1 elements in logits", fn);
  sp.B = d->B; sp.Q = d->Q; sp.C = d->C; sp.M = d->M; sp.img_w = d->img_w; sp.img_h = d->img_h;
  sp.c_class = d->c_class; sp.c_l1 = d->c_l1; sp.c_giou = d->c_giou; sp.w_ce = d->w_ce; sp.w_l1 = d->w_l1; sp.w_giou = d->w_giou;
  sp.eos_coef = d->eos_coef; sp.conf_thr = d->conf_thr; sp.max_det = d->max_det;
  return GSR_OK;
}

int gsr_setdet_workspace_bytes(const GsrSetDetSpec* d, int64_t* bytes) {
  gsr_setdet::Args ar;
  if (int rc = setdet_spec("gsr_setdet_workspace_bytes", d, ar.sp)) return rc;
  if (!bytes) return set_err(GSR_ERR_INVALID, "gsr_setdet_workspace_bytes: null bytes");
  Carve c;
  setdet_regions(c, ar);
  *bytes = (int64_t)c.off;
  return GSR_OK;
}

int gsr_setdet_loss(const GsrSetDetSpec* d, const float* logits, const float* boxes, const float* gt_boxes, const int32_t* gt_cls,
                    void* ws, int64_t ws_bytes, float* loss, float* grad_logits, float* grad_boxes, int32_t* match, int32_t* tgt,
                    void* stream) {
  gsr_setdet::Args ar;
  if (int rc = setdet_spec("gsr_setdet_loss", d, ar.sp)) return rc;
  const gsr_setdet::Spec& sp = ar.sp;
  if (!logits || !boxes || !gt_boxes || !gt_cls || !ws || !loss)
    return set_err(GSR_ERR_INVALID, "gsr_setdet_loss: null logits / boxes / gt_boxes / gt_cls / ws / loss");
  Carve c(ws);
  setdet_regions(c, ar);
  if (int rc = check_workspace("gsr_setdet_loss", ws, ws_bytes, c.off, 16, "gsr_setdet_workspace_bytes")) return rc;
  if (int rc = check_aligned4("gsr_setdet_loss", logits, boxes, gt_boxes, gt_cls, loss, grad_logits, grad_boxes, match, tgt)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ar.logits = logits; ar.boxes = boxes; ar.gt_boxes = gt_boxes; ar.gt_cls = gt_cls;
  ar.loss = loss; ar.grad_logits = grad_logits; ar.grad_boxes = grad_boxes; ar.match_out = match; ar.tgt_out = tgt;
  const unsigned long long queries = (unsigned long long)sp.B * (unsigned long long)sp.Q;
  hipLaunchKernelGGL(gsr_setdet::k_setdet_cost, dim3((unsigned)((queries + gsr_setdet::COST_WAVES - 1) / gsr_setdet::COST_WAVES)),
                     dim3(gsr_setdet::COST_THREADS), 0, st, ar);
  LAUNCH_CHECK("gsr_setdet_loss (cost)");
  hipLaunchKernelGGL(gsr_setdet::k_setdet_match, dim3((unsigned)sp.B), dim3(gsr_setdet::MATCH_THREADS), 0, st, ar);
  LAUNCH_CHECK("gsr_setdet_loss (match)");
  const unsigned blocks = setdet_term_blocks(sp);
  hipLaunchKernelGGL(gsr_setdet::k_setdet_terms, dim3(blocks), dim3(gsr_setdet::TERM_THREADS), 0, st, ar);
  LAUNCH_CHECK("gsr_setdet_loss (terms)");
  hipLaunchKernelGGL(gsr_setdet::k_setdet_final, dim3(1), dim3(gsr_setdet::FIN_THREADS), 0, st, ar, blocks);
  LAUNCH_CHECK("gsr_setdet_loss (final)");
  return GSR_OK;
}

int gsr_setdet_postprocess(const GsrSetDetSpec* d, const float* logits, const float* boxes, float* dets, int32_t* counts,
                           void* stream) {
  gsr_setdet::Spec sp;
  if (int rc = setdet_spec("gsr_setdet_postprocess", d, sp)) return rc;
  if (!logits || !boxes || !dets || !counts) return set_err(GSR_ERR_INVALID, "gsr_setdet_postprocess: null logits / boxes / dets / counts");
  if (int rc = check_aligned4("gsr_setdet_postprocess", logits, boxes, dets, counts)) return rc;
  hipLaunchKernelGGL(gsr_setdet::k_setdet_post, dim3((unsigned)sp.B), dim3((unsigned)((sp.Q + 63) / 64 * 64)), 0, static_cast<hipStream_t>(stream),
                     sp, logits, boxes, dets, counts);
  LAUNCH_CHECK("gsr_setdet_postprocess");
  return GSR_OK;
}

// ---- two-stage detector stage (gsr_rcnn.h / gsr_rcnn.hip.h): no allocation, no copy, no host wait; every entry checks the
// members of the spec it uses on the host before the first launch.  Workspace, each region rounded up to 256 bytes:
// [nrows 1 i32][slab blocks*2 f32] for the loss; [boxes B*R*4 f32][score B*R f32][cls B*R i32][ncand B i32]
// [keep B*max_det i32][nkept B i32][the NMS walk's own workspace] for the output stage; the two share the start.
static unsigned rcnn_row_blocks(long long B, long long S) {
  return (unsigned)((B * S + gsr_rcnn::ROW_WAVES - 1) / gsr_rcnn::ROW_WAVES);
}

static void rcnn_loss_regions(Carve& c, const GsrRcnnSpec* d, gsr_rcnn::LossArgs& ar) {
  ar.nrows = c.take<int32_t>(1);
  ar.slab = c.take<float>((size_t)rcnn_row_blocks(d->B, d->S) * 2);
}

// keep / nkept: what the NMS walk writes and k_rcnn_gather reads; nms: the walk's own workspace
static void rcnn_post_regions(Carve& c, const GsrRcnnSpec* d, gsr_rcnn::PostArgs& ar, int32_t*& keep, int32_t*& nkept, DetWs& nms) {
  const size_t BR = (size_t)d->B * (size_t)d->R;
  ar.boxes = c.take<float>(BR * 4);
  ar.score = c.take<float>(BR);
  ar.cls = c.take<int32_t>(BR);
  ar.ncand = c.take<int32_t>((size_t)d->B);
  ar.keep = keep = c.take<int32_t>((size_t)d->B * (size_t)d->max_det);
  ar.nkept = nkept = c.take<int32_t>((size_t)d->B);
  nms = det_regions(c, d->B, d->R, d->R);
}

static void rcnn_copy_spec(const GsrRcnnSpec* d, gsr_rcnn::Spec& sp) {
  sp.B = d->B; sp.R = d->R; sp.M = d->M; sp.S = d->S; sp.C = d->C; sp.max_pos = d->max_pos; sp.append_gt = d->append_gt != 0 ? 1 : 0;
  sp.seed = d->seed; sp.fg_iou = d->fg_iou; sp.Cf = d->Cf; sp.Hf = d->Hf; sp.Wf = d->Wf; sp.PH = d->PH; sp.PW = d->PW;
  sp.spatial_scale = d->spatial_scale; sp.sampling_ratio = d->sampling_ratio; sp.bw_x = d->bw_x; sp.bw_y = d->bw_y;
  sp.bw_w = d->bw_w; sp.bw_h = d->bw_h; sp.beta = d->beta; sp.w_cls = d->w_cls; sp.w_box = d->w_box; sp.conf_thr = d->conf_thr;
  sp.iou_thr = d->iou_thr; sp.max_det = d->max_det; sp.img_w = d->img_w; sp.img_h = d->img_h; sp.flags = d->flags;
}

static int rcnn_common(const char* fn, const GsrRcnnSpec* d) {
  if (!d) return set_err(GSR_ERR_INVALID, "%s: null spec", fn);
  if (d->B < 1 || d->B > 65535) return set_err(GSR_ERR_INVALID, "%s: B=%d images (1..65535)", fn, d->B);
  if (d->flags & ~GSR_RCNN_CLASS_AGNOSTIC) return set_err(GSR_ERR_INVALID, "%s: unknown flags 0x%x", fn, d->flags);
  return GSR_OK;
}

static int rcnn_sample_spec(const char* fn, const GsrRcnnSpec* d) {
  if (int rc = rcnn_common(fn, d)) return rc;
  if (d->M < 1 || d->M > gsr_rcnn::MAX_ROWS) return set_err(GSR_ERR_INVALID, "%s: M=%d gt rows per image (1..%d)", fn, d->M, gsr_rcnn::MAX_ROWS);
  if (d->S < 1 || d->S > gsr_rcnn::MAX_SAMPLE) return set_err(GSR_ERR_INVALID, "%s: S=%d RoIs per image (1..%d)", fn, d->S, gsr_rcnn::MAX_SAMPLE);
  if (d->C < 1 || d->C > gsr_rcnn::MAX_CLASSES) return set_err(GSR_ERR_INVALID, "%s: C=%d classes (1..%d)", fn, d->C, gsr_rcnn::MAX_CLASSES);
  if (d->R < 1 || (long long)d->R + (long long)d->M > gsr_rcnn::MAX_CAND)
    return set_err(GSR_ERR_INVALID, "%s: R=%d proposals with M=%d rows (R >= 1, R + M <= %d)", fn, d->R, d->M, gsr_rcnn::MAX_CAND);
  if (d->max_pos < 0 || d->max_pos > d->S) return set_err(GSR_ERR_INVALID, "%s: max_pos=%d (0..S=%d)", fn, d->max_pos, d->S);
  if (!finite_nonneg(d->fg_iou)) return set_err(GSR_ERR_INVALID, "%s: fg_iou must be finite and >= 0", fn);
  return GSR_OK;
}

static int rcnn_roi_spec(const char* fn, const GsrRcnnSpec* d, unsigned long long& pooled_elems) {
  if (int rc = rcnn_common(fn, d)) return rc;
  if (d->S < 1 || d->S > gsr_rcnn::MAX_SAMPLE) return set_err(GSR_ERR_INVALID, "%s: S=%d RoIs per image (1..%d)", fn, d->S, gsr_rcnn::MAX_SAMPLE);
  if (d->Cf < 1 || d->Hf < 1 || d->Wf < 1) return set_err(GSR_ERR_INVALID, "%s: the feature map is %d x %d x %d (sizes >= 1)", fn, d->Cf, d->Hf, d->Wf);
  if (d->Cf > 65535) return set_err(GSR_ERR_INVALID, "%s: Cf=%d channels (1..65535)", fn, d->Cf);
  if (d->PH < 1 || d->PH > gsr_rcnn::MAX_POOL || d->PW < 1 || d->PW > gsr_rcnn::MAX_POOL)
    return set_err(GSR_ERR_INVALID, "%s: the pooled size is %d x %d (1..%d each)", fn, d->PH, d->PW, gsr_rcnn::MAX_POOL);
  if (d->sampling_ratio < 0) return set_err(GSR_ERR_INVALID, "%s: sampling_ratio=%d (>= 0)", fn, d->sampling_ratio);
  if (!finite_pos(d->spatial_scale)) return set_err(GSR_ERR_INVALID, "%s: spatial_scale must be finite and > 0", fn);
  const unsigned long long feat = (unsigned long long)d->B * (unsigned long long)d->Cf * (unsigned long long)d->Hf * (unsigned long long)d->Wf;
  pooled_elems = (unsigned long long)d->B * (unsigned long long)d->S * (unsigned long long)d->Cf * (unsigned long long)(d->PH * d->PW);
  if ((unsigned long long)d->Hf * (unsigned long long)d->Wf > 0x7fffffffull || feat > 0x7fffffffull || pooled_elems > 0x7fffffffull)
    return set_err(GSR_ERR_INVALID, "%s: more than 2^31 - 1 elements in features or pooled", fn);
  return GSR_OK;
}

static int rcnn_head_spec(const char* fn, const GsrRcnnSpec* d, long long rows_per_image) {
  if (int rc = rcnn_common(fn, d)) return rc;
  if (d->C < 1 || d->C > gsr_rcnn::MAX_CLASSES) return set_err(GSR_ERR_INVALID, "%s: C=%d classes (1..%d)", fn, d->C, gsr_rcnn::MAX_CLASSES);
  if (!finite_pos(d->bw_x) || !finite_pos(d->bw_y) || !finite_pos(d->bw_w) || !finite_pos(d->bw_h))
    return set_err(GSR_ERR_INVALID, "%s: bw_x, bw_y, bw_w, bw_h must be finite and > 0", fn);
  if ((unsigned long long)d->B * (unsigned long long)rows_per_image * 4ull * (unsigned long long)d->C > 0x7fffffffull)
    return set_err(GSR_ERR_INVALID, "%s: more than 2^31 - 1 elements in scores or deltas", fn);
  return GSR_OK;
}

static int rcnn_loss_spec(const char* fn, const GsrRcnnSpec* d) {
  if (int rc = rcnn_common(fn, d)) return rc;
  if (d->S < 1 || d->S > gsr_rcnn::MAX_SAMPLE) return set_err(GSR_ERR_INVALID, "%s: S=%d RoIs per image (1..%d)", fn, d->S, gsr_rcnn::MAX_SAMPLE);
  if (d->M < 1 || d->M > gsr_rcnn::MAX_ROWS) return set_err(GSR_ERR_INVALID, "%s: M=%d gt rows per image (1..%d)", fn, d->M, gsr_rcnn::MAX_ROWS);
  if (int rc = rcnn_head_spec(fn, d, d->S)) return rc;
  if (!finite_nonneg(d->beta) || !finite_nonneg(d->w_cls) || !finite_nonneg(d->w_box))
    return set_err(GSR_ERR_INVALID, "%s: beta, w_cls, w_box must be finite and >= 0", fn);
  return GSR_OK;
}

static int rcnn_post_spec(const char* fn, const GsrRcnnSpec* d) {
  if (int rc = rcnn_common(fn, d)) return rc;
  if (d->R < 1 || d->R > gsr_rcnn::MAX_CAND) return set_err(GSR_ERR_INVALID, "%s: R=%d proposals per image (1..%d)", fn, d->R, gsr_rcnn::MAX_CAND);
  if (int rc = rcnn_head_spec(fn, d, d->R)) return rc;
  if (d->max_det < 1 || d->max_det > d->R) return set_err(GSR_ERR_INVALID, "%s: max_det=%d (1..R=%d)", fn, d->max_det, d->R);
  if (!finite_nonneg(d->conf_thr) || !finite_nonneg(d->iou_thr))
    return set_err(GSR_ERR_INVALID, "%s: conf_thr, iou_thr must be finite and >= 0", fn);
  if (!finite_pos(d->img_w) || !finite_pos(d->img_h))
    return set_err(GSR_ERR_INVALID, "%s: the frame is %g x %g (finite sizes > 0)", fn, (double)d->img_w, (double)d->img_h);
  return GSR_OK;
}

int gsr_rcnn_sample(const GsrRcnnSpec* d, const float* proposals, const int32_t* n_prop, const float* gt_boxes, const int32_t* gt_cls,
                    int32_t* idx, float* rois, int32_t* labels, int32_t* gt_row, int32_t* counts, void* stream) {
  if (int rc = rcnn_sample_spec("gsr_rcnn_sample", d)) return rc;
  if (!proposals || !gt_boxes || !gt_cls || !idx || !rois || !labels || !gt_row || !counts)
    return set_err(GSR_ERR_INVALID, "gsr_rcnn_sample: null proposals / gt_boxes / gt_cls / idx / rois / labels / gt_row / counts");
  if (int rc = check_aligned4("gsr_rcnn_sample", proposals, n_prop, gt_boxes, gt_cls, idx, rois, labels, gt_row, counts)) return rc;
  gsr_rcnn::SampleArgs ar;
  rcnn_copy_spec(d, ar.sp);
  ar.proposals = proposals; ar.n_prop = n_prop; ar.gt_boxes = gt_boxes; ar.gt_cls = gt_cls;
  ar.idx = idx; ar.rois = rois; ar.labels = labels; ar.gt_row = gt_row; ar.counts = counts;
  hipLaunchKernelGGL(gsr_rcnn::k_rcnn_sample, dim3((unsigned)d->B), dim3(gsr_rcnn::SAMP_THREADS), 0, static_cast<hipStream_t>(stream), ar);
  LAUNCH_CHECK("gsr_rcnn_sample");
  return GSR_OK;
}

int gsr_roi_align(const GsrRcnnSpec* d, const float* features, const float* rois, const int32_t* n_roi, int32_t n_roi_stride,
                  float* pooled, void* stream) {
  unsigned long long total = 0;
  if (int rc = rcnn_roi_spec("gsr_roi_align", d, total)) return rc;
  if (!features || !rois || !pooled) return set_err(GSR_ERR_INVALID, "gsr_roi_align: null features / rois / pooled");
  if (n_roi && n_roi_stride < 1) return set_err(GSR_ERR_INVALID, "gsr_roi_align: n_roi_stride=%d (>= 1)", n_roi_stride);
  if (int rc = check_aligned4("gsr_roi_align", features, rois, n_roi, pooled)) return rc;
  gsr_rcnn::RoiArgs ar{};
  rcnn_copy_spec(d, ar.sp);
  ar.features = features; ar.rois = rois; ar.n_roi = n_roi; ar.n_roi_stride = n_roi ? n_roi_stride : 0; ar.pooled = pooled;
  const unsigned long long per_roi = (unsigned long long)d->Cf * (unsigned long long)(d->PH * d->PW);
  hipLaunchKernelGGL(gsr_rcnn::k_roi_align, dim3((unsigned)(d->B * d->S), (unsigned)((per_roi + gsr_rcnn::RA_THREADS - 1) / gsr_rcnn::RA_THREADS)),
                     dim3(gsr_rcnn::RA_THREADS), 0, static_cast<hipStream_t>(stream), ar);
  LAUNCH_CHECK("gsr_roi_align");
  return GSR_OK;
}

int gsr_roi_align_backward(const GsrRcnnSpec* d, const float* rois, const int32_t* n_roi, int32_t n_roi_stride, const float* grad_pooled,
                           float* grad_features, int32_t accumulate, void* stream) {
  unsigned long long total = 0;
  if (int rc = rcnn_roi_spec("gsr_roi_align_backward", d, total)) return rc;
  if (!rois || !grad_pooled || !grad_features) return set_err(GSR_ERR_INVALID, "gsr_roi_align_backward: null rois / grad_pooled / grad_features");
  if (n_roi && n_roi_stride < 1) return set_err(GSR_ERR_INVALID, "gsr_roi_align_backward: n_roi_stride=%d (>= 1)", n_roi_stride);
  if (int rc = check_aligned4("gsr_roi_align_backward", rois, n_roi, grad_pooled, grad_features)) return rc;
  const unsigned long long tiles = (unsigned long long)((d->Hf + gsr_rcnn::RB_TILE - 1) / gsr_rcnn::RB_TILE) *
                                   (unsigned long long)((d->Wf + gsr_rcnn::RB_TILE - 1) / gsr_rcnn::RB_TILE);
  if (tiles > 0x7fffffffull) return set_err(GSR_ERR_INVALID, "gsr_roi_align_backward: more than 2^31 - 1 tiles");
  gsr_rcnn::RoiArgs ar{};
  rcnn_copy_spec(d, ar.sp);
  ar.rois = rois; ar.n_roi = n_roi; ar.n_roi_stride = n_roi ? n_roi_stride : 0; ar.grad_pooled = grad_pooled;
  ar.grad_features = grad_features; ar.accumulate = accumulate != 0 ? 1 : 0;
  hipLaunchKernelGGL(gsr_rcnn::k_roi_align_bwd,
                     dim3((unsigned)tiles, (unsigned)((d->Cf + gsr_rcnn::RB_CHUNK - 1) / gsr_rcnn::RB_CHUNK), (unsigned)d->B),
                     dim3(gsr_rcnn::RB_THREADS), 0, static_cast<hipStream_t>(stream), ar);
  LAUNCH_CHECK("gsr_roi_align_backward");
  return GSR_OK;
}

int gsr_rcnn_workspace_bytes(const GsrRcnnSpec* d, int64_t* bytes) {
  if (int rc = rcnn_common("gsr_rcnn_workspace_bytes", d)) return rc;
  if (!bytes) return set_err(GSR_ERR_INVALID, "gsr_rcnn_workspace_bytes: null bytes");
  const bool loss = d->S >= 1 && d->S <= gsr_rcnn::MAX_SAMPLE;
  const bool post = d->R >= 1 && d->R <= gsr_rcnn::MAX_CAND && d->max_det >= 1 && d->max_det <= d->R;
  if (!loss && !post)
    return set_err(GSR_ERR_INVALID, "gsr_rcnn_workspace_bytes: neither S=%d (1..%d) nor R=%d (1..%d) with max_det=%d (1..R) is in range",
                   d->S, gsr_rcnn::MAX_SAMPLE, d->R, gsr_rcnn::MAX_CAND, d->max_det);
  Carve cl, cp;                                  // the two share the start
  gsr_rcnn::LossArgs la;
  gsr_rcnn::PostArgs pa;
  int32_t *keep, *nkept;
  DetWs nms;
  if (loss) rcnn_loss_regions(cl, d, la);
  if (post) rcnn_post_regions(cp, d, pa, keep, nkept, nms);
  *bytes = (int64_t)std::max(cl.off, cp.off);
  return GSR_OK;
}

int gsr_rcnn_loss(const GsrRcnnSpec* d, const float* scores, const float* deltas, const float* rois, const int32_t* labels,
                  const int32_t* gt_row, const float* gt_boxes, void* ws, int64_t ws_bytes, float* loss, float* grad_scores,
                  float* grad_deltas, void* stream) {
  if (int rc = rcnn_loss_spec("gsr_rcnn_loss", d)) return rc;
  if (!scores || !deltas || !rois || !labels || !gt_row || !gt_boxes || !ws || !loss)
    return set_err(GSR_ERR_INVALID, "gsr_rcnn_loss: null scores / deltas / rois / labels / gt_row / gt_boxes / ws / loss");
  gsr_rcnn::LossArgs ar;
  Carve c(ws);
  rcnn_loss_regions(c, d, ar);
  if (int rc = check_workspace("gsr_rcnn_loss", ws, ws_bytes, c.off, 16, "gsr_rcnn_workspace_bytes")) return rc;
  if (int rc = check_aligned4("gsr_rcnn_loss", scores, deltas, rois, labels, gt_row, gt_boxes, loss, grad_scores, grad_deltas)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  rcnn_copy_spec(d, ar.sp);
  ar.scores = scores; ar.deltas = deltas; ar.rois = rois; ar.labels = labels; ar.gt_row = gt_row; ar.gt_boxes = gt_boxes;
  ar.loss = loss; ar.grad_scores = grad_scores; ar.grad_deltas = grad_deltas;
  const unsigned blocks = rcnn_row_blocks(d->B, d->S);
  hipLaunchKernelGGL(gsr_rcnn::k_rcnn_count, dim3(1), dim3(gsr_rcnn::FIN_THREADS), 0, st, ar);
  LAUNCH_CHECK("gsr_rcnn_loss (count)");
  hipLaunchKernelGGL(gsr_rcnn::k_rcnn_rows, dim3(blocks), dim3(gsr_rcnn::ROW_THREADS), 0, st, ar);
  LAUNCH_CHECK("gsr_rcnn_loss (rows)");
  hipLaunchKernelGGL(gsr_rcnn::k_rcnn_final, dim3(1), dim3(gsr_rcnn::FIN_THREADS), 0, st, ar, blocks);
  LAUNCH_CHECK("gsr_rcnn_loss (final)");
  return GSR_OK;
}

int gsr_rcnn_postprocess(const GsrRcnnSpec* d, const float* scores, const float* deltas, const float* proposals, const int32_t* n_prop,
                         void* ws, int64_t ws_bytes, float* dets, int32_t* counts, void* stream) {
  if (int rc = rcnn_post_spec("gsr_rcnn_postprocess", d)) return rc;
  if (!scores || !deltas || !proposals || !ws || !dets || !counts)
    return set_err(GSR_ERR_INVALID, "gsr_rcnn_postprocess: null scores / deltas / proposals / ws / dets / counts");
  gsr_rcnn::PostArgs ar;
  int32_t *keep, *nkept;
  DetWs nms;
  Carve c(ws);
  rcnn_post_regions(c, d, ar, keep, nkept, nms);
  if (int rc = check_workspace("gsr_rcnn_postprocess", ws, ws_bytes, c.off, 16, "gsr_rcnn_workspace_bytes")) return rc;
  if (int rc = check_aligned4("gsr_rcnn_postprocess", scores, deltas, proposals, n_prop, dets, counts)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  rcnn_copy_spec(d, ar.sp);
  ar.scores = scores; ar.deltas = deltas; ar.proposals = proposals; ar.n_prop = n_prop;
  ar.dets = dets; ar.counts = counts;
  hipLaunchKernelGGL(gsr_rcnn::k_rcnn_post, dim3((unsigned)d->B), dim3(gsr_rcnn::POST_THREADS), 0, st, ar);
  LAUNCH_CHECK("gsr_rcnn_postprocess (candidates)");
  // gsr_det_nms's two launches on the compacted candidates: entries at or beyond ncand[b] do not take part
  if (int rc = launch_nms_walk("gsr_rcnn_postprocess", d->B, d->R, ar.boxes, ar.score, ar.cls, ar.ncand, d->iou_thr, d->max_det, nms,
                               keep, nkept, st))
    return rc;
  hipLaunchKernelGGL(gsr_rcnn::k_rcnn_gather, dim3((unsigned)d->B), dim3(256), 0, st, ar);
  LAUNCH_CHECK("gsr_rcnn_postprocess (gather)");
  return GSR_OK;
}

// ---- RPN proposal stage (gsr_rpn.h / gsr_rpn.hip.h): no allocation, no copy, no host wait; every entry checks the members
// of the spec it uses on the host before the first launch.  Workspace (gsr_rpn_nms alone), each region rounded up to 256
// bytes: [order B*N i32][nvalid B i32].
static void rpn_regions(Carve& c, const GsrRpnSpec* d, gsr_rpn::NmsArgs& ar) {
  ar.order = c.take<int32_t>((size_t)d->B * (size_t)d->N);
  ar.nvalid = c.take<int32_t>((size_t)d->B);
}

static void rpn_copy_spec(const GsrRpnSpec* d, gsr_rpn::Spec& sp) {
  sp.B = d->B; sp.A = d->A; sp.Hf = d->Hf; sp.Wf = d->Wf; sp.stride = d->stride; sp.shift0 = d->shift0; sp.img_w = d->img_w;
  sp.img_h = d->img_h; sp.min_size = d->min_size; sp.pre_topk = d->pre_topk; sp.level = d->level; sp.cand_offset = d->cand_offset;
  sp.N = d->N; sp.post_topk = d->post_topk; sp.iou_thr = d->iou_thr; sp.flags = d->flags;
}

static int rpn_common(const char* fn, const GsrRpnSpec* d) {
  if (!d) return set_err(GSR_ERR_INVALID, "%s: null spec", fn);
  if (d->B < 1 || d->B > 65535) return set_err(GSR_ERR_INVALID, "%s: B=%d images (1..65535)", fn, d->B);
  if (d->flags != 0u) return set_err(GSR_ERR_INVALID, "%s: unknown flags 0x%x", fn, d->flags);
  if (d->N < 1 || d->N > gsr_rpn::MAX_SLOTS) return set_err(GSR_ERR_INVALID, "%s: N=%d candidate slots per image (1..%d)", fn, d->N, gsr_rpn::MAX_SLOTS);
  return GSR_OK;
}

static int rpn_select_spec(const char* fn, const GsrRpnSpec* d) {
  if (int rc = rpn_common(fn, d)) return rc;
  if (d->A < 1 || d->Hf < 1 || d->Wf < 1) return set_err(GSR_ERR_INVALID, "%s: the level is %d anchors on %d x %d cells (sizes >= 1)", fn, d->A, d->Hf, d->Wf);
  const unsigned long long n_in = (unsigned long long)d->A * (unsigned long long)d->Hf * (unsigned long long)d->Wf;
  if (n_in > 0x7fffffffull || (unsigned long long)d->B * n_in * 4ull > 0x7fffffffull)
    return set_err(GSR_ERR_INVALID, "%s: more than 2^31 - 1 elements in logits or deltas", fn);
  if (d->stride < 1 || (long long)d->Hf * d->stride > (1ll << 24) || (long long)d->Wf * d->stride > (1ll << 24))
    return set_err(GSR_ERR_INVALID, "%s: stride=%d (>= 1, Hf * stride and Wf * stride <= 2^24)", fn, d->stride);
  if (!(d->shift0 >= -3.0e38f && d->shift0 <= 3.0e38f)) return set_err(GSR_ERR_INVALID, "%s: shift0 must be finite", fn);
  if (!finite_pos(d->img_w) || !finite_pos(d->img_h))
    return set_err(GSR_ERR_INVALID, "%s: the frame is %g x %g (finite sizes > 0)", fn, (double)d->img_w, (double)d->img_h);
  if (!finite_nonneg(d->min_size)) return set_err(GSR_ERR_INVALID, "%s: min_size must be finite and >= 0", fn);
  if (d->pre_topk < 1) return set_err(GSR_ERR_INVALID, "%s: pre_topk=%d (>= 1)", fn, d->pre_topk);
  if (d->level < 0) return set_err(GSR_ERR_INVALID, "%s: level=%d (>= 0)", fn, d->level);
  const long long n_l = (long long)std::min<unsigned long long>(n_in, (unsigned long long)d->pre_topk);
  if (d->cand_offset < 0 || (long long)d->cand_offset + n_l > (long long)d->N)
    return set_err(GSR_ERR_INVALID, "%s: cand_offset=%d with %lld slots of this level (cand_offset >= 0, cand_offset + min(pre_topk, A*Hf*Wf) <= N=%d)",
                   fn, d->cand_offset, n_l, d->N);
  return GSR_OK;
}

static int rpn_nms_spec(const char* fn, const GsrRpnSpec* d) {
  if (int rc = rpn_common(fn, d)) return rc;
  if (d->post_topk < 1 || d->post_topk > std::min(d->N, gsr_rpn::MAX_POST))
    return set_err(GSR_ERR_INVALID, "%s: post_topk=%d (1..min(N=%d, %d))", fn, d->post_topk, d->N, gsr_rpn::MAX_POST);
  if (!finite_nonneg(d->iou_thr)) return set_err(GSR_ERR_INVALID, "%s: iou_thr must be finite and >= 0", fn);
  return GSR_OK;
}

int gsr_rpn_workspace_bytes(const GsrRpnSpec* d, int64_t* bytes) {
  if (int rc = rpn_common("gsr_rpn_workspace_bytes", d)) return rc;
  if (!bytes) return set_err(GSR_ERR_INVALID, "gsr_rpn_workspace_bytes: null bytes");
  Carve c;
  gsr_rpn::NmsArgs ar;
  rpn_regions(c, d, ar);
  *bytes = (int64_t)c.off;
  return GSR_OK;
}

int gsr_rpn_select(const GsrRpnSpec* d, const float* logits, const float* deltas, const float* cell_anchors, float* cand_boxes,
                   float* cand_scores, int32_t* cand_level, void* stream) {
  if (int rc = rpn_select_spec("gsr_rpn_select", d)) return rc;
  if (!logits || !deltas || !cell_anchors || !cand_boxes || !cand_scores || !cand_level)
    return set_err(GSR_ERR_INVALID, "gsr_rpn_select: null logits / deltas / cell_anchors / cand_boxes / cand_scores / cand_level");
  if (int rc = check_aligned4("gsr_rpn_select", logits, deltas, cell_anchors, cand_boxes, cand_scores, cand_level)) return rc;
  gsr_rpn::SelectArgs ar;
  rpn_copy_spec(d, ar.sp);
  ar.logits = logits; ar.deltas = deltas; ar.cell_anchors = cell_anchors;
  ar.cand_boxes = cand_boxes; ar.cand_scores = cand_scores; ar.cand_level = cand_level;
  hipLaunchKernelGGL(gsr_rpn::k_rpn_select, dim3((unsigned)d->B), dim3(gsr_rpn::RPN_THREADS), 0, static_cast<hipStream_t>(stream), ar);
  LAUNCH_CHECK("gsr_rpn_select");
  return GSR_OK;
}

int gsr_rpn_nms(const GsrRpnSpec* d, const float* cand_boxes, const float* cand_scores, const int32_t* cand_level, void* ws,
                int64_t ws_bytes, float* proposals, float* scores, int32_t* keep, int32_t* counts, void* stream) {
  if (int rc = rpn_nms_spec("gsr_rpn_nms", d)) return rc;
  if (!cand_boxes || !cand_scores || !cand_level || !ws || !proposals || !scores || !keep || !counts)
    return set_err(GSR_ERR_INVALID, "gsr_rpn_nms: null cand_boxes / cand_scores / cand_level / ws / proposals / scores / keep / counts");
  gsr_rpn::NmsArgs ar;
  Carve c(ws);
  rpn_regions(c, d, ar);
  if (int rc = check_workspace("gsr_rpn_nms", ws, ws_bytes, c.off, 16, "gsr_rpn_workspace_bytes")) return rc;
  if (int rc = check_aligned4("gsr_rpn_nms", cand_boxes, cand_scores, cand_level, proposals, scores, keep, counts)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  rpn_copy_spec(d, ar.sp);
  ar.cand_boxes = cand_boxes; ar.cand_scores = cand_scores; ar.cand_level = cand_level;
  ar.proposals = proposals; ar.scores = scores; ar.keep = keep; ar.counts = counts;
  hipLaunchKernelGGL(gsr_rpn::k_rpn_order, dim3((unsigned)d->B), dim3(gsr_rpn::RPN_THREADS), 0, st, ar);
  LAUNCH_CHECK("gsr_rpn_nms (order)");
  hipLaunchKernelGGL(gsr_rpn::k_rpn_walk, dim3((unsigned)d->B), dim3(gsr_rpn::RPN_THREADS), 0, st, ar);
  LAUNCH_CHECK("gsr_rpn_nms (walk)");
  return GSR_OK;
}

// ---- FPN RoI pooler (gsr_fpn.h / gsr_fpn.hip.h): no allocation, no copy, no host wait, no workspace (the level lists are
// outputs the caller keeps for the backward); both entries check the whole spec on the host before the first launch.
static int fpn_spec(const char* fn, const GsrFpnSpec* d, gsr_fpn::Spec& sp, unsigned long long& tiles) {
  if (!d) return set_err(GSR_ERR_INVALID, "%s: null spec", fn);
  if (d->B < 1 || d->B > 65535) return set_err(GSR_ERR_INVALID, "%s: B=%d images (1..65535)", fn, d->B);
  if (d->S < 1 || d->S > gsr_fpn::MAX_SAMPLE) return set_err(GSR_ERR_INVALID, "%s: S=%d RoIs per image (1..%d)", fn, d->S, gsr_fpn::MAX_SAMPLE);
  if (d->Cf < 1 || d->Cf > 65535) return set_err(GSR_ERR_INVALID, "%s: Cf=%d channels (1..65535)", fn, d->Cf);
  if (d->PH < 1 || d->PH > gsr_rcnn::MAX_POOL || d->PW < 1 || d->PW > gsr_rcnn::MAX_POOL)
    return set_err(GSR_ERR_INVALID, "%s: the pooled size is %d x %d (1..%d each)", fn, d->PH, d->PW, gsr_rcnn::MAX_POOL);
  if (d->sampling_ratio < 0) return set_err(GSR_ERR_INVALID, "%s: sampling_ratio=%d (>= 0)", fn, d->sampling_ratio);
  if (d->nl < 1 || d->nl > gsr_fpn::MAX_LEVELS) return set_err(GSR_ERR_INVALID, "%s: nl=%d levels (1..%d)", fn, d->nl, gsr_fpn::MAX_LEVELS);
  if (!finite_pos(d->canonical_size)) return set_err(GSR_ERR_INVALID, "%s: canonical_size must be finite and > 0", fn);
  const unsigned long long pooled = (unsigned long long)d->B * (unsigned long long)d->S * (unsigned long long)d->Cf * (unsigned long long)(d->PH * d->PW);
  if (pooled > 0x7fffffffull) return set_err(GSR_ERR_INVALID, "%s: more than 2^31 - 1 elements in pooled", fn);
  sp = gsr_fpn::Spec{};
  sp.B = d->B; sp.S = d->S; sp.Cf = d->Cf; sp.PH = d->PH; sp.PW = d->PW; sp.sampling_ratio = d->sampling_ratio; sp.nl = d->nl;
  sp.canonical_size = d->canonical_size;
  tiles = 0;
  for (int l = 0; l < d->nl; ++l) {
    if (d->Hf[l] < 1 || d->Wf[l] < 1) return set_err(GSR_ERR_INVALID, "%s: level %d is %d x %d cells (sizes >= 1)", fn, l, d->Hf[l], d->Wf[l]);
    if (!finite_pos(d->scale[l])) return set_err(GSR_ERR_INVALID, "%s: scale[%d] must be finite and > 0", fn, l);
    if (l >= 1 && (!finite_pos(d->thr[l]) || (l >= 2 && !(d->thr[l] > d->thr[l - 1]))))
      return set_err(GSR_ERR_INVALID, "%s: thr[1..nl-1] must be finite, > 0 and strictly ascending (thr[%d])", fn, l);
    const unsigned long long hw = (unsigned long long)d->Hf[l] * (unsigned long long)d->Wf[l];
    if (hw > 0x7fffffffull || (unsigned long long)d->B * (unsigned long long)d->Cf * hw > 0x7fffffffull)
      return set_err(GSR_ERR_INVALID, "%s: more than 2^31 - 1 elements in the features of level %d", fn, l);
    tiles += (unsigned long long)((d->Hf[l] + gsr_rcnn::RB_TILE - 1) / gsr_rcnn::RB_TILE) *
             (unsigned long long)((d->Wf[l] + gsr_rcnn::RB_TILE - 1) / gsr_rcnn::RB_TILE);
    sp.Hf[l] = d->Hf[l]; sp.Wf[l] = d->Wf[l]; sp.scale[l] = d->scale[l]; sp.thr[l] = l >= 1 ? d->thr[l] : 0.0f;
  }
  if (tiles > 0x7fffffffull) return set_err(GSR_ERR_INVALID, "%s: more than 2^31 - 1 tiles in all levels", fn);
  return GSR_OK;
}

int gsr_fpn_pool(const GsrFpnSpec* d, const float* const* features, const float* rois, const int32_t* n_roi, int32_t n_roi_stride,
                 float* pooled, int32_t* roi_level, int32_t* level_list, int32_t* level_count, void* stream) {
  gsr_fpn::PoolArgs ar{};
  unsigned long long tiles = 0;
  if (int rc = fpn_spec("gsr_fpn_pool", d, ar.sp, tiles)) return rc;
  if (!features || !rois || !pooled || !roi_level || !level_list || !level_count)
    return set_err(GSR_ERR_INVALID, "gsr_fpn_pool: null features / rois / pooled / roi_level / level_list / level_count");
  if (n_roi && n_roi_stride < 1) return set_err(GSR_ERR_INVALID, "gsr_fpn_pool: n_roi_stride=%d (>= 1)", n_roi_stride);
  for (int l = 0; l < d->nl; ++l) {
    if (!features[l]) return set_err(GSR_ERR_INVALID, "gsr_fpn_pool: null features of level %d", l);
    if (int rc = check_aligned4("gsr_fpn_pool", features[l])) return rc;
    ar.features[l] = features[l];
  }
  if (int rc = check_aligned4("gsr_fpn_pool", rois, n_roi, pooled, roi_level, level_list, level_count)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ar.rois = rois; ar.n_roi = n_roi; ar.n_roi_stride = n_roi ? n_roi_stride : 0; ar.pooled = pooled;
  ar.roi_level = roi_level; ar.level_list = level_list; ar.level_count = level_count;
  hipLaunchKernelGGL(gsr_fpn::k_fpn_assign, dim3((unsigned)d->B), dim3((unsigned)((d->S + 63) / 64 * 64)), 0, st, ar);
  LAUNCH_CHECK("gsr_fpn_pool (assign)");
  const unsigned long long per_roi = (unsigned long long)d->Cf * (unsigned long long)(d->PH * d->PW);
  hipLaunchKernelGGL(gsr_fpn::k_fpn_pool, dim3((unsigned)(d->B * d->S), (unsigned)((per_roi + gsr_rcnn::RA_THREADS - 1) / gsr_rcnn::RA_THREADS)),
                     dim3(gsr_rcnn::RA_THREADS), 0, st, ar);
  LAUNCH_CHECK("gsr_fpn_pool (pool)");
  return GSR_OK;
}

int gsr_fpn_pool_backward(const GsrFpnSpec* d, const float* rois, const int32_t* level_list, const int32_t* level_count,
                          const float* grad_pooled, float* const* grad_features, int32_t accumulate, void* stream) {
  gsr_fpn::PoolArgs ar{};
  unsigned long long tiles = 0;
  if (int rc = fpn_spec("gsr_fpn_pool_backward", d, ar.sp, tiles)) return rc;
  if (!rois || !level_list || !level_count || !grad_pooled || !grad_features)
    return set_err(GSR_ERR_INVALID, "gsr_fpn_pool_backward: null rois / level_list / level_count / grad_pooled / grad_features");
  unsigned long long first = 0;
  for (int l = 0; l < gsr_fpn::MAX_LEVELS; ++l) {
    ar.tile_start[l] = (uint32_t)first;
    if (l >= d->nl) continue;
    if (!grad_features[l]) return set_err(GSR_ERR_INVALID, "gsr_fpn_pool_backward: null grad_features of level %d", l);
    if (int rc = check_aligned4("gsr_fpn_pool_backward", grad_features[l])) return rc;
    ar.grad_features[l] = grad_features[l];
    first += (unsigned long long)((d->Hf[l] + gsr_rcnn::RB_TILE - 1) / gsr_rcnn::RB_TILE) *
             (unsigned long long)((d->Wf[l] + gsr_rcnn::RB_TILE - 1) / gsr_rcnn::RB_TILE);
  }
  ar.tile_start[gsr_fpn::MAX_LEVELS] = (uint32_t)tiles;
  if (int rc = check_aligned4("gsr_fpn_pool_backward", rois, level_list, level_count, grad_pooled)) return rc;
  ar.rois = rois; ar.grad_pooled = grad_pooled;
  ar.level_list = const_cast<int32_t*>(level_list); ar.level_count = const_cast<int32_t*>(level_count);   // read only by this kernel
  ar.accumulate = accumulate != 0 ? 1 : 0;
  hipLaunchKernelGGL(gsr_fpn::k_fpn_pool_bwd,
                     dim3((unsigned)tiles, (unsigned)((d->Cf + gsr_rcnn::RB_CHUNK - 1) / gsr_rcnn::RB_CHUNK), (unsigned)d->B),
                     dim3(gsr_rcnn::RB_THREADS), 0, static_cast<hipStream_t>(stream), ar);
  LAUNCH_CHECK("gsr_fpn_pool_backward");
  return GSR_OK;
}

// ---- fused image losses (gsr_imgloss.h / gsr_imgloss.hip.h): no allocation, no copy, no host wait; the workspace is the
// caller's.  Every check is made on the host before a pointer is followed.
static bool finite_any(float v) { return v >= -3.0e38f && v <= 3.0e38f; }       // false for a NaN

static int imgloss_spec(const char* fn, const GsrImgLossSpec* d) {
  if (!d) return set_err(GSR_ERR_INVALID, "%s: null spec", fn);
  if (d->B < 1 || d->C < 1 || d->H < 1 || d->W < 1)
    return set_err(GSR_ERR_INVALID, "%s: the images are [%d,%d,%d,%d] (sizes >= 1)", fn, d->B, d->C, d->H, d->W);
  if (d->C > gsr_il::MAX_CHANNELS) return set_err(GSR_ERR_INVALID, "%s: C=%d channels (1..%d)", fn, d->C, gsr_il::MAX_CHANNELS);
  const unsigned long long hw = (unsigned long long)d->H * (unsigned long long)d->W;       // < 2^62
  if (hw > 0x7fffffffull || (unsigned long long)d->C * hw > 0x7fffffffull || (unsigned long long)d->B * (unsigned long long)d->C * hw > 0x7fffffffull)
    return set_err(GSR_ERR_INVALID, "%s: more than 2^31 - 1 elements in an image tensor", fn);
  if (!finite_any(d->w_l1) || !finite_any(d->w_l2) || !finite_any(d->w_ssim)) return set_err(GSR_ERR_INVALID, "%s: the weights must be finite", fn);
  if ((d->flags & ~(GSR_IMGLOSS_CLAMP01 | GSR_IMGLOSS_NO_GRAD)) != 0u) return set_err(GSR_ERR_INVALID, "%s: unknown flags 0x%x", fn, d->flags);
  return GSR_OK;
}

// the workspace's regions: the per-tile partials, then (with_grad) the three derivative maps
static void imgloss_regions(Carve& c, const GsrImgLossSpec* d, bool with_grad, gsr_il::Args& ar) {
  ar.tiles_x = (d->W + gsr_il::IMGLOSS_TW - 1) / gsr_il::IMGLOSS_TW;
  ar.tpp = gsr_il::tiles_of(d->H, d->W);
  const size_t tiles = (size_t)d->B * (size_t)d->C * (size_t)ar.tpp;                       // <= B C H W < 2^31
  ar.part = c.take<float>(3 * tiles);
  ar.dmaps = with_grad ? c.take<float>(3 * (size_t)d->B * (size_t)d->C * (size_t)d->H * (size_t)d->W) : nullptr;
}

int gsr_imgloss_workspace_bytes(const GsrImgLossSpec* d, int64_t* bytes) {
  if (int rc = imgloss_spec("gsr_imgloss_workspace_bytes", d)) return rc;
  if (!bytes) return set_err(GSR_ERR_INVALID, "gsr_imgloss_workspace_bytes: null bytes");
  Carve c;
  gsr_il::Args ar{};
  imgloss_regions(c, d, (d->flags & GSR_IMGLOSS_NO_GRAD) == 0u, ar);
  *bytes = (int64_t)c.off;
  return GSR_OK;
}

int gsr_imgloss(const GsrImgLossSpec* d, const float* img, const float* ref, void* ws, int64_t ws_bytes, float* terms, float* grad_img,
                float* ssim_map, void* stream) {
  if (int rc = imgloss_spec("gsr_imgloss", d)) return rc;
  if (!img || !ref || !terms || !ws) return set_err(GSR_ERR_INVALID, "gsr_imgloss: null img / ref / terms / ws");
  if (grad_img && (d->flags & GSR_IMGLOSS_NO_GRAD) != 0u) return set_err(GSR_ERR_INVALID, "gsr_imgloss: grad_img given with GSR_IMGLOSS_NO_GRAD");
  gsr_il::Args ar{};
  Carve c(ws);
  imgloss_regions(c, d, grad_img != nullptr, ar);
  if (int rc = check_workspace("gsr_imgloss", ws, ws_bytes, c.off, 16, "gsr_imgloss_workspace_bytes")) return rc;
  if (int rc = check_aligned4("gsr_imgloss", img, ref, terms, grad_img, ssim_map)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ar.B = d->B; ar.C = d->C; ar.H = d->H; ar.W = d->W; ar.w_l1 = d->w_l1; ar.w_l2 = d->w_l2; ar.w_ssim = d->w_ssim; ar.flags = d->flags;
  ar.img = img; ar.ref = ref; ar.terms = terms; ar.grad = grad_img; ar.ssim_map = ssim_map;
  ar.inv_n = 1.0f / (float)((long long)d->C * d->H * d->W);
  const unsigned tiles = (unsigned)((size_t)d->B * (size_t)d->C * (size_t)ar.tpp);
  hipLaunchKernelGGL(gsr_il::k_imgloss_tile, dim3(tiles), dim3(gsr_il::IL_THREADS), 0, st, ar);
  LAUNCH_CHECK("gsr_imgloss (tiles)");
  hipLaunchKernelGGL(gsr_il::k_imgloss_sum, dim3((unsigned)d->B), dim3(gsr_il::SUM_THREADS), 0, st, ar);
  LAUNCH_CHECK("gsr_imgloss (sum)");
  if (grad_img) {
    hipLaunchKernelGGL(gsr_il::k_imgloss_grad, dim3(tiles), dim3(gsr_il::IL_THREADS), 0, st, ar);
    LAUNCH_CHECK("gsr_imgloss (gradient)");
  }
  return GSR_OK;
}

// ---- RPN loss stage (gsr_rpnloss.h / gsr_rpnloss.hip.h): no allocation, no copy, no host wait, no float atomics; the
// workspace is the caller's and one sizer serves both entries.  Every check is made on the host before a pointer is followed.
// Workspace, each region rounded up to 256 bytes: [rowmax B*M u32][kind counts B*2 i32][thresholds B*2 u64][pre-labels B*R
// i32][slab B*tiles*2 f32].
struct RpnLossPlan {
  gsr_rpnl::Spec sp;
  int32_t off[gsr_rpnl::MAX_LEVELS + 1];
  uint32_t tile_start[gsr_rpnl::MAX_LEVELS + 1];
  long long R;
  unsigned long long tiles;
};

static int rpnloss_spec(const char* fn, const GsrRpnLossSpec* d, RpnLossPlan& p) {
  namespace RL = gsr_rpnl;
  if (!d) return set_err(GSR_ERR_INVALID, "%s: null spec", fn);
  if (d->B < 1 || d->B > 65535) return set_err(GSR_ERR_INVALID, "%s: B=%d images (1..65535)", fn, d->B);
  if (d->M < 1 || d->M > RL::MAX_ROWS) return set_err(GSR_ERR_INVALID, "%s: M=%d gt rows (1..%d)", fn, d->M, RL::MAX_ROWS);
  if (d->nl < 1 || d->nl > RL::MAX_LEVELS) return set_err(GSR_ERR_INVALID, "%s: nl=%d levels (1..%d)", fn, d->nl, RL::MAX_LEVELS);
  if (d->flags != 0u) return set_err(GSR_ERR_INVALID, "%s: unknown flags 0x%x", fn, d->flags);
  if (d->batch_per_image < 1 || d->batch_per_image > RL::MAX_BATCH)
    return set_err(GSR_ERR_INVALID, "%s: batch_per_image=%d (1..%d)", fn, d->batch_per_image, RL::MAX_BATCH);
  if (d->pos_quota < 0 || d->pos_quota > d->batch_per_image)
    return set_err(GSR_ERR_INVALID, "%s: pos_quota=%d (0..batch_per_image=%d)", fn, d->pos_quota, d->batch_per_image);
  if (!finite_nonneg(d->iou_lo) || !finite_nonneg(d->iou_hi) || !(d->iou_lo <= d->iou_hi))
    return set_err(GSR_ERR_INVALID, "%s: the thresholds are %g and %g (finite, 0 <= iou_lo <= iou_hi)", fn, (double)d->iou_lo, (double)d->iou_hi);
  if (!all_finite_nonneg({d->beta, d->w_cls, d->w_loc})) return set_err(GSR_ERR_INVALID, "%s: beta and the weights must be finite and >= 0", fn);
  p.sp = RL::Spec{};
  p.sp.B = d->B; p.sp.M = d->M; p.sp.nl = d->nl; p.sp.batch_per_image = d->batch_per_image; p.sp.pos_quota = d->pos_quota;
  p.sp.seed = d->seed; p.sp.iou_lo = d->iou_lo; p.sp.iou_hi = d->iou_hi; p.sp.beta = d->beta; p.sp.w_cls = d->w_cls; p.sp.w_loc = d->w_loc;
  p.sp.flags = d->flags;
  unsigned long long R = 0, tiles = 0;
  for (int l = 0; l < RL::MAX_LEVELS; ++l) {
    p.tile_start[l] = (uint32_t)tiles;
    if (l >= d->nl) continue;
    if (d->A[l] < 1 || d->Hf[l] < 1 || d->Wf[l] < 1)
      return set_err(GSR_ERR_INVALID, "%s: level %d is %d anchors on %d x %d cells (sizes >= 1)", fn, l, d->A[l], d->Hf[l], d->Wf[l]);
    const unsigned long long hw = (unsigned long long)d->Hf[l] * (unsigned long long)d->Wf[l];                                   // < 2^62
    if (hw > (unsigned long long)RL::MAX_ANCHORS || (unsigned long long)d->A[l] * hw > (unsigned long long)RL::MAX_ANCHORS)       // < 2^55
      return set_err(GSR_ERR_INVALID, "%s: more than 2^24 anchors in level %d", fn, l);
    const unsigned long long n_l = (unsigned long long)d->A[l] * hw;
    if ((unsigned long long)d->B * n_l * 4ull > 0x7fffffffull)
      return set_err(GSR_ERR_INVALID, "%s: more than 2^31 - 1 elements in the deltas of level %d", fn, l);
    if (d->stride[l] < 1 || (long long)d->Hf[l] * d->stride[l] > (1ll << 24) || (long long)d->Wf[l] * d->stride[l] > (1ll << 24))
      return set_err(GSR_ERR_INVALID, "%s: stride[%d]=%d (>= 1, Hf * stride and Wf * stride <= 2^24)", fn, l, d->stride[l]);
    if (!finite_any(d->shift0[l])) return set_err(GSR_ERR_INVALID, "%s: shift0[%d] must be finite", fn, l);
    p.sp.A[l] = d->A[l]; p.sp.Hf[l] = d->Hf[l]; p.sp.Wf[l] = d->Wf[l]; p.sp.stride[l] = d->stride[l]; p.sp.shift0[l] = d->shift0[l];
    R += n_l;
    tiles += (n_l + gsr_rpnl::RL_THREADS - 1) / gsr_rpnl::RL_THREADS;
  }
  p.tile_start[RL::MAX_LEVELS] = (uint32_t)tiles;
  if (R > (unsigned long long)RL::MAX_ANCHORS) return set_err(GSR_ERR_INVALID, "%s: R=%llu anchors per image in all levels (1..2^24)", fn, R);
  if ((unsigned long long)d->B * R > 0x7fffffffull) return set_err(GSR_ERR_INVALID, "%s: more than 2^31 - 1 elements in labels", fn);
  p.R = RL::level_offsets(p.sp, p.off);
  p.tiles = tiles;
  return GSR_OK;
}

static void rpnloss_regions(Carve& c, const RpnLossPlan& p, gsr_rpnl::LabelArgs& la, gsr_rpnl::LossArgs& lo) {
  const size_t B = (size_t)p.sp.B;
  la.rowmax = c.take<uint32_t>(B * (size_t)p.sp.M);
  la.kind_count = c.take<int32_t>(B * 2);
  la.thr = c.take<unsigned long long>(B * 2);
  la.pre = c.take<int32_t>(B * (size_t)p.R);
  lo.slab = c.take<float>(B * (size_t)p.tiles * 2);
}

// nl level pointers of a host array: each non-null and 4-byte aligned
static int rpnloss_levels(const char* fn, const char* what, const float* const* src, int nl, const float** dst) {
  for (int l = 0; l < nl; ++l) {
    if (!src[l]) return set_err(GSR_ERR_INVALID, "%s: null %s of level %d", fn, what, l);
    if (int rc = check_aligned4(fn, src[l])) return rc;
    dst[l] = src[l];
  }
  return GSR_OK;
}

int gsr_rpnloss_workspace_bytes(const GsrRpnLossSpec* d, int64_t* bytes) {
  RpnLossPlan p;
  if (int rc = rpnloss_spec("gsr_rpnloss_workspace_bytes", d, p)) return rc;
  if (!bytes) return set_err(GSR_ERR_INVALID, "gsr_rpnloss_workspace_bytes: null bytes");
  Carve c;
  gsr_rpnl::LabelArgs la{};
  gsr_rpnl::LossArgs lo{};
  rpnloss_regions(c, p, la, lo);
  *bytes = (int64_t)c.off;
  return GSR_OK;
}

int gsr_rpnloss_label(const GsrRpnLossSpec* d, const float* const* cell_anchors, const float* gt_boxes, const int32_t* gt_cls, void* ws,
                      int64_t ws_bytes, int32_t* labels, int32_t* matched, int32_t* counts, int32_t* prelabels, void* stream) {
  namespace RL = gsr_rpnl;
  const char* fn = "gsr_rpnloss_label";
  RpnLossPlan p;
  if (int rc = rpnloss_spec(fn, d, p)) return rc;
  if (!cell_anchors || !gt_boxes || !gt_cls || !ws || !labels || !matched || !counts)
    return set_err(GSR_ERR_INVALID, "%s: null cell_anchors / gt_boxes / gt_cls / ws / labels / matched / counts", fn);
  RL::LabelArgs ar{};
  RL::LossArgs unused{};
  Carve c(ws);
  rpnloss_regions(c, p, ar, unused);
  if (int rc = check_workspace(fn, ws, ws_bytes, c.off, 16, "gsr_rpnloss_workspace_bytes")) return rc;
  if (int rc = rpnloss_levels(fn, "cell_anchors", cell_anchors, d->nl, ar.cells)) return rc;
  if (int rc = check_aligned4(fn, gt_boxes, gt_cls, labels, matched, counts, prelabels)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ar.sp = p.sp;
  for (int l = 0; l <= RL::MAX_LEVELS; ++l) ar.off[l] = p.off[l];
  ar.R = (int32_t)p.R;
  ar.gt_boxes = gt_boxes; ar.gt_cls = gt_cls; ar.prelabels = prelabels; ar.labels = labels; ar.matched = matched; ar.counts = counts;
  const unsigned n_init = (unsigned)d->B * (unsigned)std::max(d->M, 2);
  const dim3 per_anchor((unsigned)((p.R + RL::RL_THREADS - 1) / RL::RL_THREADS), (unsigned)d->B);
  hipLaunchKernelGGL(RL::k_rpnloss_init, dim3((n_init + RL::RL_THREADS - 1) / RL::RL_THREADS), dim3(RL::RL_THREADS), 0, st, ar);
  LAUNCH_CHECK("gsr_rpnloss_label (init)");
  hipLaunchKernelGGL(RL::k_rpnloss_rowmax, per_anchor, dim3(RL::RL_THREADS), 0, st, ar);
  LAUNCH_CHECK("gsr_rpnloss_label (row maxima)");
  hipLaunchKernelGGL(RL::k_rpnloss_prelabel, per_anchor, dim3(RL::RL_THREADS), 0, st, ar);
  LAUNCH_CHECK("gsr_rpnloss_label (pre-labels)");
  hipLaunchKernelGGL(RL::k_rpnloss_select, dim3(2u, (unsigned)d->B), dim3(RL::RL_SEL_THREADS), 0, st, ar);
  LAUNCH_CHECK("gsr_rpnloss_label (select)");
  hipLaunchKernelGGL(RL::k_rpnloss_labels, per_anchor, dim3(RL::RL_THREADS), 0, st, ar);
  LAUNCH_CHECK("gsr_rpnloss_label (labels)");
  return GSR_OK;
}

int gsr_rpnloss(const GsrRpnLossSpec* d, const int32_t* labels, const int32_t* matched, const float* const* logits, const float* const* deltas,
                const float* const* cell_anchors, const float* gt_boxes, void* ws, int64_t ws_bytes, float* loss, float* const* grad_logits,
                float* const* grad_deltas, void* stream) {
  namespace RL = gsr_rpnl;
  const char* fn = "gsr_rpnloss";
  RpnLossPlan p;
  if (int rc = rpnloss_spec(fn, d, p)) return rc;
  if (!labels || !matched || !logits || !deltas || !cell_anchors || !gt_boxes || !ws || !loss)
    return set_err(GSR_ERR_INVALID, "%s: null labels / matched / logits / deltas / cell_anchors / gt_boxes / ws / loss", fn);
  RL::LabelArgs unused{};
  RL::LossArgs ar{};
  Carve c(ws);
  rpnloss_regions(c, p, unused, ar);
  if (int rc = check_workspace(fn, ws, ws_bytes, c.off, 16, "gsr_rpnloss_workspace_bytes")) return rc;
  if (int rc = rpnloss_levels(fn, "logits", logits, d->nl, ar.logits)) return rc;
  if (int rc = rpnloss_levels(fn, "deltas", deltas, d->nl, ar.deltas)) return rc;
  if (int rc = rpnloss_levels(fn, "cell_anchors", cell_anchors, d->nl, ar.cells)) return rc;
  if (grad_logits)
    if (int rc = rpnloss_levels(fn, "grad_logits", grad_logits, d->nl, const_cast<const float**>(ar.grad_logits))) return rc;
  if (grad_deltas)
    if (int rc = rpnloss_levels(fn, "grad_deltas", grad_deltas, d->nl, const_cast<const float**>(ar.grad_deltas))) return rc;
  if (int rc = check_aligned4(fn, labels, matched, gt_boxes, loss)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ar.sp = p.sp;
  for (int l = 0; l <= RL::MAX_LEVELS; ++l) { ar.off[l] = p.off[l]; ar.tile_start[l] = p.tile_start[l]; }
  ar.R = (int32_t)p.R;
  ar.gt_boxes = gt_boxes; ar.labels = labels; ar.matched = matched; ar.loss = loss;
  ar.norm = (float)((long long)d->batch_per_image * (long long)d->B);
  hipLaunchKernelGGL(RL::k_rpnloss_terms, dim3((unsigned)p.tiles, (unsigned)d->B), dim3(RL::RL_THREADS), 0, st, ar);
  LAUNCH_CHECK("gsr_rpnloss (terms)");
  hipLaunchKernelGGL(RL::k_rpnloss_final, dim3(1), dim3(RL::RL_THREADS), 0, st, ar, (unsigned)((unsigned long long)d->B * p.tiles));
  LAUNCH_CHECK("gsr_rpnloss (final)");
  return GSR_OK;
}

// ---- object-map classifier (gsr_objmap.h / gsr_objmap.hip.h): no allocation, no copy, no host wait, no float atomics; the
// workspace is the caller's.  Every check is made on the host before a pointer is followed.
static int objmap_spec(const char* fn, const GsrObjMapSpec* d) {
  if (!d) return set_err(GSR_ERR_INVALID, "%s: null spec", fn);
  if (d->B < 1 || d->H < 1 || d->W < 1) return set_err(GSR_ERR_INVALID, "%s: the map is [%d,16,%d,%d] (sizes >= 1)", fn, d->B, d->H, d->W);
  if (d->K < 1 || d->K > gsr_om::MAX_CLASSES) return set_err(GSR_ERR_INVALID, "%s: K=%d classes (1..%d)", fn, d->K, gsr_om::MAX_CLASSES);
  if (d->B > 65535) return set_err(GSR_ERR_INVALID, "%s: B=%d images (1..65535)", fn, d->B);
  const unsigned long long hw = (unsigned long long)d->H * (unsigned long long)d->W;       // < 2^62
  if (hw > 0x7fffffffull || (unsigned long long)d->B * gsr_om::CH * hw > 0x7fffffffull ||
      (unsigned long long)d->B * (unsigned long long)d->K * 5ull > 0x7fffffffull)
    return set_err(GSR_ERR_INVALID, "%s: more than 2^31 - 1 elements in a tensor", fn);
  if ((d->flags & ~GSR_OBJMAP_LOSS) != 0u) return set_err(GSR_ERR_INVALID, "%s: unknown flags 0x%x", fn, d->flags);
  return GSR_OK;
}

// the workspace's regions, with GSR_OBJMAP_LOSS alone: the classify workgroups' CE partials, the init workgroups' counts
static void objmap_regions(Carve& c, const GsrObjMapSpec* d, gsr_om::Args& ar) {
  ar.hw = d->H * d->W;
  ar.nblk = gsr_om::blocks_of(d->H, d->W);
  if ((d->flags & GSR_OBJMAP_LOSS) == 0u) return;
  ar.slab = c.take<float>((size_t)d->B * (size_t)ar.nblk);
  ar.vpart = c.take<int32_t>((size_t)d->B * gsr_om::INIT_BLOCKS);
}

int gsr_objmap_workspace_bytes(const GsrObjMapSpec* d, int64_t* bytes) {
  if (int rc = objmap_spec("gsr_objmap_workspace_bytes", d)) return rc;
  if (!bytes) return set_err(GSR_ERR_INVALID, "gsr_objmap_workspace_bytes: null bytes");
  Carve c;
  gsr_om::Args ar{};
  objmap_regions(c, d, ar);
  *bytes = (int64_t)c.off;
  return GSR_OK;
}

int gsr_objmap(const GsrObjMapSpec* d, const float* objmap, const float* weight, const float* bias, const int32_t* target,
               const uint8_t* palette, void* ws, int64_t ws_bytes, int32_t* ids, float* conf, int32_t* stats, uint8_t* paint,
               float* terms, float* grad, void* stream) {
  const char* fn = "gsr_objmap";
  if (int rc = objmap_spec(fn, d)) return rc;
  if (!objmap || !weight || !bias || !ids) return set_err(GSR_ERR_INVALID, "gsr_objmap: null objmap / weight / bias / ids");
  if (paint && !palette) return set_err(GSR_ERR_INVALID, "gsr_objmap: paint given without a palette");
  const bool loss_flag = (d->flags & GSR_OBJMAP_LOSS) != 0u;
  if ((terms || grad) && !loss_flag) return set_err(GSR_ERR_INVALID, "gsr_objmap: terms / grad given without GSR_OBJMAP_LOSS");
  if ((terms || grad) && !target) return set_err(GSR_ERR_INVALID, "gsr_objmap: terms / grad given without a target");
  if (loss_flag && !ws) return set_err(GSR_ERR_INVALID, "gsr_objmap: null ws with GSR_OBJMAP_LOSS");
  gsr_om::Args ar{};
  Carve c(ws);
  objmap_regions(c, d, ar);
  if (int rc = check_workspace(fn, ws, ws_bytes, c.off, 16, "gsr_objmap_workspace_bytes")) return rc;
  if (int rc = check_aligned4(fn, objmap, weight, bias, target, ids, conf, stats, terms, grad)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  ar.B = d->B; ar.H = d->H; ar.W = d->W; ar.K = d->K;
  ar.objmap = objmap; ar.target = target; ar.palette = palette;
  ar.ids = ids; ar.conf = conf; ar.stats = stats; ar.paint = paint; ar.terms = terms; ar.grad = grad;
  const bool loss = terms || grad;
  const dim3 threads(gsr_om::OM_THREADS);
  if (stats || loss) {
    hipLaunchKernelGGL(gsr_om::k_objmap_init, dim3(gsr_om::INIT_BLOCKS, (unsigned)d->B), threads, 0, st, ar, weight, bias, loss ? 1 : 0);
    LAUNCH_CHECK("gsr_objmap (init)");
  }
  const dim3 grid((unsigned)ar.nblk, (unsigned)d->B);
  const size_t lds = stats ? 5 * (size_t)d->K * sizeof(int32_t) : 0;
  if (loss) hipLaunchKernelGGL(gsr_om::k_objmap_classify<true>, grid, threads, lds, st, ar, weight, bias);
  else hipLaunchKernelGGL(gsr_om::k_objmap_classify<false>, grid, threads, lds, st, ar, weight, bias);
  LAUNCH_CHECK("gsr_objmap (classify)");
  if (stats || terms) {
    hipLaunchKernelGGL(gsr_om::k_objmap_final, dim3((unsigned)d->B), threads, 0, st, ar);
    LAUNCH_CHECK("gsr_objmap (final)");
  }
  return GSR_OK;
}

int gsr_debug_wave_clock(unsigned long long* buf) {
  g_wave_clock.store(buf);
  return GSR_OK;
}

int gsr_debug_wave_clock_fwd(unsigned long long* buf) {
  g_wave_clock_fwd.store(buf);
  return GSR_OK;
}

int gsr_test_scan(const uint32_t* in, uint32_t* out, uint32_t n, void* stream) {
  if (!in || !out) return set_err(GSR_ERR_INVALID, "gsr_test_scan: null argument");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int dev = cur_dev();
  void* blk = pool_alloc(dev, sizeof(uint32_t) * ((size_t)n / 2048 + 2), st);
  if (!blk) return set_err(GSR_ERR_NOMEM, "gsr_test_scan: allocation failed");
  scan_exclusive_u32(in, out, n, nullptr, static_cast<uint32_t*>(blk), st);
  pool_free(dev, blk);
  LAUNCH_CHECK("test scan");
  return GSR_OK;
}

int gsr_test_sort_pairs(uint32_t* keys, uint32_t* vals, uint32_t n, int32_t begin_bit, int32_t end_bit, int32_t iota,
                        void* stream) {
  if (!keys || !vals) return set_err(GSR_ERR_INVALID, "gsr_test_sort_pairs: null argument");
  if (n == 0) return GSR_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int dev = cur_dev();
  const uint32_t tbl = radix_table_words(n);
  void* blk = pool_alloc(dev, sizeof(uint32_t) * ((size_t)2 * n + tbl + RS_BINS), st);
  if (!blk) return set_err(GSR_ERR_NOMEM, "gsr_test_sort_pairs: allocation failed");
  uint32_t* k1 = static_cast<uint32_t*>(blk);
  uint32_t* v1 = k1 + n;
  uint32_t* table = v1 + n;
  uint32_t* sums = table + tbl;
  const int res = radix_sort_pairs(keys, vals, k1, v1, n, nullptr, begin_bit, end_bit, iota != 0, table, sums, st);
  if (res) {
    (void)hipMemcpyAsync(keys, k1, sizeof(uint32_t) * n, hipMemcpyDeviceToDevice, st);
    (void)hipMemcpyAsync(vals, v1, sizeof(uint32_t) * n, hipMemcpyDeviceToDevice, st);
  }
  pool_free(dev, blk);
  LAUNCH_CHECK("test sort");
  return GSR_OK;
}

int gsr_test_scan_ex(const uint32_t* in, uint32_t* out, uint32_t n, const uint32_t* n_dev, uint32_t* chunk_first,
                     uint32_t chunk_len, uint32_t chunk_cap, void* stream) {
  if (!in || !out) return set_err(GSR_ERR_INVALID, "gsr_test_scan_ex: null argument");
  if (chunk_first && chunk_len == 0u) return set_err(GSR_ERR_INVALID, "gsr_test_scan_ex: chunk_first needs chunk_len > 0");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int dev = cur_dev();
  void* blk = pool_alloc(dev, sizeof(uint32_t) * ((size_t)n / 2048 + 2), st);
  if (!blk) return set_err(GSR_ERR_NOMEM, "gsr_test_scan_ex: allocation failed");
  scan_exclusive_u32(in, out, n, n_dev, static_cast<uint32_t*>(blk), st, chunk_first, chunk_first ? chunk_len : 1u,
                     chunk_first ? chunk_cap : 0u);
  pool_free(dev, blk);
  LAUNCH_CHECK("test scan");
  return GSR_OK;
}

int gsr_test_sort_pairs_ex(uint32_t* keys, uint32_t* vals, uint32_t n, const uint32_t* n_dev, int32_t begin_bit,
                           int32_t end_bit, int32_t iota, int32_t rounds, uint32_t* key_ranges, uint32_t key_limit,
                           void* stream) {
  if (!keys || !vals) return set_err(GSR_ERR_INVALID, "gsr_test_sort_pairs_ex: null argument");
  if (rounds != 0 && rounds != RS_ROUNDS_MIN && rounds != RS_ROUNDS_MAX)
    return set_err(GSR_ERR_INVALID, "gsr_test_sort_pairs_ex: rounds %d (0 = automatic, 8 or 16)", rounds);
  if (begin_bit < 0 || end_bit > 32 || end_bit < begin_bit)
    return set_err(GSR_ERR_INVALID, "gsr_test_sort_pairs_ex: bad bit range [%d, %d)", begin_bit, end_bit);
  if (key_ranges && begin_bit != 0)
    return set_err(GSR_ERR_INVALID, "gsr_test_sort_pairs_ex: key_ranges need begin_bit 0 (a sort on the whole key), got %d", begin_bit);
  if (n == 0) return GSR_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int dev = cur_dev();
  const uint32_t tbl = radix_table_words(n);
  void* blk = pool_alloc(dev, sizeof(uint32_t) * ((size_t)2 * n + tbl + RS_BINS), st);
  if (!blk) return set_err(GSR_ERR_NOMEM, "gsr_test_sort_pairs_ex: allocation failed");
  uint32_t* k1 = static_cast<uint32_t*>(blk);
  uint32_t* v1 = k1 + n;
  uint32_t* table = v1 + n;
  uint32_t* sums = table + tbl;
  const int res = radix_sort_pairs(keys, vals, k1, v1, n, n_dev, begin_bit, end_bit, iota != 0, table, sums, st, false,
                                   key_ranges, key_limit, rounds);
  if (res) {
    (void)hipMemcpyAsync(keys, k1, sizeof(uint32_t) * n, hipMemcpyDeviceToDevice, st);
    (void)hipMemcpyAsync(vals, v1, sizeof(uint32_t) * n, hipMemcpyDeviceToDevice, st);
  }
  pool_free(dev, blk);
  LAUNCH_CHECK("test sort");
  return GSR_OK;
}

void gsr_profile(int32_t enable) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  g_prof = (uint32_t)enable;
  for (ProfSpan& s : g_spans) { g_free_events.push_back(s.a); g_free_events.push_back(s.b); }
  g_spans.clear();
  for (int i = 0; i < GSR_STAGE_COUNT; ++i) { g_ms[i] = 0.f; g_calls[i] = 0; }
}

int gsr_profile_timeline(float* out, int max_spans) {
  // diagnostic: (stage, start ms, end ms) of every recorded span, relative to the first span's start; consumes them
  std::lock_guard<std::mutex> lk(g_prof_mu);
  int n = 0;
  hipEvent_t base = g_spans.empty() ? nullptr : g_spans[0].a;
  for (ProfSpan& s : g_spans) {
    if (hipEventSynchronize(s.b) != hipSuccess) break;
    float t0 = 0.f, t1 = 0.f;
    if (n < max_spans && out && hipEventElapsedTime(&t0, base, s.a) == hipSuccess &&
        hipEventElapsedTime(&t1, base, s.b) == hipSuccess) {
      out[3 * n] = (float)s.stage; out[3 * n + 1] = t0; out[3 * n + 2] = t1;
      ++n;
    }
  }
  for (ProfSpan& s : g_spans) { g_free_events.push_back(s.a); g_free_events.push_back(s.b); }
  g_spans.clear();
  (void)hipGetLastError();
  return n;
}

int gsr_profile_read(float* ms, int64_t* calls) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (ProfSpan& s : g_spans) {
    hipError_t e = hipEventSynchronize(s.b);
    if (e != hipSuccess) return set_err(GSR_ERR_DEVICE, "gsr_profile_read: %s", hipGetErrorString(e));
    float m = 0.f;
    if (hipEventElapsedTime(&m, s.a, s.b) == hipSuccess) { g_ms[s.stage] += m; g_calls[s.stage] += 1; }
    g_free_events.push_back(s.a); g_free_events.push_back(s.b);
  }
  g_spans.clear();
  for (int i = 0; i < GSR_STAGE_COUNT; ++i) {
    if (ms) ms[i] = g_ms[i];
    if (calls) calls[i] = g_calls[i];
  }
  return GSR_OK;
}

}  // extern "C"
