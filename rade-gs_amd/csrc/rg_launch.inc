// rg_launch.inc -- host orchestration + C ABI (include/radegs.h).  Included at the end of
// radegs_kernels.hip so the kernels above are visible; not a stand-alone translation unit.
//
//   radegs_forward   follows the stage order of Rasterizer::forward  (DGR/cuda_rasterizer/rasterizer_impl.cu:254-425)
//   radegs_backward  follows Rasterizer::backward                    (rasterizer_impl.cu:429-571)
#include <dlfcn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/radegs.h"
#include "rg_prims.h"

namespace rg {

static thread_local std::string g_last_error;
static thread_local int g_last_forward_streams = -1;   // radegs_last_forward_used_streams

static int fail(int code, const char* what, hipError_t e = hipSuccess) {
  char buf[512];
  if (e != hipSuccess) snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
  else snprintf(buf, sizeof(buf), "%s", what);
  g_last_error = buf;
  return code;
}

#define RG_HIP(call)                                                        \
  do {                                                                      \
    hipError_t e_ = (call);                                                 \
    if (e_ != hipSuccess) return fail(RADEGS_ERR_HIP, #call, e_);           \
  } while (0)

#define RG_LAUNCH_CHECK(name, dbg, stream)                                  \
  do {                                                                      \
    hipError_t e_ = hipGetLastError();                                      \
    if (e_ != hipSuccess) return fail(RADEGS_ERR_HIP, name, e_);            \
    if (dbg) {                                                              \
      e_ = hipStreamSynchronize(stream);                                    \
      if (e_ != hipSuccess) return fail(RADEGS_ERR_HIP, name " (debug sync)", e_); \
    }                                                                       \
  } while (0)

// getHigherMsb, DGR/cuda_rasterizer/rasterizer_impl.cu:35-50 (number of tile-id bits to sort on)
static uint32_t higher_msb(uint32_t n) {
  uint32_t msb = sizeof(n) * 4, step = msb;
  while (step > 1) {
    step /= 2;
    if (n >> msb) msb += step; else msb -= step;
  }
  if (n >> msb) msb++;
  return msb;
}

// rocPRIM cross-check of the hand-written scan / sorts (RADEGS_PRIMS=rocprim): a test-only shared object next to this library,
// loaded on demand -- it is not linked into the product.
struct PrimsCheck {
  prims_temp_geom_fn temp_geom = nullptr; prims_temp_bin_fn temp_bin = nullptr; prims_sort_by_depth_fn sort_by_depth = nullptr;
  prims_scan_fn scan = nullptr; prims_sort_by_tile_fn sort_by_tile = nullptr;
  bool ok = false;
};
static const PrimsCheck& prims_check() {
  static const PrimsCheck pc = [] {
    PrimsCheck c;
    Dl_info info;
    if (!dladdr(reinterpret_cast<const void*>(&prims_check), &info) || !info.dli_fname) return c;
    std::string path(info.dli_fname);
    const size_t slash = path.rfind('/');
    path = (slash == std::string::npos ? std::string(".") : path.substr(0, slash)) + "/libradegs_prims_check.so";
    void* h = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!h) return c;
    c.temp_geom = reinterpret_cast<prims_temp_geom_fn>(dlsym(h, "radegs_prims_temp_bytes_geom"));
    c.temp_bin = reinterpret_cast<prims_temp_bin_fn>(dlsym(h, "radegs_prims_temp_bytes_bin"));
    c.sort_by_depth = reinterpret_cast<prims_sort_by_depth_fn>(dlsym(h, "radegs_prims_sort_by_depth"));
    c.scan = reinterpret_cast<prims_scan_fn>(dlsym(h, "radegs_prims_scan_tiles_in_depth_order"));
    c.sort_by_tile = reinterpret_cast<prims_sort_by_tile_fn>(dlsym(h, "radegs_prims_sort_by_tile"));
    c.ok = c.temp_geom && c.temp_bin && c.sort_by_depth && c.scan && c.sort_by_tile;
    return c;
  }();
  return pc;
}

// The library's run-time switches (INTEGRATION.md section 4 documents each): environment variables, read ONCE when the library is first
// used and again only through radegs_reload_env() (the test-suite flips them between cases inside one process).
struct Switches {
  int streams = -1;            // RADEGS_STREAMS=0/1: force the tile-wide kernels / the sub-tile entry streams (default: chosen per launch)
  int streams_bwd = 1;         // RADEGS_STREAMS_BWD=0: tile-wide backward even after a stream forward (it is valid after either)
  size_t streams_max_bytes = size_t(4096) << 20;   // RADEGS_STREAMS_MAX_MB: entry-stream storage above this is not asked for
  int speculate = 1;           // RADEGS_SPECULATE=0: the reference's blocking read-back of num_rendered
  int speculate_hint = 0;      // RADEGS_SPECULATE_HINT=n: force the capacity prediction (tests of the redo path)
  int speculate_chunks = 0;    // RADEGS_SPECULATE_CHUNKS=n: force the predicted entry-stream storage, in chunks of 192 B (same purpose)
  bool rocprim = false;        // RADEGS_PRIMS=rocprim: scan / sorts through the test-only device-library cross-check
  int bwd_ppl = 0;             // RADEGS_BWD_PPL=2/4: pixels per lane of the tile-wide backward (default: chosen per launch)
  int mask_in_key = 0;         // RADEGS_MASK_IN_KEY=1: the block masks of the entry streams ride in 32-bit tile keys at any scene size (the
                               // layout scenes of 2^24 Gaussians and more use; lets a small test scene walk that path)
};
static int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  if (!v || !*v) return dflt;
  return atoi(v);
}
static Switches read_switches() {
  Switches w;
  w.streams = env_int("RADEGS_STREAMS", -1);
  w.streams_bwd = env_int("RADEGS_STREAMS_BWD", 1);
  w.streams_max_bytes = (size_t)std::max(0, env_int("RADEGS_STREAMS_MAX_MB", 4096)) << 20;
  w.speculate = env_int("RADEGS_SPECULATE", 1);
  w.speculate_hint = env_int("RADEGS_SPECULATE_HINT", 0);
  w.speculate_chunks = env_int("RADEGS_SPECULATE_CHUNKS", 0);
  const char* pr = getenv("RADEGS_PRIMS");
  w.rocprim = pr && !strcmp(pr, "rocprim");
  w.bwd_ppl = env_int("RADEGS_BWD_PPL", 0);
  w.mask_in_key = env_int("RADEGS_MASK_IN_KEY", 0);
  return w;
}
static std::mutex g_sw_mu;
static Switches& switches_storage() { static Switches w = read_switches(); return w; }
static Switches switches() { std::lock_guard<std::mutex> l(g_sw_mu); return switches_storage(); }

// ---- optional per-stage timing with HIP events on the launch stream (bench.py's roofline leg) ----
enum Stage { ST_PRE_FWD = 0, ST_SORT_DEPTH, ST_SCAN, ST_EMIT, ST_SORT_TILE, ST_RANGES, ST_BLEND_FWD, ST_ACC_ZERO, ST_BLEND_BWD,
             ST_PRE_BWD, ST_BLOCK_LISTS, ST_ORDERED_SORT, ST_ORDERED_SUMS, ST_COUNT };
static const char* kStageNames[ST_COUNT] = {"preprocess_fwd", "sort_depth", "scan", "emit_instances", "sort_tile", "tile_ranges",
                                            "blend_fwd", "acc_zero", "blend_bwd", "preprocess_bwd", "block_lists", "ordered_sort",
                                            "ordered_sums"};
struct ProfRec { int stage; hipEvent_t a, b; };
// atomics: autograd runs every device's backward on its own worker thread, and the switches are flipped from the main thread
static std::atomic<bool> g_prof_on{false};
static std::atomic<int> g_prof_only{-1};   // >= 0: time this stage only (an event pair costs ~10 us of stream bubble per stage boundary)
static std::atomic<int> g_prof_every{1};   // with g_prof_only: time every n-th launch of that stage (the pair's bubble then costs 1/n per step)
static std::atomic<unsigned> g_prof_tick{0};
static std::vector<ProfRec> g_prof_recs;
static std::vector<hipEvent_t> g_prof_pool;
static std::mutex g_prof_mu;

static hipEvent_t prof_event() {
  if (!g_prof_pool.empty()) { hipEvent_t e = g_prof_pool.back(); g_prof_pool.pop_back(); return e; }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}
struct StageTimer {
  hipStream_t s; hipEvent_t a = nullptr, b = nullptr; int stage; bool on;
  StageTimer(int st, hipStream_t stream) : s(stream), stage(st) {
    const int only = g_prof_only.load(), every = g_prof_every.load();
    on = g_prof_on.load() && (only < 0 || only == st);
    if (on && only == st && every > 1) on = (g_prof_tick.fetch_add(1) % (unsigned)every) == 0;
    if (on) { std::lock_guard<std::mutex> l(g_prof_mu); a = prof_event(); b = prof_event(); (void)hipEventRecord(a, s); }
  }
  ~StageTimer() {
    if (on) { (void)hipEventRecord(b, s); std::lock_guard<std::mutex> l(g_prof_mu); g_prof_recs.push_back({stage, a, b}); }
  }
};

static CamArgs make_cam(const float* view, const float* proj, const float* campos, int W, int H, float tan_fovx, float tan_fovy,
                        float kernel_size, float scale_modifier) {
  CamArgs c;
  c.view = view; c.proj = proj; c.campos = campos;
  c.focal_y = H / (2.0f * tan_fovy);  // rasterizer_impl.cu:288-289
  c.focal_x = W / (2.0f * tan_fovx);
  c.tan_fovx = tan_fovx; c.tan_fovy = tan_fovy; c.kernel_size = kernel_size; c.scale_modifier = scale_modifier;
  c.W = W; c.H = H; c.gx = (W + kTile - 1) / kTile; c.gy = (H + kTile - 1) / kTile;
  return c;
}

// Sub-tile entry streams (rg_streams.inc) or the tile-wide kernels?  Streams win while splats are small against a tile (the
// sub-lists then hold a fraction of the tile list each); for large splats every entry reaches every block, the sub-lists only
// multiply the list traffic and building them costs more than they save.  Measured on the MI355X (400k Gaussians at 1080p, depth mode;
// ms for lists + forward + backward, streams | tile-wide):
//     tiles per Gaussian R/P     3.8            9.6            21.6           48             98
//                                0.45 | 0.63    0.92 | 1.20    0.94 | 0.97    1.13 | 0.82    1.71 | 0.75
// -> on that family of scenes streams win below ~24 tiles per Gaussian, in every map mode (with the coord map an entry's accumulator
// record is two 64-B lines, which the stream backward updates with one atomic instruction each; round 5, same box: C2 with both maps
// 2.03 ms against 2.55 for the per-tile LDS merge of round 4 and 2.84 tile-wide; C4 4.11 against 4.66; profiles/r05_ab_linewise.txt).
// But tiles per Gaussian is the wrong statistic for a heavy-tailed scene: on C2H (synth_scene: a trained scene's shape -- 2 % of the
// splats span 16..240 tiles each and supply most of the instances, R/P = 13.5) the streams take 3.56 ms against 1.46 tile-wide: an
// instance of a large splat reaches all 8 blocks of its tile, so its work and its atomic line updates are multiplied by 8 instead of
// divided.  What decides is the size of the splat the average INSTANCE belongs to, S = sum t_i^2 / sum t_i over the tile counts t_i
// (the scan's two kernels add it up: per-block partial sums, then the last block's total -- no atomics).  On the sweep above S = 12 | 44 | 113 | 259 | 501; C2H: 645; C5: 634.
// -> streams while S < 112.  S of the previous forward at this (device, W, H) decides a speculative forward, the exact S an exact one;
// without S (RADEGS_PRIMS=rocprim) the old rule R < 24 P stands in.
constexpr float kStreamsMaxWeightedSize = 112.0f;
// Where an instance's 8-bit block mask travels through the tile sort: in the top byte of the VALUE next to a Gaussian index below 2^24,
// or -- scenes of 2^24 Gaussians and more -- in the top byte of a 32-bit tile KEY (the sort only looks at the low tile bits).
static bool mask_rides_in_key(const Switches& sw, int P) { return P >= (1 << kMaskShift) || sw.mask_in_key != 0; }
// The stream kernels address the 64-byte blend records with 32-bit byte offsets next to a scalar base: 2^26 Gaussians (the tile-wide
// kernels have no such limit and take over beyond it, whatever the switch says).
constexpr int kStreamsMaxGaussians = (1 << 26) - 1;
static bool use_streams(const Switches& sw, long long R_est, int P, float weighted_size) {
  if (P > kStreamsMaxGaussians) return false;
  if (sw.streams >= 0) return sw.streams != 0;
  if (R_est <= 0) return false;
  if (weighted_size > 0.0f) return weighted_size < kStreamsMaxWeightedSize;
  return R_est < 24ll * P;
}
// Which image-state buffers hold entry streams written by the forward: the backward may only replay them when the forward that
// filled THIS buffer produced them (the tile-wide backward is valid after either forward, so an unknown pointer falls back to it).
// A bounded map in least-recently-noted order: a C-ABI caller that never calls radegs_forget_image cannot grow it without limit, and
// an address that falls out merely costs its backward the faster formulation.  The device-side double check is the buffer's own
// stream_tag word: a stream backward that finds another value there raises the error flag below and returns without touching anything.
static std::mutex g_stream_mu;
static std::unordered_map<const void*, uint64_t> g_stream_images;   // address -> tick of its last forward
static uint64_t g_stream_tick = 0;
constexpr size_t kStreamImagesMax = 4096;
static void note_stream_image(const void* img, bool on) {
  std::lock_guard<std::mutex> l(g_stream_mu);
  if (!on) { g_stream_images.erase(img); return; }
  if (g_stream_images.size() >= kStreamImagesMax && g_stream_images.find(img) == g_stream_images.end()) {   // drop the oldest half
    std::vector<uint64_t> ticks;
    ticks.reserve(g_stream_images.size());
    for (auto& kv : g_stream_images) ticks.push_back(kv.second);
    std::nth_element(ticks.begin(), ticks.begin() + ticks.size() / 2, ticks.end());
    const uint64_t cut = ticks[ticks.size() / 2];
    for (auto it = g_stream_images.begin(); it != g_stream_images.end();) it = it->second < cut ? g_stream_images.erase(it) : std::next(it);
  }
  g_stream_images[img] = ++g_stream_tick;
}
static bool image_has_streams(const void* img) {
  std::lock_guard<std::mutex> l(g_stream_mu);
  return g_stream_images.find(img) != g_stream_images.end();
}

// Run-time flags as template arguments: f(std::true_type or std::false_type, ...), one instantiation per combination.
template <class F> static void dispatch(bool a, F&& f) { if (a) f(std::true_type()); else f(std::false_type()); }
template <class F> static void dispatch(bool coord, bool depth, F&& f) {   // the blend kernels' <COORD, DEPTH>
  dispatch(coord, [&](auto c) { dispatch(depth, [&](auto d) { f(c, d); }); });
}

// The Gaussian-side inputs shared by radegs_forward and radegs_integrate.
struct GaussIn {
  int P, D, M;
  const float *means3D, *scales, *rotations, *cov3D_precomp, *opacities, *shs, *colors_precomp;
  int* radii;
};
template <class Args> static GaussIn gauss_in(const Args* A) {
  return GaussIn{A->P, A->D, A->M, A->means3D, A->scales, A->rotations, A->cov3D_precomp, A->opacities, A->shs, A->colors_precomp, A->radii};
}
// The checks of the Gaussian-side inputs that radegs_forward, radegs_integrate and radegs_backward_from_sums share, in this order and
// with upstream's messages ("excatly" included).  `present`: the caller's required pointers are all there; `colors`: the call takes
// SHs or precomputed colours.
template <class Args> static int check_gaussians(const Args* A, bool present, bool colors) {
  if (!present) return fail(RADEGS_ERR_INVALID_ARG, "missing required tensor");
  if (colors && (A->shs == nullptr) == (A->colors_precomp == nullptr))
    return fail(RADEGS_ERR_INVALID_ARG, "Please provide excatly one of either SHs or precomputed colors!");
  if (((A->scales == nullptr) || (A->rotations == nullptr)) == (A->cov3D_precomp == nullptr))
    return fail(RADEGS_ERR_INVALID_ARG, "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!");
  return 0;
}

// ---- speculative binning --------------------------------------------------------------------------------------------------
// The reference sizes the binning buffer from num_rendered, which it reads back with a blocking copy in the middle of
// the forward (rasterizer_impl.cu:354): on this GPU that is an ~80 us bubble per call (sync + allocation + relaunch) in a
// 2 ms step.  After the first call on a device the previous value predicts the next one well (consecutive training views),
// so the buffers are allocated for a CAPACITY of 1.25x the (slowly decaying, 1/64 per call) running maximum before anything is
// launched, the binning kernels are launched for that capacity and read the real count on the device, and the host only looks
// at the count when everything else of the forward -- the blend included -- is queued.  If the prediction was too small the
// dropped instances are detected then and the forward is redone with the exact size.  RADEGS_SPECULATE=0 turns it off.
// The prediction is kept per (device, image size): a training loop that alternates resolutions (train / test cameras, multi-scale
// schedules) would otherwise ping-pong one hint between very different counts.
struct HintKey { int dev, W, H; bool operator==(const HintKey& o) const { return dev == o.dev && W == o.W && H == o.H; } };
struct HintKeyHash { size_t operator()(const HintKey& k) const { return ((size_t)k.dev * 1000003u + (size_t)k.W) * 1000003u + (size_t)k.H; } };
// What the previous forwards of a (device, W, H) needed: instances (num_rendered), chunks of entry-stream storage, the splat size S
// (use_streams), whether the depths of such a view once left the 3-pass sort's window, and whether its streams exceeded
// RADEGS_STREAMS_MAX_MB (the launcher then stops asking for them instead of redoing every forward).
// The "do not fit" verdict is not for ever (ADVICE r5): one oversized view -- a densification peak before pruning -- would otherwise keep
// this (device, W, H) on the slower tile-wide path for the rest of the run.  It holds for kNoFitForwards attempts, then the streams are
// tried again (and refused again for as long if the lists still exceed the budget).
constexpr uint32_t kNoFitForwards = 64;
struct History { uint32_t R = 0, chunks = 0; float weighted_size = 0.0f; uint32_t no_fit_left = 0; bool sort4 = false; };
static std::mutex g_hist_mu;
static std::unordered_map<HintKey, History, HintKeyHash> g_hist;
// The record as an attempt finds it; the attempt ticks the no-fit countdown (*no_fit: the streams stay refused this time).
static History history_begin(const HintKey& k, bool* no_fit) {
  std::lock_guard<std::mutex> l(g_hist_mu);
  auto it = g_hist.find(k);
  *no_fit = it != g_hist.end() && it->second.no_fit_left != 0u;
  if (*no_fit) it->second.no_fit_left--;
  return it == g_hist.end() ? History() : it->second;
}
template <class F> static void history_update(const HintKey& k, F&& f) {
  std::lock_guard<std::mutex> l(g_hist_mu);
  if (g_hist.size() > 1024 && g_hist.find(k) == g_hist.end()) g_hist.clear();
  f(g_hist[k]);
}
// Words of the mapped host block the kernels write directly (system-scope stores into pinned, coherent host memory).
enum { PIN_COUNT = 0,      // num_rendered of the forward in flight (emit_instances_kernel)
       PIN_KEY_OVERFLOW,   // a visible depth key outside the 3-pass sort's window (preprocess_fwd_kernel)
       PIN_SEQ,            // sequence number of the forward whose PIN_COUNT has landed: written AFTER the count with release order, so
                           // the host needs no event (a marker packet drains the queue: a 6-us bubble per forward in round 4's timeline)
       PIN_STREAM_ERR,     // a stream backward found an image buffer without entry streams (blend_bwd_streams_kernel)
       PIN_CHUNKS,         // chunks of entry-stream storage the forward's lists needed (block_lists_kernel's last list-building workgroup, before PIN_SEQ) ...
       PIN_CHUNK_OVERFLOW, // ... and whether they exceeded the capacity they were given
       PIN_SQ_LO, PIN_SQ_HI,   // sum over the Gaussians of (tiles touched)^2, 64 bits (emit_instances_kernel, with PIN_COUNT): use_streams()
       PIN_WORDS = 16 };
struct PinnedCount {
  volatile uint32_t* h = nullptr;   // [PIN_WORDS]
  uint32_t* d = nullptr;            // the same words as the device addresses them
  uint32_t seq = 0;                 // last sequence number handed to a forward
  bool ok() {
    if (!h) {
      void* p = nullptr;
      if (hipHostMalloc(&p, PIN_WORDS * sizeof(uint32_t), hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) p = nullptr;
      if (p) memset(p, 0, PIN_WORDS * sizeof(uint32_t));
      h = static_cast<volatile uint32_t*>(p);
      if (h && hipHostGetDevicePointer(reinterpret_cast<void**>(&d), p, 0) != hipSuccess) { (void)hipHostFree(p); h = nullptr; d = nullptr; }
    }
    return h && d;
  }
  uint32_t* dev() const { return d; }
};
// one per (host thread, device): the mapped word's device address belongs to the device that was current when it was obtained, and a
// thread may drive several GPUs (ADVICE r3)
static PinnedCount& pinned_for(int dev) {
  static thread_local PinnedCount per_dev[64];
  return per_dev[dev >= 0 && dev < 64 ? dev : 0];
}

// A stream backward that found an image buffer without entry streams raised PIN_STREAM_ERR (rg_streams.inc); the next call into the
// library on that thread and device reports it once.
static int check_stream_error(int dev) {
  if (dev < 0 || dev >= 64) return 0;
  PinnedCount& pin = pinned_for(dev);
  if (pin.h && pin.h[PIN_STREAM_ERR] != 0u) {
    pin.h[PIN_STREAM_ERR] = 0u;
    return fail(RADEGS_ERR_STATE, "an earlier radegs_backward was handed an image buffer that does not hold the entry streams of its forward "
                                  "(state buffer reused or overwritten between forward and backward); that call's gradients are invalid");
  }
  return 0;
}

static std::atomic<unsigned long long> g_spec_calls{0}, g_spec_misses{0};   // speculative forwards / those that had to be redone

// ---- one forward or integrate: attempts at the binning until one fits ---------------------------------------------------------
// How an attempt ended: its binning fitted; or the forward is redone with exact sizes (a capacity was too small); or with exact sizes
// and the 4-pass depth sort (a visible depth key left the 3-pass sort's window, so the order is not to be trusted).
enum Outcome { kFits = 0, kRedoExact, kRedo4Pass };

// What an attempt settles before its first launch.  The first attempt of a call is speculative where it can be (history, a mapped
// host block, no debug sync) and exact otherwise; a redo is exact, with the 4-pass sort after kRedo4Pass.
struct Plan {
  Switches sw;
  HintKey key{0, 0, 0};
  History hist;                 // the record of `key` as this attempt found it
  bool no_fit = false;          // entry streams refused at `key` this time (History::no_fit_left)
  bool speculative = false, hint_forced = false;   // hint_forced: the prediction is RADEGS_SPECULATE_HINT's (no R nor S is recorded)
  uint32_t hint = 0, cap = 0;   // predicted num_rendered; speculative: capacity of the instance arrays
  uint32_t seq = 0;             // speculative: what the device writes to PIN_SEQ once the counts have landed (0: exact)
  PinnedCount* pin = nullptr;   // the mapped host words of this thread and device, if it has them
  const PrimsCheck* prims = nullptr;   // RADEGS_PRIMS=rocprim: depth sort, scan and tile sort through the device library
  // depth sort: three 9-bit passes over (key - bits(0.2f)) instead of four 8-bit ones, valid while every visible z < 13 107 -- the
  // preprocess flags a key outside that window in a mapped host word (size_exact, finish_speculative look at it)
  bool sort27 = false;
  bool key16 = false;           // 16-bit tile keys (a third less sort traffic) wherever the tile id fits
  bool rect = false;            // packed tile rectangles (8 bits per field): gathered into depth order by the scan, read by the emission
  bool mask_in_key = false;     // with entry streams, the block mask rides in a 32-bit tile KEY (scenes of 2^24 Gaussians and more)
  bool sq_sum = false;          // the scan adds up S's numerator, sum over the Gaussians of (tiles touched)^2
  int tile_bits = 0;
};

struct Alloc {
  radegs_alloc_fn fn; void* user;
  void* operator()(size_t bytes) const { return fn(user, bytes); }
};
// One forward or integrate call: its inputs and allocators, and the state its attempts carve.
struct Binning {
  GaussIn G; CamArgs cam; bool coord = false;
  float4* inte_rec = nullptr;   // != nullptr: the INTE preprocess (integrate path), which also writes [P][8] floats there
  Alloc geom, bin, image;
  bool streams_allowed = false, dbg = false; hipStream_t stream = nullptr;
  GeomState gs; BinState bs; ImageState is;
  size_t chunk_cap = 0;         // with entry streams (is.blk_chunks != nullptr): chunks of list storage in the image state
  uint32_t R = 0;               // num_rendered, once the host knows it
};

static int plan_attempt(const Binning& B, Outcome prev, Plan& p) {
  p.sw = switches();
  if (p.sw.rocprim) {
    if (!prims_check().ok) return fail(RADEGS_ERR_INVALID_ARG, "RADEGS_PRIMS=rocprim: libradegs_prims_check.so (test-only) is not next to the library");
    p.prims = &prims_check();
  }
  int devid = 0;
  (void)hipGetDevice(&devid);
  p.key = HintKey{devid, B.cam.W, B.cam.H};
  p.hist = history_begin(p.key, &p.no_fit);
  p.hint_forced = p.sw.speculate_hint > 0;   // tests: force a (too small) prediction
  p.hint = p.hint_forced ? (uint32_t)p.sw.speculate_hint : p.hist.R;
  PinnedCount& pin = pinned_for(devid);
  if (devid < 64 && pin.ok()) p.pin = &pin;
  // the device library's primitives come plain: no speculation, rect gather, 16-bit keys, 27-bit sort or S statistic around them
  const bool own = p.prims == nullptr;
  p.speculative = prev == kFits && p.sw.speculate != 0 && p.hint > 0 && !B.dbg && own && p.pin;
  p.sort27 = own && p.pin && prev != kRedo4Pass && !p.hist.sort4;
  p.tile_bits = (int)higher_msb((uint32_t)(B.cam.gx * B.cam.gy));
  p.key16 = own && p.tile_bits <= 16;
  p.rect = own && B.cam.gx <= 255 && B.cam.gy <= 255;
  p.sq_sum = own;
  p.mask_in_key = mask_rides_in_key(p.sw, B.G.P);
  if (p.speculative) {
    p.cap = (uint32_t)std::min<uint64_t>((uint64_t)p.hint + p.hint / 4 + 4096, 0x7FFFFFFFull);
    p.seq = ++pin.seq;
  }
  return 0;
}

static int alloc_geometry(Binning& B, const Plan& p) {
  const size_t P = (size_t)B.G.P;
  size_t temp = std::max(sort_temp_bytes(P), scan_temp_bytes(P));
  if (p.prims) temp = std::max(temp, p.prims->temp_geom(P));
  void* ptr = B.geom(GeomState::carve(nullptr, P, B.coord, temp).total);
  if (!ptr) return fail(RADEGS_ERR_ALLOC, "geometry buffer allocation failed");
  B.gs = GeomState::carve(ptr, P, B.coord, temp);
  return 0;
}

// Image state for `capacity` instances; its tail holds the sub-tile entry streams when the call allows them and use_streams() says so
// (is.blk_chunks != nullptr afterwards).  With entry streams its tail holds `chunk_cap` chunks: what the previous forward at this
// (device, W, H) needed + 25 % when the overflow can be noticed without a stall (speculative attempt: finish_speculative), otherwise the
// capacity that cannot overflow (stream_chunk_capacity_safe); never more than RADEGS_STREAMS_MAX_MB -- a speculative attempt may try
// its luck inside that budget, an exact one then goes without streams.
static bool alloc_image(Binning& B, const Plan& p, size_t capacity, float weighted_size) {
  const Switches& sw = p.sw;
  const bool overflow_is_detected = p.speculative;
  bool streams = B.streams_allowed && use_streams(sw, (long long)capacity, B.G.P, weighted_size) && !(p.no_fit && sw.streams < 0);
  size_t chunk_cap = 0;
  if (streams) {
    const uint32_t hint = p.hist.chunks;
    const size_t safe = stream_chunk_capacity_safe(std::max<size_t>(capacity, 1), (size_t)(B.cam.gx * B.cam.gy));
    const size_t budget = sw.streams_max_bytes / (kChunkWords * sizeof(uint32_t));
    chunk_cap = (overflow_is_detected && hint) ? std::min(safe, (size_t)hint + hint / 4 + 4096) : safe;
    if (overflow_is_detected && sw.speculate_chunks > 0) chunk_cap = (size_t)sw.speculate_chunks;
    if (chunk_cap > budget) chunk_cap = overflow_is_detected ? budget : 0;
    if (chunk_cap > 0xFFFFFFF0ull) chunk_cap = 0xFFFFFFF0ull;   // chunk indices are 32-bit (0.8 TB of lists)
    streams = chunk_cap != 0;
  }
  const size_t W = (size_t)B.cam.W, H = (size_t)B.cam.H;
  void* ptr = B.image(ImageState::carve(nullptr, W, H, chunk_cap).total);
  if (!ptr && streams) {   // the stream-sized state did not fit: the tile-wide formulation needs none of it
    streams = false; chunk_cap = 0;
    ptr = B.image(ImageState::carve(nullptr, W, H, 0).total);
  }
  if (!ptr) return false;
  B.is = ImageState::carve(ptr, W, H, chunk_cap);
  B.chunk_cap = chunk_cap;
  if (!streams) B.is.blk_chunks = nullptr;
  note_stream_image(ptr, streams);
  g_last_forward_streams = streams ? 1 : 0;
  return true;
}

// Binning state and image state for `capacity` instances.
static int alloc_binning(Binning& B, const Plan& p, size_t capacity, float weighted_size) {
  size_t temp = sort_temp_bytes(capacity);
  if (p.prims) temp = std::max(temp, p.prims->temp_bin(capacity, p.tile_bits));
  void* ptr = B.bin(BinState::carve(nullptr, capacity, temp).total);
  if (!ptr) return fail(RADEGS_ERR_ALLOC, "binning buffer allocation failed");
  B.bs = BinState::carve(ptr, capacity, temp);
  if (!alloc_image(B, p, capacity, weighted_size)) return fail(RADEGS_ERR_ALLOC, "image buffer allocation failed");
  return 0;
}

// 1. per-Gaussian preprocess, 2. depth order of the Gaussians, 3. instance offsets in that order
static int queue_geometry(Binning& B, const Plan& p) {
  const GaussIn& G = B.G;
  const GeomState& gs = B.gs;
  hipStream_t stream = B.stream;
  if (p.sort27) p.pin->h[PIN_KEY_OVERFLOW] = 0u;
  {
    StageTimer tm(ST_PRE_FWD, stream);
    PreFwdArgs pa;
    pa.P = G.P; pa.D = G.D; pa.M = G.M;
    pa.means3D = G.means3D; pa.scales = G.scales; pa.rotations = G.rotations; pa.cov3D_precomp = G.cov3D_precomp;
    pa.opacities = G.opacities; pa.shs = G.shs; pa.colors_precomp = G.colors_precomp;
    pa.cam = B.cam; pa.write_b = B.coord ? 1 : 0;
    pa.radii = G.radii; pa.inte_rec = B.inte_rec; pa.splat_a = reinterpret_cast<float4*>(gs.splat_a); pa.splat_b = reinterpret_cast<float4*>(gs.splat_b);
    pa.tiles_touched = gs.tiles_touched; pa.depth_key = gs.depth_key; pa.clamped = gs.clamped; pa.rect = gs.rect;
    pa.key_overflow = p.sort27 ? p.pin->dev() + PIN_KEY_OVERFLOW : nullptr;
    dispatch(B.inte_rec != nullptr, [&](auto inte) { hipLaunchKernelGGL(preprocess_fwd_kernel<inte>, dim3((G.P + 255) / 256), dim3(256), 0, stream, pa); });
    RG_LAUNCH_CHECK("preprocess_fwd_kernel", B.dbg, stream);
  }
  const size_t P = (size_t)G.P;
  {
    StageTimer tm(ST_SORT_DEPTH, stream);
    if (p.prims) RG_HIP(p.prims->sort_by_depth(gs.temp, gs.temp_bytes, gs.depth_key, gs.depth_key_sorted, gs.idx_sorted, P, stream));
    else if (p.sort27) RG_HIP(radix_sort_pairs_u32_27(gs.temp, gs.temp_bytes, gs.depth_key, gs.depth_key_sorted, nullptr, gs.idx_sorted, P, kDepthKeyBase, stream));
    else RG_HIP(radix_sort_pairs_u32(gs.temp, gs.temp_bytes, gs.depth_key, gs.depth_key_sorted, nullptr, gs.idx_sorted, P, 32, stream));
  }
  {
    StageTimer tm(ST_SCAN, stream);
    if (p.prims) RG_HIP(p.prims->scan(gs.temp, gs.temp_bytes, gs.tiles_touched, gs.idx_sorted, gs.offsets, P, stream));
    else RG_HIP(inclusive_scan_gather_u32(gs.temp, gs.temp_bytes, p.rect ? gs.rect : gs.tiles_touched, gs.idx_sorted, gs.offsets, P, stream,
                                          p.rect ? gs.rect_sorted : nullptr, gs.tile_sq_sum));
  }
  return 0;
}

// 4. exact sizes: the one host sync of the reference's forward -- num_rendered sizes the binning buffer (rasterizer_impl.cu:354)
static int size_exact(Binning& B, const Plan& p, Outcome& out) {
  uint32_t R = 0;
  unsigned long long sq = 0ull;
  RG_HIP(hipMemcpyAsync(&R, B.gs.offsets + (B.G.P - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, B.stream));
  if (p.sq_sum) RG_HIP(hipMemcpyAsync(&sq, B.gs.tile_sq_sum, sizeof(sq), hipMemcpyDeviceToHost, B.stream));
  RG_HIP(hipStreamSynchronize(B.stream));
  if (p.sort27 && p.pin->h[PIN_KEY_OVERFLOW] != 0u) {
    history_update(p.key, [](History& h) { h.sort4 = true; });
    out = kRedo4Pass;
    return 0;
  }
  if (R > 0x7FFFFFFFu) return fail(RADEGS_ERR_INVALID_ARG, "num_rendered overflows int32");
  const float weighted_size = (R && p.sq_sum) ? (float)((double)sq / (double)R) : 0.0f;
  if (!p.hint_forced)
    history_update(p.key, [&](History& h) { h.R = std::max(R, p.hint - p.hint / 64); if (weighted_size > 0.0f) h.weighted_size = weighted_size; });
  B.R = R;
  return alloc_binning(B, p, R, weighted_size);
}

// 5. instances, 6. sorted by tile, 7. tile ranges: for the capacity of a speculative attempt (the real count is read on the device) or
// for the exact count
static int queue_instances(Binning& B, const Plan& p) {
  const GeomState& gs = B.gs; const BinState& bs = B.bs; const ImageState& is = B.is;
  hipStream_t stream = B.stream;
  if (!p.speculative && B.R == 0) {
    RG_HIP(hipMemsetAsync(is.ranges, 0, (size_t)(B.cam.gx * B.cam.gy) * 2 * sizeof(uint32_t), stream));
    RG_HIP(hipMemsetAsync(is.stream_tag, 0, 4 * sizeof(uint32_t), stream));
    return 0;
  }
  const int P = B.G.P;
  const uint32_t n = p.speculative ? p.cap : B.R;
  const uint32_t* n_dev = p.speculative ? gs.offsets + (P - 1) : nullptr;
  const bool streams = is.blk_chunks != nullptr;
  const bool mask_in_key = streams && p.mask_in_key;
  const bool key16 = p.key16 && !mask_in_key;
  {
    StageTimer tm(ST_EMIT, stream);
    // with entry streams every instance also learns which blocks of its tile it can reach (top byte of the value); the kernel also
    // clears the tile ranges and, speculative, mirrors num_rendered into the host's pinned words
    uint32_t* const count_mirror = p.speculative ? p.pin->dev() : nullptr;
    dispatch(streams, [&](auto masks) {
      hipLaunchKernelGGL(emit_instances_kernel<masks>, dim3((P + 255) / 256), dim3(256), 0, stream, P, gs.idx_sorted, gs.offsets,
                         gs.tiles_touched, reinterpret_cast<const float4*>(gs.splat_a), B.G.radii, p.rect ? gs.rect_sorted : nullptr,
                         B.cam.gx, B.cam.gy, bs.tile_keys, bs.point_list_unsorted, n, is.ranges, count_mirror, p.seq, is.stream_tag,
                         key16 ? 1 : 0, mask_in_key ? 1 : 0, gs.tile_sq_sum);
    });
    RG_LAUNCH_CHECK("emit_instances_kernel", B.dbg, stream);
  }
  {
    StageTimer tm(ST_SORT_TILE, stream);
    if (p.prims)
      RG_HIP(p.prims->sort_by_tile(bs.temp, bs.temp_bytes, bs.tile_keys, bs.tile_keys_sorted, bs.point_list_unsorted, bs.point_list, (size_t)n,
                                   p.tile_bits, stream));
    else if (key16)
      RG_HIP(radix_sort_pairs_u16(bs.temp, bs.temp_bytes, reinterpret_cast<const uint16_t*>(bs.tile_keys), reinterpret_cast<uint16_t*>(bs.tile_keys_sorted),
                                  bs.point_list_unsorted, bs.point_list, (size_t)n, p.tile_bits, stream, n_dev));
    else
      RG_HIP(radix_sort_pairs_u32(bs.temp, bs.temp_bytes, bs.tile_keys, bs.tile_keys_sorted, bs.point_list_unsorted, bs.point_list,
                                  (size_t)n, p.tile_bits, stream, n_dev));
  }
  {
    StageTimer tm(ST_RANGES, stream);
    if (key16)   // 8 keys per thread
      hipLaunchKernelGGL(tile_ranges_kernel<uint16_t>, dim3((n + 8 * kRangeThreads - 1) / (8 * kRangeThreads)), dim3(kRangeThreads), 0, stream,
                         (int)n, reinterpret_cast<const uint16_t*>(bs.tile_keys_sorted), reinterpret_cast<uint2*>(is.ranges), n_dev, 0xFFFFu, (int)n);
    else         // 4 keys per thread
      hipLaunchKernelGGL(tile_ranges_kernel<uint32_t>, dim3((n + 4 * kRangeThreads - 1) / (4 * kRangeThreads)), dim3(kRangeThreads), 0, stream,
                         (int)n, bs.tile_keys_sorted, reinterpret_cast<uint2*>(is.ranges), n_dev, mask_in_key ? kGidMask : 0xFFFFFFFFu, (int)n);
    RG_LAUNCH_CHECK("tile_ranges_kernel", B.dbg, stream);
  }
  return 0;
}

// 7b. sub-tile entry lists (rg_streams.inc) and 8. the blend of a forward
static int queue_blend(const Binning& B, const Plan& p, const RadegsFwdArgs* A) {
  const GeomState& gs = B.gs; const BinState& bs = B.bs; const ImageState& is = B.is; const CamArgs& cam = B.cam;
  hipStream_t stream = B.stream;
  const int ntiles = cam.gx * cam.gy;
  const bool streams = is.blk_chunks != nullptr;
  if (streams) {
    StageTimer tm(ST_BLOCK_LISTS, stream);
    uint32_t* const pin_words = p.speculative ? p.pin->dev() : nullptr;   // a speculative forward reports to the host's mapped words
    BlockListArgs la;
    la.ranges = reinterpret_cast<const uint2*>(is.ranges); la.point_list = bs.point_list; la.keys_sorted = bs.tile_keys_sorted;
    la.gx = cam.gx; la.ntiles = ntiles;
    la.blk_count = is.blk_count; la.blk_base = is.blk_base; la.blk_chunks = is.blk_chunks;
    la.wg_need = is.wg_need; la.stream_meta = is.stream_tag; la.chunk_capacity = (uint32_t)B.chunk_cap;
    // a grid that fills the chip once (8 workgroups of 4 waves per CU), a multiple of 8 so that tiles keep their XCD
    const int list_grid = std::min(ntiles, kListGridMax);
    // block_lists_kernel's FIRST workgroups sort the blocks of every 64-tile neighbourhood by list length (balance_blocks needs the counts
    // only): their number rounded up to a multiple of 8, so that a list-building workgroup runs on the XCD block_counts_kernel's ran on
    const int nblocks = ntiles * kBlocksPerTile;
    const int bal_groups = (((nblocks + kBalanceBlocks - 1) / kBalanceBlocks) + 7) & ~7;
    la.list_grid = list_grid; la.bal_groups = bal_groups; la.blk_order = is.blk_order;
    la.pin_chunks = pin_words ? pin_words + PIN_CHUNKS : nullptr; la.pin_seq = pin_words ? pin_words + PIN_SEQ : nullptr; la.seq = p.seq;
    dispatch(p.mask_in_key, [&](auto mask_in_key) {
      hipLaunchKernelGGL(block_counts_kernel<mask_in_key>, dim3(list_grid), dim3(kListThreads), 0, stream, la);
      hipLaunchKernelGGL(block_lists_kernel<mask_in_key>, dim3(bal_groups + list_grid), dim3(kListThreads), 0, stream, la);
    });
    RG_LAUNCH_CHECK("block_lists_kernel", B.dbg, stream);
  }
  {
    StageTimer tm(ST_BLEND_FWD, stream);
    BlendFwdArgs ba;
    ba.ranges = reinterpret_cast<const uint2*>(is.ranges); ba.point_list = bs.point_list;
    ba.splat_a = reinterpret_cast<const float4*>(gs.splat_a); ba.splat_b = reinterpret_cast<const float4*>(gs.splat_b);
    ba.W = cam.W; ba.H = cam.H; ba.gx = cam.gx; ba.ntiles = ntiles; ba.focal_x = cam.focal_x; ba.focal_y = cam.focal_y;
    ba.bg = A->background;
    ba.out_color = A->out_color; ba.out_coord = A->out_coord; ba.out_mcoord = A->out_mcoord; ba.out_depth = A->out_depth;
    ba.out_mdepth = A->out_mdepth; ba.out_alpha = A->out_alpha; ba.out_normal = A->out_normal;
    ba.n_contrib = is.n_contrib; ba.accum_coord = is.accum_coord; ba.accum_depth = is.accum_depth; ba.normal_length = is.normal_length;
    ba.blk_count = is.blk_count; ba.blk_base = is.blk_base; ba.blk_consumed = is.blk_consumed; ba.blk_chunks = is.blk_chunks; ba.blk_order = is.blk_order;
    const bool coord = A->require_coord != 0, depth = A->require_depth != 0;
    if (streams) dispatch(coord, depth, [&](auto c, auto d) { hipLaunchKernelGGL((blend_fwd_streams_kernel<c, d>), dim3(ntiles * 2), dim3(64), 0, stream, ba); });
    else dispatch(coord, depth, [&](auto c, auto d) {   // tile-wide: one wave per 16x8 strip, 2 pixels per lane (measured best on every BASELINE config)
      hipLaunchKernelGGL((blend_fwd_kernel<c, d, 2>), dim3(ntiles * 2), dim3(64), 0, stream, ba);
    });
    RG_LAUNCH_CHECK("blend_fwd_kernel", B.dbg, stream);
  }
  return 0;
}

static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  __asm__ __volatile__("yield");
#else
  std::atomic_signal_fence(std::memory_order_seq_cst);
#endif
}
// The host looks at the counts of a speculative attempt: records them and tells whether the predicted capacities held.
static int finish_speculative(Binning& B, const Plan& p, Outcome& out) {
  volatile uint32_t* const h = p.pin->h;
  // the count leaves the emission kernel early in the forward and everything else is queued behind it by now: normally it is there
  // already.  Poll the sequence word (written after the count, release order); a stream that does not deliver within ~2 s of polling is
  // synchronised the ordinary way so that a device error surfaces as an error code, not as a hang.
  for (uint32_t spins = 0; h[PIN_SEQ] != p.seq;) {
    if (++spins <= 4096u) { cpu_relax(); continue; }   // ~50 us of busy polling: the usual case ends here
    if (spins > 4096u + 40000u) {
      RG_HIP(hipStreamSynchronize(B.stream));
      if (h[PIN_SEQ] != p.seq) return fail(RADEGS_ERR_HIP, "num_rendered did not arrive from the device");
      break;
    }
    struct timespec ts = {0, 50000};
    nanosleep(&ts, nullptr);
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  const uint32_t R = h[PIN_COUNT];
  if (R > 0x7FFFFFFFu) return fail(RADEGS_ERR_INVALID_ARG, "num_rendered overflows int32");
  const uint64_t sq = (uint64_t)h[PIN_SQ_LO] | ((uint64_t)h[PIN_SQ_HI] << 32);
  const float weighted_size = R ? (float)((double)sq / (double)R) : 0.0f;
  if (!p.hint_forced)
    history_update(p.key, [&](History& r) { r.R = std::max(R, p.hint - p.hint / 64); if (weighted_size > 0.0f) r.weighted_size = weighted_size; });
  bool chunk_overflow = false;
  if (B.is.blk_chunks) {
    const uint32_t need = h[PIN_CHUNKS];
    chunk_overflow = h[PIN_CHUNK_OVERFLOW] != 0u || need > B.chunk_cap;
    // lists that do not even fit the configured budget: stop asking for streams at this (device, W, H)
    const bool no_fit = (size_t)need * kChunkWords * sizeof(uint32_t) > p.sw.streams_max_bytes;
    history_update(p.key, [&](History& r) { r.chunks = std::max(need, r.chunks - r.chunks / 64); r.no_fit_left = no_fit ? kNoFitForwards : 0u; });
  }
  B.R = R;
  g_spec_calls++;
  if (p.sort27 && h[PIN_KEY_OVERFLOW] != 0u) {
    history_update(p.key, [](History& r) { r.sort4 = true; });
    out = kRedo4Pass;
  } else {
    out = (R > p.cap || chunk_overflow) ? kRedoExact : kFits;
  }
  if (out != kFits) g_spec_misses++;
  return 0;
}

// Stages 1-7 (preprocess and binning) of a forward or integrate, and for a forward (A != nullptr) 7b-8 (lists and blend); returns
// num_rendered or < 0.  Each attempt is planned, allocates and queues the stages; a speculative one queues the blend too before the
// host looks at its counts.  An attempt that did not fit is redone from the start, once its work has drained.
static int bin_and_blend(Binning& B, const RadegsFwdArgs* A) {
  Outcome prev = kFits;
  for (;;) {
    Plan p;
    Outcome out = kFits;
    int rc = plan_attempt(B, prev, p);
    if (rc < 0) return rc;
    if ((rc = alloc_geometry(B, p)) < 0) return rc;
    if (p.speculative && (rc = alloc_binning(B, p, p.cap, p.hist.weighted_size)) < 0) return rc;   // before the first launch
    if ((rc = queue_geometry(B, p)) < 0) return rc;
    if (!p.speculative && (rc = size_exact(B, p, out)) < 0) return rc;
    if (out == kFits) {
      if ((rc = queue_instances(B, p)) < 0) return rc;
      if (A && (rc = queue_blend(B, p, A)) < 0) return rc;
      if (p.speculative && (rc = finish_speculative(B, p, out)) < 0) return rc;
      if (out == kFits) return (int)B.R;
    }
    if (p.speculative) RG_HIP(hipStreamSynchronize(B.stream));   // (an exact attempt has synchronised already)
    prev = out;
  }
}

}  // namespace rg

using namespace rg;

extern "C" {

const char* radegs_last_error(void) { return g_last_error.c_str(); }
void radegs_forget_image(const void* image_buffer) { note_stream_image(image_buffer, false); }
void radegs_reload_env(void) { std::lock_guard<std::mutex> l(g_sw_mu); switches_storage() = read_switches(); }
int radegs_last_forward_used_streams(void) { return g_last_forward_streams; }
const char* radegs_version(void) { return "radegs-hip 0.6.0 (gfx950)"; }

size_t radegs_geometry_bytes(int P, int require_coord) {
  return GeomState::carve(nullptr, (size_t)P, require_coord != 0, std::max(sort_temp_bytes((size_t)P), scan_temp_bytes((size_t)P))).total;
}
size_t radegs_image_bytes(int width, int height) { return ImageState::carve(nullptr, (size_t)width, (size_t)height).total; }
size_t radegs_binning_bytes(int R) { return BinState::carve(nullptr, (size_t)R, sort_temp_bytes((size_t)R)).total; }

int radegs_forward(const RadegsFwdArgs* A, radegs_alloc_fn geom_alloc, void* geom_user, radegs_alloc_fn binning_alloc,
                   void* binning_user, radegs_alloc_fn image_alloc, void* image_user, void* stream_v) {
  if (!A || !geom_alloc || !binning_alloc || !image_alloc) return fail(RADEGS_ERR_INVALID_ARG, "null argument");
  if (A->P < 0 || A->width <= 0 || A->height <= 0) return fail(RADEGS_ERR_INVALID_ARG, "bad sizes");
  if (A->P == 0) return 0;  // rasterize_points.cu:90: nothing is launched
  int rc = check_gaussians(A, A->means3D && A->opacities && A->viewmatrix && A->projmatrix && A->cam_pos && A->background && A->radii &&
                                  A->out_color && A->out_alpha, true);
  if (rc < 0) return rc;
  if (A->prefiltered) return fail(RADEGS_ERR_INVALID_ARG, "prefiltered=True is not supported (it selects the integrate path upstream)");
  if (A->shs && (A->D + 1) * (A->D + 1) > A->M) return fail(RADEGS_ERR_INVALID_ARG, "sh_degree needs more SH rows than provided");
  const bool coord = A->require_coord != 0, depth = A->require_depth != 0;
  if (coord && (!A->out_coord || !A->out_mcoord)) return fail(RADEGS_ERR_INVALID_ARG, "coord outputs missing");
  if (depth && (!A->out_depth || !A->out_mdepth)) return fail(RADEGS_ERR_INVALID_ARG, "depth outputs missing");
  if ((coord || depth) && !A->out_normal) return fail(RADEGS_ERR_INVALID_ARG, "normal output missing");
  int devid = 0;
  (void)hipGetDevice(&devid);
  if ((rc = check_stream_error(devid)) < 0) return rc;
  Binning B;
  B.G = gauss_in(A);
  B.cam = make_cam(A->viewmatrix, A->projmatrix, A->cam_pos, A->width, A->height, A->tan_fovx, A->tan_fovy, A->kernel_size, A->scale_modifier);
  B.coord = coord;
  B.geom = {geom_alloc, geom_user}; B.bin = {binning_alloc, binning_user}; B.image = {image_alloc, image_user};
  B.streams_allowed = true; B.dbg = A->debug != 0; B.stream = static_cast<hipStream_t>(stream_v);
  return bin_and_blend(B, A);
}

// ---- backward: the stages of Rasterizer::backward ----------------------------------------------------------------------------
// The scratch of radegs_backward_ordered, carved at 256-byte steps: one partial record per position of point_list, the positions sorted by
// Gaussian (keys and positions), the sort's temporary.
struct OrderedScratch {
  float* part = nullptr; uint32_t* keys = nullptr; uint32_t* pos = nullptr; void* sort_temp = nullptr; size_t part_bytes = 0, sort_bytes = 0, total = 0;
  static OrderedScratch carve(void* base, size_t R, bool coord) {
    OrderedScratch o;
    Carver c(base);
    o.part_bytes = R * (size_t)acc_record_floats(coord) * sizeof(float);
    o.sort_bytes = sort_temp_bytes(R);
    o.part = c.take<float>(R * (size_t)acc_record_floats(coord));
    o.keys = c.take<uint32_t>(R);
    o.pos = c.take<uint32_t>(R);
    o.sort_temp = c.take<char>(o.sort_bytes);
    o.total = c.off;
    return o;
  }
};

// One backward call: its arguments, the states of its forward, the per-Gaussian records and what the stages need to queue their work.
// radegs_backward_from_sums fills the per-Gaussian part only (A, cam, gs, acc, rec, stream, dbg).
struct Backward {
  const RadegsBwdArgs* A = nullptr;
  CamArgs cam;
  GeomState gs; BinState bs; ImageState is;
  float* acc = nullptr; int rec = 0;   // [P][rec] records: the accumulator, or the caller's sums (never written then)
  hipStream_t stream = nullptr;
  bool dbg = false, coord = false, depth = false;
  bool acc_reuse = false;              // the accumulator came all zeros and goes back so (RadegsBwdArgs::acc_reuse)
  int devid = 0;
  OrderedScratch os;                   // radegs_backward_ordered with R > 0; os.part == nullptr otherwise
  bool ordered() const { return os.part != nullptr; }
};

// The checks every backward entry point makes once its own pointers are there, in this order.  needs_state: a whole backward, which
// replays the forward's image and binning state and may hand back dL_drgb_clamped in place of dL_dsh (the factored exchange); the hook
// over caller-supplied sums reads the geometry state only and always returns dL_dsh.  Returns 1: go on; 0: P == 0, nothing is launched;
// < 0: the error.
static int check_backward_args(const RadegsBwdArgs* A, bool needs_state) {
  if (A->struct_size != sizeof(RadegsBwdArgs)) return fail(RADEGS_ERR_INVALID_ARG, "RadegsBwdArgs.struct_size does not match this library's include/radegs.h");
  if (A->P == 0) return 0;
  if (!A->geom_buffer || (needs_state && (!A->image_buffer || (A->R > 0 && !A->binning_buffer))))
    return fail(RADEGS_ERR_INVALID_ARG, "state buffers missing");
  if (!A->dL_dmean2D || !A->dL_dcolor || !A->dL_dopacity || !A->dL_dmean3D || !A->dL_dcov3D || !A->dL_dscale || !A->dL_drot)
    return fail(RADEGS_ERR_INVALID_ARG, "gradient outputs missing");
  if (A->shs && !A->dL_dsh && !(needs_state && A->dL_drgb_clamped)) return fail(RADEGS_ERR_INVALID_ARG, "dL_dsh missing");
  return 1;
}

// What has to be zero before the blend: the accumulator, unless its owner keeps it zero -- or, ordered, the partial records (the blend
// leaves out those of entries it skips; ordered_sums_kernel then writes every record of the accumulator).
static int queue_acc_zero(const Backward& B) {
  void* const what = B.ordered() ? static_cast<void*>(B.os.part) : (B.acc_reuse ? nullptr : static_cast<void*>(B.acc));
  if (!what) return 0;
  StageTimer tm(ST_ACC_ZERO, B.stream);
  RG_HIP(hipMemsetAsync(what, 0, B.ordered() ? B.os.part_bytes : (size_t)B.A->P * B.rec * sizeof(float), B.stream));
  return 0;
}

// The four formulations of the blend backward.  All leave the same record per Gaussian (raw moments in components 9..14, rg_streams.inc).
//   ordered   radegs_backward_ordered: the tile-wide kernel, one wave per tile, one partial record per list position
//   streams   replays the forward's entry streams -- only when the forward that filled THIS image buffer wrote them, and while the
//             accumulator fits the kernel's 32-bit byte offsets (33 M Gaussians with the coord map, 67 M without)
//   packed2   tile-wide, valid after either forward: one wave per 16x8 strip (2 pixels per lane)
//   packed4   tile-wide, one wave per tile (4 per lane) once every entry covers the tile anyway.  Measured on the MI355X: within 1 % of
//             packed2 either way up to 200 tiles per Gaussian on synthetic scenes, -8 % on C5 (4K, heavy overdraw: 4.41 against 4.80 ms);
//             never with the coord map (+5 %) -> from R >= 64 P on, without the coord map
enum class BlendBwd { ordered, streams, packed2, packed4 };
constexpr uint64_t kStreamBwdMaxAccBytes = 0xFFFFFFFFull;
static BlendBwd choose_blend_bwd(const Switches& sw, bool ordered, bool has_streams, int P, int R, bool coord) {
  if (ordered) return BlendBwd::ordered;
  const bool acc_fits = (uint64_t)P * (uint64_t)(acc_record_floats(coord) * sizeof(float)) <= kStreamBwdMaxAccBytes;
  if (has_streams && sw.streams_bwd && acc_fits) return BlendBwd::streams;
  if (sw.bwd_ppl == 2) return BlendBwd::packed2;
  if (sw.bwd_ppl == 4) return BlendBwd::packed4;
  return (!coord && (long long)R >= 64ll * P) ? BlendBwd::packed4 : BlendBwd::packed2;
}

// renderCUDA bwd (R > 0): the pixels' cotangents into per-Gaussian records -- the accumulator, or the ordered scratch's partial records
static int queue_blend_bwd(const Backward& B) {
  const RadegsBwdArgs* A = B.A;
  const GeomState& gs = B.gs; const BinState& bs = B.bs; const ImageState& is = B.is; const CamArgs& cam = B.cam;
  hipStream_t stream = B.stream;
  const int ntiles = cam.gx * cam.gy;
  StageTimer tm(ST_BLEND_BWD, stream);
  BlendBwdArgs ba;
  ba.ranges = reinterpret_cast<const uint2*>(is.ranges); ba.point_list = bs.point_list;
  ba.splat_a = reinterpret_cast<const float4*>(gs.splat_a); ba.splat_b = reinterpret_cast<const float4*>(gs.splat_b);
  ba.W = cam.W; ba.H = cam.H; ba.gx = cam.gx; ba.ntiles = ntiles; ba.focal_x = cam.focal_x; ba.focal_y = cam.focal_y;
  ba.bg = A->background; ba.alphas = A->alphas; ba.normalmap = A->normalmap;
  ba.n_contrib = is.n_contrib; ba.accum_coord = is.accum_coord; ba.accum_depth = is.accum_depth; ba.normal_length = is.normal_length;
  ba.dL_dpix = A->dL_dpix; ba.dL_dcoord = A->dL_dpix_coord; ba.dL_dmcoord = A->dL_dpix_mcoord; ba.dL_ddepth = A->dL_dpix_depth;
  ba.dL_dmdepth = A->dL_dpix_mdepth; ba.dL_dalpha = A->dL_dalphas; ba.dL_dnormal = A->dL_dpix_normal;
  ba.acc = B.ordered() ? B.os.part : B.acc; ba.P = A->P;
  ba.blk_base = is.blk_base; ba.blk_consumed = is.blk_consumed; ba.blk_chunks = is.blk_chunks; ba.blk_order = is.blk_order; ba.stream_tag = is.stream_tag;
  {
    PinnedCount& pin = pinned_for(B.devid);
    ba.stream_err = (B.devid < 64 && pin.ok()) ? pin.dev() + PIN_STREAM_ERR : nullptr;
  }
  if (!ba.alphas || !ba.dL_dpix || !ba.dL_dalpha) return fail(RADEGS_ERR_INVALID_ARG, "pixel gradients missing");
  if (B.coord && (!ba.dL_dcoord || !ba.dL_dmcoord)) return fail(RADEGS_ERR_INVALID_ARG, "coord gradients missing");
  if (B.depth && (!ba.dL_ddepth || !ba.dL_dmdepth)) return fail(RADEGS_ERR_INVALID_ARG, "depth gradients missing");
  if ((B.coord || B.depth) && (!ba.dL_dnormal || !ba.normalmap)) return fail(RADEGS_ERR_INVALID_ARG, "normal gradients missing");
  const BlendBwd how = choose_blend_bwd(switches(), B.ordered(), image_has_streams(A->image_buffer), A->P, A->R, B.coord);
  dispatch(B.coord, B.depth, [&](auto c, auto d) {
    switch (how) {
      case BlendBwd::ordered: hipLaunchKernelGGL((blend_bwd_ordered_kernel<c, d>), dim3(ntiles), dim3(64), 0, stream, ba); break;
      case BlendBwd::streams: hipLaunchKernelGGL((blend_bwd_streams_kernel<c, d>), dim3(ntiles * 2), dim3(64), 0, stream, ba); break;
      case BlendBwd::packed2: hipLaunchKernelGGL((blend_bwd_packed_kernel<c, d, 2>), dim3(ntiles * 2), dim3(64), 0, stream, ba); break;
      case BlendBwd::packed4: hipLaunchKernelGGL((blend_bwd_packed_kernel<c, d, 4>), dim3(ntiles), dim3(64), 0, stream, ba); break;
    }
  });
  RG_LAUNCH_CHECK("blend_bwd_kernel", B.dbg, stream);
  return 0;
}

// Ordered only: the partial records into the accumulator in a fixed order -- a stable sort of (point_list[r], r), after which every
// Gaussian's positions are consecutive and ascending, then one sum per Gaussian and component over its run
static int queue_ordered_sums(const Backward& B) {
  const int P = B.A->P, R = B.A->R;
  const OrderedScratch& os = B.os;
  {
    StageTimer tm(ST_ORDERED_SORT, B.stream);
    int bits = 1;
    while (bits < 32 && (1ull << bits) < (unsigned long long)P) bits++;
    RG_HIP(radix_sort_pairs_u32(os.sort_temp, os.sort_bytes, B.bs.point_list, os.keys, nullptr, os.pos, (size_t)R, bits, B.stream));
  }
  StageTimer tm(ST_ORDERED_SUMS, B.stream);
  const unsigned nb = (unsigned)(((size_t)P * B.rec + 255) / 256);
  if (B.coord) hipLaunchKernelGGL((ordered_sums_kernel<32>), dim3(nb), dim3(256), 0, B.stream, P, (uint32_t)R, os.keys, os.pos, os.part, B.acc);
  else hipLaunchKernelGGL((ordered_sums_kernel<16>), dim3(nb), dim3(256), 0, B.stream, P, (uint32_t)R, os.keys, os.pos, os.part, B.acc);
  RG_LAUNCH_CHECK("ordered_sums_kernel", B.dbg, B.stream);
  return 0;
}

// How a launch of preprocess_bwd_kernel treats the records (PreBwdArgs::keep, rezero, drgb_done)
enum PreBwdFlags : unsigned { kKeepSums = 1u, kRezero = 2u, kDrgbDone = 4u };

// The drgb_ready hand-off (include/radegs.h): the rows the factored exchange all-gathers leave one kernel early, and the caller is told
static int queue_drgb(const Backward& B, unsigned& flags) {
  const RadegsBwdArgs* A = B.A;
  if (!A->dL_drgb_clamped || !A->drgb_ready) return 0;
  hipLaunchKernelGGL(drgb_clamped_kernel, dim3((A->P + 255) / 256), dim3(256), 0, B.stream, A->P, A->radii, B.gs.clamped, B.acc, B.rec, A->dL_drgb_clamped);
  RG_LAUNCH_CHECK("drgb_clamped_kernel", B.dbg, B.stream);
  A->drgb_ready(A->drgb_ready_user);
  flags |= kDrgbDone;
  return 0;
}

// The per-Gaussian backward (computeCov2DCUDA + preprocessCUDA bwd, backward.cu:145-628) over the records B.acc
static int queue_preprocess_bwd(const Backward& B, RecordKind kind, unsigned flags) {
  const RadegsBwdArgs* A = B.A;
  StageTimer tm(ST_PRE_BWD, B.stream);
  const int P = A->P;
  PreBwdArgs pa;
  pa.P = P; pa.D = A->D; pa.M = A->M;
  pa.means3D = A->means3D; pa.scales = A->scales; pa.rotations = A->rotations; pa.cov3D_precomp = A->cov3D_precomp; pa.shs = A->shs;
  pa.radii = A->radii; pa.splat_a = reinterpret_cast<const float4*>(B.gs.splat_a); pa.clamped = B.gs.clamped; pa.acc = B.acc; pa.rec = B.rec;
  pa.cam = B.cam;
  pa.dL_dmean2D = A->dL_dmean2D; pa.dL_dcolor = A->dL_dcolor; pa.dL_dopacity = A->dL_dopacity; pa.dL_dmean3D = A->dL_dmean3D;
  pa.dL_dcov3D = A->dL_dcov3D; pa.dL_dsh = A->shs ? A->dL_dsh : nullptr; pa.dL_dscale = A->dL_dscale; pa.dL_drot = A->dL_drot;
  pa.dL_drgb_clamped = A->dL_drgb_clamped;
  pa.opacity_grad_intended = A->opacity_grad_intended;
  pa.kind = kind;
  pa.keep = (flags & kKeepSums) ? 1 : 0; pa.rezero = (flags & kRezero) ? 1 : 0; pa.drgb_done = (flags & kDrgbDone) ? 1 : 0;
  {  // 16-byte slab moves where shape and alignment allow (SH degree 3: M = 16; also M = 4); any other shape or a tensor off a 16-byte boundary takes the word loop
    const int rowf = A->M * 3;
    const bool aligned = (reinterpret_cast<uintptr_t>(pa.shs) & 15u) == 0 && (reinterpret_cast<uintptr_t>(pa.dL_dsh) & 15u) == 0;
    pa.vec_slab = (pa.shs && rowf % 4 == 0 && rowf <= 4 * kSlabVecs && aligned) ? 1 : 0;
  }
  const size_t sh_lds = pa.shs ? (size_t)kPreBwdThreads * (A->M * 3 + 1) * sizeof(float) : 0;
  const int nblocks = (P + kPreBwdThreads - 1) / kPreBwdThreads;
  // RadegsBwdArgs::grad_chunks: several launches over consecutive ranges of Gaussians, the caller told after each one (its all-reduce of
  // the finished rows then runs under the launches that follow)
  const int chunks = (A->grad_chunks > 1 && A->grads_ready) ? std::min(A->grad_chunks, nblocks) : 1;
  const int per = (nblocks + chunks - 1) / chunks;
  for (int c = 0; c * per < nblocks; c++) {
    const int nb = std::min(per, nblocks - c * per);
    pa.first_block = c * per;
    hipLaunchKernelGGL(preprocess_bwd_kernel, dim3(nb), dim3(kPreBwdThreads), sh_lds, B.stream, pa);
    RG_LAUNCH_CHECK("preprocess_bwd_kernel", B.dbg, B.stream);
    if (chunks > 1) {
      const int first = c * per * kPreBwdThreads;
      A->grads_ready(A->grads_ready_user, first, std::min(nb * kPreBwdThreads, P - first));
    }
  }
  return 0;
}

// radegs_backward (ordered = false) and radegs_backward_ordered (ordered = true): they differ in how the blend backward's wave totals
// reach the per-Gaussian records, nowhere else.
static int backward_impl(const RadegsBwdArgs* A, radegs_alloc_fn accum_alloc, void* accum_user, bool ordered, void* scratch, size_t scratch_bytes,
                         void* stream_v) {
  if (!A || !accum_alloc) return fail(RADEGS_ERR_INVALID_ARG, "null argument");
  int rc = check_backward_args(A, true);
  if (rc <= 0) return rc;
  Backward B;
  B.A = A; B.stream = static_cast<hipStream_t>(stream_v);
  B.dbg = A->debug != 0; B.coord = A->require_coord != 0; B.depth = A->require_depth != 0;
  const int P = A->P, R = A->R;
  if (ordered && R > 0) {
    if (!scratch) return fail(RADEGS_ERR_INVALID_ARG, "radegs_backward_ordered: scratch is NULL with R > 0");
    B.os = OrderedScratch::carve(scratch, (size_t)R, B.coord);
    if (scratch_bytes < B.os.total) return fail(RADEGS_ERR_INVALID_ARG, "radegs_backward_ordered: scratch smaller than radegs_backward_ordered_scratch_bytes(P, R, require_coord)");
  }
  (void)hipGetDevice(&B.devid);
  if ((rc = check_stream_error(B.devid)) < 0) return rc;
  B.cam = make_cam(A->viewmatrix, A->projmatrix, A->cam_pos, A->width, A->height, A->tan_fovx, A->tan_fovy, A->kernel_size, A->scale_modifier);
  B.gs = GeomState::carve(A->geom_buffer, (size_t)P, B.coord, 0);
  B.bs = BinState::carve(A->binning_buffer, (size_t)R, 0);
  B.is = ImageState::carve(A->image_buffer, (size_t)A->width, (size_t)A->height);
  B.rec = acc_record_floats(B.coord);
  B.acc = static_cast<float*>(accum_alloc(accum_user, (size_t)P * B.rec * sizeof(float)));
  if (!B.acc) return fail(RADEGS_ERR_ALLOC, "accumulator allocation failed");
  B.acc_reuse = A->acc_reuse != 0 && !A->keep_sums;   // the caller's scratch is zero and wants to stay so (include/radegs.h)

  if ((rc = queue_acc_zero(B)) < 0) return rc;
  if (R > 0 && (rc = queue_blend_bwd(B)) < 0) return rc;
  if (B.ordered() && (rc = queue_ordered_sums(B)) < 0) return rc;
  // a blend leaves raw moments; without one (R == 0) the records are the zeros they started as
  const RecordKind kind = R > 0 ? RecordKind::raw_moments : RecordKind::blend_sums;
  unsigned flags = (B.acc_reuse ? kRezero : 0u) | ((R > 0 && A->keep_sums) ? kKeepSums : 0u);
  if ((rc = queue_drgb(B, flags)) < 0) return rc;
  return queue_preprocess_bwd(B, kind, flags);
}

int radegs_backward(const RadegsBwdArgs* A, radegs_alloc_fn accum_alloc, void* accum_user, void* stream_v) {
  return backward_impl(A, accum_alloc, accum_user, false, nullptr, 0, stream_v);
}

size_t radegs_backward_ordered_scratch_bytes(int /*P*/, int R, int require_coord) {
  return OrderedScratch::carve(nullptr, (size_t)(R > 0 ? R : 0), require_coord != 0).total;
}

int radegs_backward_ordered(const RadegsBwdArgs* A, radegs_alloc_fn accum_alloc, void* accum_user, void* scratch, size_t scratch_bytes,
                            void* stream_v) {
  return backward_impl(A, accum_alloc, accum_user, true, scratch, scratch_bytes, stream_v);
}

// The per-Gaussian half alone, over the caller's sums, with the hand-off hooks of radegs_backward (tests reach the separate
// dL_drgb_clamped kernel and the chunked launches this way)
int radegs_backward_from_sums(const RadegsBwdArgs* A, const float* sums, void* stream_v) {
  if (!A || !sums) return fail(RADEGS_ERR_INVALID_ARG, "null argument");
  int rc = check_backward_args(A, false);
  if (rc <= 0) return rc;
  if ((rc = check_gaussians(A, A->radii && A->means3D && A->viewmatrix && A->projmatrix && A->cam_pos, false)) < 0) return rc;
  if (reinterpret_cast<uintptr_t>(sums) & 15u) return fail(RADEGS_ERR_INVALID_ARG, "sums must be 16-byte aligned");
  Backward B;
  B.A = A; B.stream = static_cast<hipStream_t>(stream_v);
  B.dbg = A->debug != 0; B.coord = A->require_coord != 0;
  B.cam = make_cam(A->viewmatrix, A->projmatrix, A->cam_pos, A->width, A->height, A->tan_fovx, A->tan_fovy, A->kernel_size, A->scale_modifier);
  B.gs = GeomState::carve(A->geom_buffer, (size_t)A->P, B.coord, 0);
  B.rec = acc_record_floats(B.coord);
  B.acc = const_cast<float*>(sums);   // read only: neither kKeepSums nor kRezero
  unsigned flags = 0;
  if ((rc = queue_drgb(B, flags)) < 0) return rc;
  return queue_preprocess_bwd(B, RecordKind::reference_sums, flags);
}

// The query points of radegs_integrate: project, count per pixel, scan, scatter (a counting sort on the pixel index).  Also clears the
// image state's two n_contrib planes (integrate_kernel writes plane 0 only).
static int queue_points(const RadegsIntegrateArgs* A, const CamArgs& cam, const PointState& ps, uint32_t* n_contrib, bool dbg, hipStream_t stream) {
  const int PN = A->PN, W = A->width, H = A->height;
  const size_t HW = (size_t)W * H;
  RG_HIP(hipMemsetAsync(ps.pix_count, 0, HW * sizeof(uint32_t), stream));
  RG_HIP(hipMemsetAsync(n_contrib, 0, 2 * HW * sizeof(uint32_t), stream));
  PointsPreArgs pp;
  pp.PN = PN; pp.points3D = A->points3D; pp.view = A->viewmatrix; pp.focal_x = cam.focal_x; pp.focal_y = cam.focal_y; pp.W = W; pp.H = H;
  pp.p2d = reinterpret_cast<float2*>(ps.p2d); pp.pdepth = ps.pdepth; pp.ppix = ps.ppix; pp.pix_count = ps.pix_count;
  pp.out_alpha_integrated = A->out_alpha_integrated; pp.out_color_integrated = A->out_color_integrated;
  pp.out_coordinate2d = A->out_coordinate2d; pp.out_sdf = A->out_sdf;
  hipLaunchKernelGGL(points_preprocess_kernel, dim3((PN + 255) / 256), dim3(256), 0, stream, pp);
  RG_LAUNCH_CHECK("points_preprocess_kernel", dbg, stream);
  RG_HIP(inclusive_scan_gather_u32(ps.temp, ps.temp_bytes, ps.pix_count, nullptr, ps.pix_incl, HW, stream));
  hipLaunchKernelGGL(points_scatter_kernel, dim3((PN + 255) / 256), dim3(256), 0, stream, PN, ps.ppix, ps.pix_count, ps.pix_incl,
                     ps.pt_sorted);
  RG_LAUNCH_CHECK("points_scatter_kernel", dbg, stream);
  return 0;
}

int radegs_integrate(const RadegsIntegrateArgs* A, radegs_alloc_fn geom_alloc, void* geom_user, radegs_alloc_fn binning_alloc,
                     void* binning_user, radegs_alloc_fn image_alloc, void* image_user, radegs_alloc_fn point_alloc, void* point_user,
                     void* stream_v) {
  if (!A || !geom_alloc || !binning_alloc || !image_alloc || !point_alloc) return fail(RADEGS_ERR_INVALID_ARG, "null argument");
  if (A->P < 0 || A->PN < 0 || A->width <= 0 || A->height <= 0) return fail(RADEGS_ERR_INVALID_ARG, "bad sizes");
  if (!A->out_color || (A->PN > 0 && (!A->out_alpha_integrated || !A->out_color_integrated || !A->out_coordinate2d || !A->out_sdf)) ||
      (A->P > 0 && !A->radii))
    return fail(RADEGS_ERR_INVALID_ARG, "missing output tensor");
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  const bool dbg = A->debug != 0;
  const int P = A->P, PN = A->PN, W = A->width, H = A->height;
  const size_t HW = (size_t)W * H;
  RG_HIP(hipMemsetAsync(A->out_color, 0, 9 * HW * sizeof(float), stream));
  if (P > 0) RG_HIP(hipMemsetAsync(A->radii, 0, (size_t)P * sizeof(int), stream));
  if (P == 0 || PN == 0) {  // rasterize_points.cu:330: nothing is launched; outputs keep their initial values
    if (PN > 0) {
      PointsPreArgs pp{};
      pp.PN = PN; pp.out_alpha_integrated = A->out_alpha_integrated; pp.out_color_integrated = A->out_color_integrated;
      pp.out_coordinate2d = A->out_coordinate2d; pp.out_sdf = A->out_sdf;
      hipLaunchKernelGGL(points_init_kernel, dim3((PN + 255) / 256), dim3(256), 0, stream, pp);
      RG_LAUNCH_CHECK("points_init_kernel", dbg, stream);
    }
    return 0;
  }
  const int rc = check_gaussians(A, A->means3D && A->opacities && A->viewmatrix && A->projmatrix && A->cam_pos && A->background && A->points3D,
                                 true);
  if (rc < 0) return rc;
  if (A->shs && (A->D + 1) * (A->D + 1) > A->M) return fail(RADEGS_ERR_INVALID_ARG, "sh_degree needs more SH rows than provided");
  const CamArgs cam = make_cam(A->viewmatrix, A->projmatrix, A->cam_pos, W, H, A->tan_fovx, A->tan_fovy, A->kernel_size, A->scale_modifier);
  const int ntiles = cam.gx * cam.gy;
  const size_t ptemp = scan_temp_bytes(HW);
  const size_t pbytes = PointState::carve(nullptr, (size_t)P, (size_t)PN, HW, ptemp).total;
  void* pptr = point_alloc(point_user, pbytes);
  if (!pptr) return fail(RADEGS_ERR_ALLOC, "point buffer allocation failed");
  PointState ps = PointState::carve(pptr, (size_t)P, (size_t)PN, HW, ptemp);

  Binning B;
  B.G = gauss_in(A); B.cam = cam; B.inte_rec = reinterpret_cast<float4*>(ps.inte_rec);
  B.geom = {geom_alloc, geom_user}; B.bin = {binning_alloc, binning_user}; B.image = {image_alloc, image_user};
  B.dbg = dbg; B.stream = stream;
  const int R = bin_and_blend(B, nullptr);
  if (R < 0) return R;
  const GeomState& gs = B.gs;
  const BinState& bs = B.bs;
  const ImageState& is = B.is;

  const int rq = queue_points(A, cam, ps, is.n_contrib, dbg, stream);
  if (rq < 0) return rq;
  {
    IntegrateArgs ia;
    ia.ranges = reinterpret_cast<const uint2*>(is.ranges); ia.point_list = bs.point_list;
    ia.splat_a = reinterpret_cast<const float4*>(gs.splat_a); ia.inte_rec = reinterpret_cast<const float4*>(ps.inte_rec);
    ia.W = W; ia.H = H; ia.gx = cam.gx; ia.bg = A->background;
    ia.pix_incl = ps.pix_incl; ia.pt_sorted = ps.pt_sorted; ia.p2d = reinterpret_cast<const float2*>(ps.p2d); ia.pdepth = ps.pdepth;
    ia.out9 = A->out_color; ia.final_T = ps.final_T; ia.n_contrib = is.n_contrib;
    ia.out_alpha_integrated = A->out_alpha_integrated; ia.out_color_integrated = A->out_color_integrated;
    ia.out_coordinate2d = A->out_coordinate2d; ia.out_sdf = A->out_sdf;
    hipLaunchKernelGGL(integrate_kernel, dim3(ntiles * 4), dim3(64), 0, stream, ia);
    RG_LAUNCH_CHECK("integrate_kernel", dbg, stream);
  }
  return R;
}

int radegs_sh_grad_from_views(int P, int D, int M, int nviews, const float* means3D, const float* campos, const float* drgb_clamped,
                              float scale, float* dL_dsh, void* stream_v) {
  if (P < 0 || nviews < 0 || D < 0 || D > 3 || M < (D + 1) * (D + 1)) return fail(RADEGS_ERR_INVALID_ARG, "bad sizes");
  if (P == 0) return 0;
  if (!means3D || !dL_dsh || (nviews > 0 && (!campos || !drgb_clamped))) return fail(RADEGS_ERR_INVALID_ARG, "null argument");
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  const size_t lds = (size_t)kPreBwdThreads * (M * 3 + 1) * sizeof(float);
  hipLaunchKernelGGL(sh_grad_from_views_kernel, dim3((P + kPreBwdThreads - 1) / kPreBwdThreads), dim3(kPreBwdThreads), lds, stream, P, D, M,
                     nviews, means3D, campos, drgb_clamped, scale, dL_dsh);
  RG_LAUNCH_CHECK("sh_grad_from_views_kernel", false, stream);
  return 0;
}

int radegs_mark_visible(int P, const float* means3D, const float* viewmatrix, const float* /*projmatrix*/, unsigned char* present,
                        void* stream_v) {
  if (P < 0) return fail(RADEGS_ERR_INVALID_ARG, "bad P");
  if (P == 0) return 0;
  if (!means3D || !viewmatrix || !present) return fail(RADEGS_ERR_INVALID_ARG, "null argument");
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  hipLaunchKernelGGL(mark_visible_kernel, dim3((P + 255) / 256), dim3(256), 0, stream, P, means3D, viewmatrix, present);
  RG_LAUNCH_CHECK("mark_visible_kernel", false, stream);
  return 0;
}

void radegs_binning_stats(unsigned long long* speculative_calls, unsigned long long* misses, int reset) {
  if (speculative_calls) *speculative_calls = g_spec_calls.load();
  if (misses) *misses = g_spec_misses.load();
  if (reset) { g_spec_calls = 0; g_spec_misses = 0; }
}

void radegs_profile_enable(int on) {
  std::lock_guard<std::mutex> l(g_prof_mu);
  g_prof_on = on != 0;
}
void radegs_profile_select(int stage) {
  std::lock_guard<std::mutex> l(g_prof_mu);
  g_prof_only = (stage >= 0 && stage < ST_COUNT) ? stage : -1;
}
void radegs_profile_stride(int every) {
  std::lock_guard<std::mutex> l(g_prof_mu);
  g_prof_every = every > 1 ? every : 1;
  g_prof_tick = 0;
}
int radegs_profile_num_stages(void) { return ST_COUNT; }
const char* radegs_profile_stage_name(int i) { return (i >= 0 && i < ST_COUNT) ? kStageNames[i] : ""; }
int radegs_profile_collect(float* ms_total, int* count, int n) {
  std::lock_guard<std::mutex> l(g_prof_mu);
  for (int i = 0; i < n; i++) { ms_total[i] = 0.f; count[i] = 0; }
  for (auto& r : g_prof_recs) {
    float ms = 0.f;
    hipError_t e = hipEventSynchronize(r.b);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, r.a, r.b);
    if (e == hipSuccess && r.stage < n) { ms_total[r.stage] += ms; count[r.stage]++; }
    g_prof_pool.push_back(r.a);
    g_prof_pool.push_back(r.b);
  }
  g_prof_recs.clear();
  return 0;
}

long long radegs_debug_export(const char* name, int P, int R, int width, int height, int require_coord, const void* geom_buffer,
                              const void* binning_buffer, const void* image_buffer, void* dst, size_t dst_bytes, void* stream_v) {
  if (!name || !dst) return fail(RADEGS_ERR_INVALID_ARG, "null argument");
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  const bool coord = require_coord != 0;
  GeomState gs = GeomState::carve(const_cast<void*>(geom_buffer), (size_t)P, coord, 0);
  BinState bs = BinState::carve(const_cast<void*>(binning_buffer), (size_t)R, 0);
  ImageState is = ImageState::carve(const_cast<void*>(image_buffer), (size_t)width, (size_t)height);
  const size_t tiles = (size_t)((width + 15) / 16) * ((height + 15) / 16), N = (size_t)width * height;
  const void* src = nullptr;
  size_t bytes = 0;
  const std::string n(name);
  if (n == "point_list") { src = bs.point_list; bytes = (size_t)R * 4; }
  else if (n == "ranges") { src = is.ranges; bytes = tiles * 8; }
  else if (n == "n_contrib") { src = is.n_contrib; bytes = N * 8; }
  else if (n == "tiles_touched") { src = gs.tiles_touched; bytes = (size_t)P * 4; }
  else if (n == "splat_a") { src = gs.splat_a; bytes = (size_t)P * 64; }
  else if (n == "splat_b") { src = gs.splat_b; bytes = coord ? (size_t)P * 48 : 0; }
  else if (n == "clamped") { src = gs.clamped; bytes = (size_t)P; }
  else if (n == "depth_key") { src = gs.depth_key; bytes = (size_t)P * 4; }
  else if (n == "blk_count") { src = is.blk_count; bytes = tiles * kBlocksPerTile * 4; }        // entry streams (valid after a stream forward)
  else if (n == "blk_consumed") { src = is.blk_consumed; bytes = tiles * kBlocksPerTile * 4; }
  else if (n == "blk_base") { src = is.blk_base; bytes = tiles * kBlocksPerTile * 4; }
  else if (n == "blk_order") { src = is.blk_order; bytes = tiles * kBlocksPerTile * 4; }
  else if (n == "stream_meta") { src = is.stream_tag; bytes = 16; }
  // the last array of the image state: its base does not depend on the capacity the forward allocated, and this function cannot know that
  // capacity -- the caller asks for stream_meta[1] * 48 words and answers for the buffer's size itself (radegs_image_bytes(w, h) - 256 + those)
  else if (n == "blk_chunks") { src = is.blk_chunks; bytes = dst_bytes; }
  else if (n == "tile_keys_sorted") { src = bs.tile_keys_sorted; bytes = (size_t)R * 4; }
  else if (n == "rect") { src = gs.rect; bytes = (size_t)P * 4; }
  else return fail(RADEGS_ERR_INVALID_ARG, "unknown array name");
  if (bytes > dst_bytes) return fail(RADEGS_ERR_INVALID_ARG, "destination too small");
  if (bytes == 0) return 0;
  if (!src) return fail(RADEGS_ERR_INVALID_ARG, "state buffer missing");
  RG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream));
  return (long long)bytes;
}

size_t radegs_point_bytes(int P, int PN, int width, int height) {
  const size_t HW = (size_t)width * height;
  return PointState::carve(nullptr, (size_t)P, (size_t)PN, HW, scan_temp_bytes(HW)).total;
}

long long radegs_debug_export_points(const char* name, int P, int PN, int width, int height, const void* point_buffer, void* dst,
                                     size_t dst_bytes, void* stream_v) {
  if (!name || !dst) return fail(RADEGS_ERR_INVALID_ARG, "null argument");
  if (P < 0 || PN < 0 || width <= 0 || height <= 0) return fail(RADEGS_ERR_INVALID_ARG, "bad sizes");
  hipStream_t stream = static_cast<hipStream_t>(stream_v);
  const size_t N = (size_t)width * height;
  PointState ps = PointState::carve(const_cast<void*>(point_buffer), (size_t)P, (size_t)PN, N, scan_temp_bytes(N));
  const void* src = nullptr;
  size_t bytes = 0;
  const std::string n(name);
  if (n == "inte_rec") { src = ps.inte_rec; bytes = (size_t)P * 32; }
  else if (n == "p2d") { src = ps.p2d; bytes = (size_t)PN * 8; }
  else if (n == "pdepth") { src = ps.pdepth; bytes = (size_t)PN * 4; }
  else if (n == "ppix") { src = ps.ppix; bytes = (size_t)PN * 4; }
  else if (n == "pt_sorted") { src = ps.pt_sorted; bytes = (size_t)PN * 4; }
  else if (n == "pix_count") { src = ps.pix_count; bytes = N * 4; }
  else if (n == "pix_incl") { src = ps.pix_incl; bytes = N * 4; }
  else if (n == "final_T") { src = ps.final_T; bytes = N * 4; }
  else return fail(RADEGS_ERR_INVALID_ARG, "unknown array name");
  if (bytes > dst_bytes) return fail(RADEGS_ERR_INVALID_ARG, "destination too small");
  if (bytes == 0) return 0;
  if (!point_buffer) return fail(RADEGS_ERR_INVALID_ARG, "state buffer missing");
  RG_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream));
  return (long long)bytes;
}

}  // extern "C"
