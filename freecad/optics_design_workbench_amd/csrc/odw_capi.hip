// odw_capi.hip -- C-ABI (include/odw_trace.h) over the gfx950 kernels.
//
// Host side of the native library: device context, scene/source upload into
// the HBM layouts of odw_device.h, inverse-CDF guide tables, the choice of a
// launch's kernel, launches on a private HIP stream, HIP-event timing, result
// fetch.  A scene's host tables, boxes, grid and trees are computed without a
// context (odw_build.h); upload_accel() here puts them on the device.  No
// torch types anywhere: plain pointers and sizes.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <atomic>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <new>
#include <thread>
#include <string>
#include <utility>
#include <vector>

#include "odw_kernels.hip"
#include "odw_grid.hip"
#include "odw_mesh.hip"
#include "odw_build.h"

using namespace odw;

namespace {

constexpr int kGuide = 1 << 16;
// Hit-list slots a wave reserves per atomic, and the smallest list that gets the room for it.
// Atomics on one address complete at about one per 3.6 ns on this chip whatever the number
// of waves, so a launch's length is bounded below by its atomic count: GettingStarted with a reservation per wave and
// recording step takes 0.23 / 0.66 ms for 1e6 / 3e6 rays, with blocks of 512 slots 0.16 / 0.34 (128: 0.19 / 0.45,
// 256: 0.17 / 0.36, 1024: 0.17 / 0.35, 4096: 0.33 / 0.68 -- the unused slots a wave tags at its end); at 1e8 rays
// 128: 10.7 ms, 256: 6.41, 512: 6.10, 1024: 6.06, 2048: 6.04, 4096: 6.13 (profiles/r03/r03q_hit_blocks.log).
constexpr uint32_t kHitBlock = 512;
constexpr uint64_t kHitBlockMinRows = 1ull << 16;
// room a list of `capacity` rows needs for reservations of `block` slots by `waves` waves: < 64 unused slots per
// block change, and the last block of every wave
static inline uint64_t hit_block_room(uint64_t capacity, uint64_t waves, uint64_t block) { return capacity * 64 / block + 64 + waves * block; }
constexpr int kPhiGuide = 1 << 8;        // azimuth table of a source (~1e2 knots)
constexpr int kSurfaceGuide = 1 << 10;  // per row of a surface sampler (tables of ~1e3 knots)
// Analytic scenes of up to this many primitives take the flat kernels (brute force over the primitives, scalar
// loads, one box test each).  Measured against the grid kernel's generic variant, which such scenes took above 16
// primitives until round 2: lens trains of 19 / 25 / 37 / 61 primitives 1.63e9 / 1.10e9 / 6.1e8 / 2.75e8 rays/s flat
// against 6.4e8 / 5.1e8 / 3.5e8 / 1.95e8 on the grid; random crowded scenes of 19 - 30 primitives 2 - 3.6 x faster
// (scripts/bench_lens_train.py, scripts/bench_crowded.py).  ODW_BVH_THRESHOLD (read when a context is created)
// overrides it: the tests keep the grid kernel's generic variant covered with 16.
constexpr int kBvhThreshold = 64;

std::string g_error;

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
};

}  // namespace

struct odw_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  void* up_pin = nullptr;                  // page-locked arena small uploads are staged in (upload())
  size_t up_off = 0;
  bool up_unstaged = false;                // an upload since the last wait was copied from the caller's memory
  int n_cu = 256;
  std::string err;

  HostScene hs;                            // host tables of the uploaded scene, needed for lazy (re)builds (odw_build.h)
  // scene-compiled flat kernel (odw_spec.hip)
  int compile_mode = 0;                    // ODW_COMPILE_*: sticky, applies to every scene uploaded later too
  bool spec_dirty = true;                  // scene / limits changed since the last binding attempt
  uint64_t source_key = 0;                 // structure of the table source the context holds (odw_spec.hip: spec_source_key), or 0
  uint64_t spec_source_key = 0;            // the same of the source the bound kernel is compiled against, 0: source-free
  hipFunction_t spec_fn = nullptr;         // bound kernel (owned by the process-wide cache), or null
  bool spec_lean = false, spec_stoch = false;
  // the bound kernel's value image (odw_build.h: SpecLayout; odw_spec.hip: spec_launch builds it at every launch)
  SpecLayout spec_layout;
  std::vector<double> spec_image_now, spec_image_host;   // this launch's image; the one in spec_image (images beyond the arguments)
  std::vector<char> spec_args;
  DevBuf spec_image;
  size_t batch_img_off = 0;                // doubles from a batch block's start to its image (0: the batch has none)
  // ODW_COMPILE_AUTO: the scene's kernel is not there yet (not hot enough, or being compiled)
  bool spec_pending = false;
  std::string spec_key;
  uint64_t spec_hot_rays = 50000000;       // rays traced with a structure on generic kernels (process-wide count) after
                                           // which its compilation starts (ODW_SPEC_HOT_RAYS at odw_create)
  double spec_seconds = 0;                 // compile time of the bound kernel (0: it came from a cache)
  int spec_cache_hit = 0;                  // 0 compiled now, 1 process cache, 2 disk cache
  bool have_scene = false, have_source = false, have_limits = false;
  bool bvh_dirty = true;
  int flat_limit = kBvhThreshold;          // most primitives the flat kernels take (ODW_BVH_THRESHOLD at odw_create)

  DevBuf prim_f64, prim_hdr, prim_i32, cond_i32, group_f64, group_i32, group_gdir, seq_mask;
  DevBuf bvh_nodes, bvh_prims, tri_nrm, asph;
  DevBuf bvh_leaf, bvh_wide;                         // leaf records and eight-wide tree of the mesh kernel (odw_mesh.hip)
  DevBuf grid_bounds, grid_cells, grid_items, dbg;   // rectilinear grid of big analytic scenes (odw_grid.hip)
  DevBuf phi_tab, t_tab, t_guide, phi_guide, d_source, d_det;
  DeviceSource h_source;
  DeviceDetector h_det;
  DevBuf hits, hit_count, chunk_counter;
  // ONE block holds what ranks sum: [kResultsHead words: the ODW_CNT_COUNT counters, padded] [n_bins histogram words]
  // [power_on: n_bins words of the power plane] [band_n: K * n_bins band counts] [band_n and power_on: K * n_bins band power]
  // -- a multi-GPU job reduces it with a single collective (odw_device_results); `counters` and `hist` are views into it
  DevBuf results, hist, counters;
  DevBuf segs, seg_count;                  // RecordRays segment list
  uint64_t seg_capacity = 0;
  DevBuf ray_o, ray_d, ray_p, ray_aos, samp_t, samp_phi;
  DevBuf sort_keys[2], sort_vals[2], sort_tmp, sorted_rows;
  // post-hoc binning of the rows in HBM (odw_posthoc.hip): the selection = sort_vals[1][0 .. ph_n)
  DevBuf ph_sel_entering, ph_flags, ph_x, ph_y, ph_sorted, ph_small, ph_part, ph_edges, ph_edges_b, ph_counts, ph_sel_hist;
  DevBuf ph_accel;                                   // tables of the polar binning (odw_posthoc.hip: PhbBinAccel)
  DevBuf ph_wl;                                      // wavelength table of a band binning (odw_hits_bin_bands, table mode)
  DevBuf ph_bitmap, ph_before, ph_row_of;            // ordered selection without a sort (odw_posthoc.hip: ph_mark_kernel)
  uint64_t alt_hit_ray_end = 0;    // the same for the list odw_swap_hit_lists has put aside
  uint64_t hit_ray_end = 0;        // ray indices of the rows in the hit list lie below this (0: list empty; 1 << 48: unknown)
  uint64_t hit_ray_begin = 0, alt_hit_ray_begin = 0;   // ... and at or above this (meaningful while hit_ray_end is a real bound)
  uint64_t ph_n = 0, ph_n_entering = 0;
  int ph_group = -1;
  bool ph_valid = false, ph_projected = false, ph_entering_built = false;
  std::vector<double> ph_moment_sums;      // per-block moment sums + centre of the current selection's points (odw_hits_project, odw_hits_moments)
  unsigned ph_moment_grid = 0;             // 0: none
  // stochastic surfaces: one table set per sampler, descriptor block, (group, kind) -> index
  struct SurfaceBufs { DevBuf phi_tab, t_tab, t_guide, atom_mass; };
  std::vector<SurfaceBufs> surf_bufs;
  DevBuf d_samplers, d_group_sampler;
  int n_samplers = 0;
  uint64_t surface_seed = 0;
  // surface source (emitter) tables + the explicit-ray staging of its launches
  DevBuf em_prim_f64, em_prim_i32, em_cond, em_face_i32, em_face_cdf, em_t_tab, em_t_guide, em_o, em_d, em_tri_nrm;
  DeviceEmitter h_emitter;
  bool emitter_active = false;   // the most recently uploaded source is a surface source
  uint64_t hit_capacity = 0, n_bins = 0;   // hit_capacity: rows the caller asked for
  bool power_on = false;                   // odw_enable_power_histogram: n_bins words of hit weights directly behind the histogram
  int band_n = 0;                          // odw_set_detector_bands: edges (K + 1; 0: no bands) -- K count planes behind the power
  double band_edges[ODW_BAND_MAX + 1] = {};//   plane's place, then with power_on K power planes
  DevBuf d_band_edges;
  uint64_t band_k() const { return band_n ? (uint64_t)band_n - 1 : 0; }
  // words behind the counters: (1 + P)(1 + K) planes of n_bins
  uint64_t plane_words() const { return n_bins * (power_on ? 2 : 1) * (1 + band_k()); }
  uint64_t hit_slots = 0;                  // rows allocated (capacity + slack for block reservations)
  // batch launches (odw_upload_scene_batch / odw_trace_batch): the value tables of batch_n scenes of one structure side by
  // side, one segment of the batch's hit list and one pair of counters per scene.  odw_batch_select makes a segment the
  // context's hit list (ctx->hits / hit_count become views; the context's own list waits in own_*)
  DevBuf batch_values, batch_hits, batch_hit_count, batch_rays_buf;
  int batch_n = 0;                         // scenes of the uploaded batch (0: none)
  size_t batch_prims = 0;                  // primitives per scene of that batch
  bool batch_launch = false;               // launch_trace: this launch is a batch
  uint64_t batch_stride = 0;               // doubles per scene block
  uint64_t batch_seg_slots = 0, batch_seg_capacity = 0, batch_rays = 0, batch_first = 0;
  int batch_traced = 0;                    // scenes of the last odw_trace_batch
  bool batch_rows_ok = false;              // its segments hold rows: the launch recorded hits and was issued without error
  bool batch_marked = false;               // ... whose rows noted their slots in phb_row_of while they were recorded
  bool batch_pts = false;                  // ... and their points in phb_pts (the chain's projection reads those)
  int batch_selected = -1;
  std::string batch_spec_text;             // the structure all scenes of the batch share (compiled kernels)
  hipFunction_t spec_batch_fn = nullptr;   // the scene-compiled kernel's BATCH variant (bound on the first batch launch)
  bool spec_batch_failed = false;          // ... could not be built for the bound structure: generic kernels for its batches
  hipFunction_t spec_power_fn = nullptr;   // ... and its POWER variant (the detector's power plane; bound on the first weighted launch)
  bool spec_power_failed = false;          // ... was asked for and is not to be asked for again for this binding (could not be built)
  const std::atomic<bool>* spec_power_wait = nullptr;   // ODW_COMPILE_AUTO: "done" of the variant's compilation under way (the job
                                           // stays in the process-wide table): weighted launches look at this flag only
  DevBuf own_hits, own_hit_count;
  uint64_t own_capacity = 0, own_slots = 0, own_ray_begin = 0, own_ray_end = 0;
  // a run's rows kept in HBM beyond the launches that recorded them (odw_archive_append / odw_archive_select)
  DevBuf archive, archive_count;
  uint64_t archive_slots = 0, archive_unused = 0, archive_ray_begin = 0, archive_ray_end = 0;
  bool archive_selected = false;
  // post-hoc binning of all segments at once (odw_batch_hits_*, odw_posthoc.hip): per-scene slices of these
  DevBuf phb_row_of, phb_words, phb_sel, phb_small, phb_rows, phb_x, phb_y, phb_part, phb_sel_hist, phb_cand, phb_counts;
  DevBuf phb_scenes, phb_hist, phb_planes, phb_strides, phb_origins, phb_accel, phb_pts;   // device-resident state of the chain (odw_posthoc_batch.hip)
  void* phb_pin_p = nullptr;               // page-locked block the chain's results arrive in
  size_t phb_pin_bytes = 0;
  hipEvent_t phb_ev = nullptr;             // end of the piece enqueued last (odw_batch_hits_begin / _measure)
  int phb_stage = 0, phb_S = 0;            // 1 begin enqueued, 2 sampled, 3 measure enqueued, 4 measured
  uint64_t phb_cap = 0, phb_nbins = 0, phb_keep = 0;
  size_t phb_part_stride = 0;
  std::vector<double> phb_edges_host;      // the edges on the device (uploaded when they change)
  int phb_edges_na = 0, phb_edges_nb = 0, phb_edges_polar = -1;
  std::vector<uint64_t> phb_used, phb_n, phb_leaving;
  std::vector<int32_t> phb_ordered;
  std::vector<char> phb_on;
  uint64_t phb_xy_stride = 0;
  int phb_group = -1;
  bool phb_valid = false, phb_projected = false;
  // second hit list (odw_swap_hit_lists): while one is traced into, the other is copied to the host
  // on a stream of its own
  DevBuf alt_hits, alt_hit_count;
  uint64_t alt_capacity = 0, alt_slots = 0;
  hipStream_t copy_stream = nullptr;
  hipEvent_t alt_ready = nullptr;          // recorded on the trace stream when the list was put aside
  bool swapping = false;                   // lists are swapped: appends stay dense (no block reservations)

  TraceParams P;
  odw_detector_desc det_desc;

  // dispersion of the scene's groups (odw_set_dispersion) and spectrum of the point source (odw_set_spectrum)
  bool disp_on = false;
  int32_t disp_kind[ODW_MAX_GROUPS] = {};
  double disp_coef[ODW_MAX_GROUPS * ODW_DISP_COEFS] = {};
  std::vector<double> base_ior;            // the groups' constants as uploaded (hs.group_f64[4 g] holds the folded values)
  bool fold_dirty = false;                 // dispersion or scene changed since the fold
  double fold_wl = 0;                      // wavelength the table words of dispersive groups were folded at
  DevBuf d_disp_kind, d_disp_coef, spec_tab, ray_wl, wl_rays, wl_out;
  int spec_n = 0, spec_mode = 0;           // the bound spectrum (0 knots: none)
  double spec_lo = 0, spec_hi = 0;         // its ends (nm)
  hipFunction_t spec_chroma_fn[2] = {nullptr, nullptr};   // the compiled kernel's variants for spectral launches: without / with the power plane
  bool spec_chroma_failed = false;         // ... could not be built for this binding: spectral launches walk the tree
  hipFunction_t spec_bands_fn[2] = {nullptr, nullptr};    // ... and their BANDS variants (band planes): without / with the power plane
  bool spec_bands_failed = false;
  SpecLayout spec_chroma_layout;           // ... and their value image (the plain one + the dispersion coefficients)
  DevBuf chroma_nodes, chroma_prims;       // the binary tree spectral launches walk in a scene that has none of its own
  int chroma_n_nodes = 0;                  // 0: to be built
  // Fresnel modes of the scene's groups (odw_set_fresnel); launches with one set walk the same tree where the scene has none
  bool fresnel_on = false, fresnel_split = false;
  int32_t fresnel_mode[ODW_MAX_GROUPS] = {};
  DevBuf d_fresnel_mode, fr_in, fr_out;
  hipFunction_t spec_fresnel_fn[2] = {nullptr, nullptr};  // the compiled kernel's variants for such launches: without / with the power plane
  bool spec_fresnel_failed = false;        // ... could not be built for this binding: they walk the tree
  SpecLayout spec_fresnel_layout;          // ... and their value image (the plain one; with a coating set, + the layers)
  // thin-film coatings of the groups (odw_set_coating): layers per group and their (index, thickness_nm) pairs
  bool coat_on = false;
  int32_t coat_n[ODW_MAX_GROUPS] = {};
  double coat[ODW_MAX_GROUPS * ODW_COAT_LAYERS * 2] = {};
  DevBuf d_coat_n, d_coat, coat_layers;

  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> free_events;
  double timing_ms = 0;
  uint64_t timing_launches = 0;
};

namespace {

int fail(odw_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  g_error = msg;
  return code;
}

#define HIPCHK(ctx, call)                                                              \
  do {                                                                                 \
    hipError_t e_ = (call);                                                            \
    if (e_ != hipSuccess)                                                              \
      return fail(ctx, ODW_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

int ensure(odw_ctx* ctx, DevBuf& b, size_t bytes) {
  if (bytes == 0) bytes = 16;
  if (b.bytes >= bytes && b.p) return ODW_OK;
  if (b.p) HIPCHK(ctx, hipFree(b.p));
  b.p = nullptr;
  b.bytes = 0;
  HIPCHK(ctx, hipMalloc(&b.p, bytes));
  b.bytes = bytes;
  return ODW_OK;
}

// Host to device on the context's stream.  Small tables (a scene's, a batch's: a few KB) travel through a page-locked
// arena of the context and are NOT waited for: a copy from pageable memory blocks the caller until it has run, and in a
// sweep it runs behind whatever other contexts have queued on the copy path -- up to a launch's length (10 ms stalls in
// the launch of a group, measured).  The caller's array may go away at once either way; upload_done() is the wait for
// copies that did not fit the arena.
constexpr size_t kUploadArena = 4u << 20, kUploadStaged = 512u << 10;
int upload(odw_ctx* ctx, DevBuf& b, const void* src, size_t bytes) {
  int rc = ensure(ctx, b, bytes);
  if (rc) return rc;
  if (!bytes) return ODW_OK;
  if (bytes <= kUploadStaged) {
    if (!ctx->up_pin) {
      if (hipHostMalloc(&ctx->up_pin, kUploadArena, hipHostMallocDefault) != hipSuccess) { ctx->up_pin = nullptr; (void)hipGetLastError(); }
      ctx->up_off = 0;
    }
    if (ctx->up_pin) {
      const size_t need = (bytes + 63) & ~(size_t)63;
      if (ctx->up_off + need > kUploadArena) {             // the arena comes round: what lies in it must have been copied
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        ctx->up_off = 0;
      }
      char* at = (char*)ctx->up_pin + ctx->up_off;
      std::memcpy(at, src, bytes);
      ctx->up_off += need;
      HIPCHK(ctx, hipMemcpyAsync(b.p, at, bytes, hipMemcpyHostToDevice, ctx->stream));
      return ODW_OK;
    }
  }
  HIPCHK(ctx, hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  ctx->up_unstaged = true;
  return ODW_OK;
}
// after a series of uploads from arrays that are about to go away: waits only if one of them was copied in place
int upload_done(odw_ctx* ctx) {
  if (ctx->up_unstaged) {
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->up_unstaged = false;
  }
  return ODW_OK;
}

void release(DevBuf& b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.bytes = 0;
}

constexpr size_t kResultsHead = 16;      // words in front of the histogram (128 B: the bins keep their alignment)
static_assert(ODW_CNT_COUNT <= kResultsHead, "counters must fit the head of the results block");

// the results block for n_words words behind the counters (a histogram of that many bins, or a histogram and its power
// plane); the counters and the first keep_words of those words survive a reallocation
int ensure_results(odw_ctx* ctx, uint64_t n_words, uint64_t keep_words = 0);
// ctx->hits / hit_count are views of a batch segment (odw_batch_select): give the context its own list back
void batch_unselect(odw_ctx* ctx);
// room for the post-hoc chain of a batch (odw_posthoc_batch.hip)
int phb_reserve(odw_ctx* ctx, int S, uint64_t rays_per_scene, uint64_t slots);

// ---- the scene's structures: built on the host (odw_build.h), uploaded here -------------------
// (read at every build: the tests that hold the two kernels, and the tree with and without cones, against each other)
BuildOptions build_options() {
  BuildOptions o;
  o.mesh_kernel = !(getenv("ODW_MESH_KERNEL") && getenv("ODW_MESH_KERNEL")[0] == '0');
  o.cones = !(getenv("ODW_MESH_CONES") && getenv("ODW_MESH_CONES")[0] == '0');
  o.cone_stats = getenv("ODW_MESH_CONE_STATS") != nullptr;
  return o;
}

// The headers and flag words of ctx->hs (compute_boxes has set ODW_FLAG_ISOLATED in them) and the tables of A into
// the context's buffers, their addresses into P.scene / P.grid.  Tables above kUploadStaged are copied in place and
// asynchronously: upload_done() below is what lets the caller drop A (and change ctx->hs) as soon as this returns.
int upload_accel(odw_ctx* ctx, const SceneAccel& A) {
  const HostScene& hs = ctx->hs;
  const bool grid = A.grid.nx > 0, tree = !A.nodes.empty(), wide = !A.leaf_recs.empty();
  const struct { bool on; DevBuf* buf; const void* src; size_t bytes; } tables[] = {
      {true, &ctx->prim_hdr, hs.prim_hdr.data(), hs.prim_hdr.size() * sizeof(double)},
      {hs.n_prims > 0, &ctx->prim_i32, hs.prim_i32.data(), hs.prim_i32.size() * sizeof(int32_t)},
      {grid, &ctx->grid_bounds, A.planes.data(), A.planes.size() * sizeof(double)},
      {grid, &ctx->grid_cells, A.cells.data(), A.cells.size() * sizeof(uint32_t)},
      {grid, &ctx->grid_items, A.items(), A.item_bytes()},
      {tree, &ctx->bvh_nodes, A.nodes.data(), A.nodes.size() * sizeof(BvhNode)},
      {tree, &ctx->bvh_prims, A.order.data(), A.order.size() * sizeof(int)},
      {wide, &ctx->bvh_leaf, A.leaf_recs.data(), A.leaf_recs.size() * sizeof(float)},
      {wide, &ctx->bvh_wide, A.wide_nodes.data(), A.wide_nodes.size() * sizeof(uint32_t)}};
  int rc = ODW_OK;
  for (const auto& t : tables)
    if (t.on && !rc) rc = upload(ctx, *t.buf, t.src, t.bytes);
  const int rc_done = upload_done(ctx);        // (also after a failed upload: an earlier one may still be reading A)
  DeviceScene& S = ctx->P.scene;
  DeviceGrid& G = ctx->P.grid;
  std::memset(&G, 0, sizeof G);
  S.n_nodes = 0;
  S.bvh_leaf = nullptr;
  S.bvh_wide = nullptr;
  if (rc || rc_done) return rc ? rc : rc_done;
  S.prim_hdr = (const double*)ctx->prim_hdr.p;
  if (grid) {
    G = A.grid;
    G.bounds = (const double*)ctx->grid_bounds.p;
    G.cells = (const uint32_t*)ctx->grid_cells.p;
    G.items = ctx->grid_items.p;
  }
  if (tree) {
    S.bvh_nodes = (const float*)ctx->bvh_nodes.p;
    S.bvh_prims = (const int32_t*)ctx->bvh_prims.p;
    S.n_nodes = (int)A.nodes.size();
  }
  if (wide) {
    S.bvh_leaf = (const float*)ctx->bvh_leaf.p;
    S.bvh_wide = (const uint32_t*)ctx->bvh_wide.p;
    for (int a = 0; a < 3; ++a) { S.wide_lo[a] = A.wide_lo[a]; S.wide_hi[a] = A.wide_hi[a]; }
  }
  return ODW_OK;
}

// boxes, headers and structures of the uploaded scene for the limits in force (first launch, odw_compile_scene,
// odw_upload_scene_batch)
int build_bvh(odw_ctx* ctx) {
  ctx->bvh_dirty = false;
  ctx->spec_dirty = true;
  ctx->chroma_n_nodes = 0;
  std::vector<Box> boxes;
  compute_boxes(ctx->hs, ctx->P.lim.dist_tol, boxes);
  SceneAccel A;
  std::string err;
  // (a tree the kernels' stack cannot hold leaves A empty: the headers still go up, so that what the context holds is a
  //  consistent scene without structures, and the launch answers with the builder's error)
  const int rc_build = build_accel(ctx->hs, std::move(boxes), ctx->P.lim.dist_tol, ctx->flat_limit, build_options(), A, err);
  const int rc = upload_accel(ctx, A);
  return rc_build ? fail(ctx, rc_build, err) : rc;
}


// ---- device-side ordering of the hit list (odw_fetch_hits) -----------------
__global__ void hit_keys_kernel(const odw_hit* __restrict__ hits, uint64_t n, uint64_t sentinel, uint64_t* __restrict__ keys,
                                uint32_t* __restrict__ vals) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const uint64_t tag = hits[i].tag;
    keys[i] = tag == ODW_TAG_UNUSED ? sentinel : ODW_HIT_RAY(tag);   // unused slots sort behind every ray
    vals[i] = (uint32_t)i;
  }
}

__global__ void seg_keys_kernel(const odw_segment* __restrict__ segs, uint64_t n, uint64_t* __restrict__ keys,
                                uint32_t* __restrict__ vals) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const uint64_t tag = segs[i].tag;
    keys[i] = (ODW_SEG_RAY(tag) << 12) | ODW_SEG_ORDINAL(tag);    // 52 bits
    vals[i] = (uint32_t)i;
  }
}

// four lanes move one 64-byte row (16 B each): coalesced reads of the index
// list, 64-B gathers, fully coalesced writes
__global__ void hit_gather_kernel(const odw_hit* __restrict__ hits, const uint32_t* __restrict__ order,
                                  uint64_t n, odw_hit* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t row = t >> 2;
  if (row < n) {
    const double2* src = reinterpret_cast<const double2*>(hits + order[row]);
    reinterpret_cast<double2*>(out + row)[t & 3] = src[t & 3];
  }
}

}  // namespace
#include "odw_spec.hip"
namespace {

// Mesh launches of device-generated rays: the order the rays are handed out in = sorted by where they start and where
// they point (odw_mesh.hip: odw_ray_key_kernel), so that the 64 rays of a wave are neighbours among all rays of the
// launch -- the same nodes, the same leaves, the same cache lines; a ray's rows depend on its number only, so the
// results are those of the unsorted launch.  Cost: one generation pass for the keys + a radix sort of (key, number)
// pairs (1e7 rays: ~0.8 ms against 10 - 17 ms of tracing); short launches and ODW_MESH_PRESORT=0 keep the plain order.
int presort_rays(odw_ctx* ctx, uint64_t first, uint64_t n, uint64_t seed) {
  // (read at every launch: the test that holds the two orders against each other)
  const bool off = getenv("ODW_MESH_PRESORT") && getenv("ODW_MESH_PRESORT")[0] == '0';
  const char* e_min = getenv("ODW_MESH_PRESORT_MIN");
  const uint64_t min_rays = e_min ? (uint64_t)atoll(e_min) : (1ull << 16);
  if (off || n < min_rays || n > 0x7FFFFFFFull) return ODW_OK;
  int rc;
  for (int k = 0; k < 2; ++k) {
    if ((rc = ensure(ctx, ctx->sort_keys[k], n * sizeof(uint64_t)))) return rc;
    if ((rc = ensure(ctx, ctx->sort_vals[k], n * sizeof(uint32_t)))) return rc;
  }
  const DeviceScene& sc = ctx->P.scene;
  double lo[3], scale[3];
  for (int a = 0; a < 3; ++a) {
    lo[a] = sc.wide_lo[a];
    const double w = sc.wide_hi[a] - sc.wide_lo[a];
    scale[a] = w > 0 ? 1024.0 / w : 0.0;
  }
  uint64_t* k_in = (uint64_t*)ctx->sort_keys[0].p;
  uint64_t* k_out = (uint64_t*)ctx->sort_keys[1].p;
  uint32_t* v_in = (uint32_t*)ctx->sort_vals[0].p;
  uint32_t* v_out = (uint32_t*)ctx->sort_vals[1].p;
  // a point source with focal length 0 starts every ray at one point: the direction bits alone, as 32-bit keys
  // (four passes of eight bits over half the bytes)
  const bool dir_only = ctx->h_source.finite_focal && ctx->h_source.focal_length == 0.0;
  const unsigned kgrid = (unsigned)((n + 255) / 256);
  size_t tmp_bytes = 0;
  if (dir_only) {
    uint32_t* k32_in = (uint32_t*)k_in;
    uint32_t* k32_out = (uint32_t*)k_out;
    hipLaunchKernelGGL(odw_ray_key_kernel<uint32_t>, dim3(kgrid), dim3(256), 0, ctx->stream, ctx->P.source, first, n, seed,
                       lo[0], lo[1], lo[2], scale[0], scale[1], scale[2], k32_in, v_in);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, k32_in, k32_out, v_in, v_out, (int)n, 0, 32, ctx->stream));
    if ((rc = ensure(ctx, ctx->sort_tmp, tmp_bytes))) return rc;
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairs(ctx->sort_tmp.p, tmp_bytes, k32_in, k32_out, v_in, v_out, (int)n, 0, 32, ctx->stream));
  } else {
    hipLaunchKernelGGL(odw_ray_key_kernel<uint64_t>, dim3(kgrid), dim3(256), 0, ctx->stream, ctx->P.source, first, n, seed,
                       lo[0], lo[1], lo[2], scale[0], scale[1], scale[2], k_in, v_in);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, k_in, k_out, v_in, v_out, (int)n, 0, 62, ctx->stream));
    if ((rc = ensure(ctx, ctx->sort_tmp, tmp_bytes))) return rc;
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairs(ctx->sort_tmp.p, tmp_bytes, k_in, k_out, v_in, v_out, (int)n, 0, 62, ctx->stream));
  }
  ctx->P.ray_order = v_out;
  ctx->ph_valid = false;           // (the sort buffers are shared with odw_hits_select)
  return ODW_OK;
}


// ---- which kernel a launch takes ---------------------------------------------------------------
// What the scene's structures alone say is accel_kind() (odw_build.h; odw_build_check answers with it), and every kind
// has its kernel.  What a launch makes of it: a scene compiled against its structure (odw_spec.hip) takes its own kernel,
// whatever else was built for it -- the variant this launch needs must be bound, for the scene as it is now.  Segment
// rows are written by the flat and tree kernels only; stochastic surfaces are unknown to the grid kernel: such
// launches fall back to the trees, which every scene with a grid has too.  (Batches hold scenes without structures:
// compiled or flat; or scenes that have structures only because of their paraboloids or ellipsoids: compiled.)
enum class TraceKernel { flat = kAccelFlat, grid = kAccelGrid, tree = kAccelTree, mesh = kAccelWide, compiled };

// Monochromatic launches and dispersion: the index of every dispersive group at the launch wavelength goes into its table
// word (hs.group_f64[4 g], from which a compiled scene's image is built per launch, and the device table the generic
// kernels read) -- on the host, before the launch, again when wavelength, dispersion or scene have changed.  No kernel
// knows about it.
int fold_dispersion(odw_ctx* ctx) {
  if (!ctx->disp_on && !ctx->fold_dirty) return ODW_OK;
  const double wl = ctx->P.wavelength;
  if (!ctx->fold_dirty && wl == ctx->fold_wl) return ODW_OK;
  const int G = ctx->hs.n_groups;
  if (ctx->disp_on) {
    std::string err;
    const int rc = disp_check_range(G, ctx->disp_kind, ctx->disp_coef, wl, wl, err);
    if (rc) return fail(ctx, rc, err);
  }
  for (int g = 0; g < G && g < (int)ctx->base_ior.size(); ++g)
    ctx->hs.group_f64[4 * (size_t)g] = (ctx->disp_on && ctx->disp_kind[g]) ? disp_index(ctx->disp_kind[g], ctx->disp_coef + ODW_DISP_COEFS * g, wl)
                                                                           : ctx->base_ior[(size_t)g];
  int rc = upload(ctx, ctx->group_f64, ctx->hs.group_f64.data(), ctx->hs.group_f64.size() * sizeof(double));
  if (rc) return rc;
  ctx->fold_wl = wl;
  ctx->fold_dirty = false;
  return ODW_OK;
}

// the context's dispersion as the CHROMA kernels read it (all kinds 0 while none is set)
int upload_dispersion(odw_ctx* ctx) {
  int rc;
  if ((rc = upload(ctx, ctx->d_disp_kind, ctx->disp_kind, sizeof ctx->disp_kind))) return rc;
  return upload(ctx, ctx->d_disp_coef, ctx->disp_coef, sizeof ctx->disp_coef);
}

// Spectral launches, and launches with a Fresnel mode set, walk the binary tree.  A scene the flat loop takes has none: one
// is built for them (one tree for both), kept beside the scene's own structures (which stay what they are: the plain
// launches of the same scene keep their kernel).
int chroma_tree(odw_ctx* ctx) {
  if (ctx->chroma_n_nodes) return ODW_OK;
  std::vector<Box> boxes;
  HostScene hs = ctx->hs;                  // (compute_boxes writes headers and flags: the context's stay as build_bvh left them)
  compute_boxes(hs, ctx->P.lim.dist_tol, boxes);
  SceneAccel A;
  std::string err;
  BuildOptions opt = build_options();
  opt.force_tree = true;
  int rc = build_accel(hs, std::move(boxes), ctx->P.lim.dist_tol, ctx->flat_limit, opt, A, err);
  if (rc) return fail(ctx, rc, err);
  if (A.nodes.empty()) return fail(ctx, ODW_ERR_DEVICE, "spectral launch: no binary tree could be built for the scene");
  if ((rc = upload(ctx, ctx->chroma_nodes, A.nodes.data(), A.nodes.size() * sizeof(BvhNode)))) return rc;
  if ((rc = upload(ctx, ctx->chroma_prims, A.order.data(), A.order.size() * sizeof(int)))) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));      // (A goes out of scope)
  ctx->chroma_n_nodes = (int)A.nodes.size();
  return ODW_OK;
}

TraceKernel choose_kernel(const odw_ctx* ctx, uint32_t flags, bool batch) {
  const DeviceScene& S = ctx->P.scene;
  const bool segments = (flags & ODW_TRACE_RECORD_SEGMENTS) != 0, stoch = ctx->n_samplers > 0;
  const hipFunction_t fn = batch ? ctx->spec_batch_fn : (flags & ODW_TRACE_POWER_HISTOGRAM) ? ctx->spec_power_fn : ctx->spec_fn;
  if (fn && ctx->spec_lean == ctx->hs.lean && ctx->spec_stoch == stoch && !segments) return TraceKernel::compiled;
  return (TraceKernel)accel_kind(ctx->P.grid.nx > 0 && !stoch && !segments, S.n_nodes != 0, S.bvh_leaf != nullptr && !segments);
}

// ray_wl: a wavelength per explicit ray (device array).  A launch with it, or one that generates its rays under a bound
// spectrum, is SPECTRAL: the CHROMA variant of the compiled kernel where one is bound for the scene as it is, else the
// CHROMA instantiations of the binary tree.  Every other launch is monochromatic: the dispersion is folded into the
// tables, the kernels are those of before.  wl_lo, wl_hi: the smallest and largest of ray_wl.
int launch_trace(odw_ctx* ctx, uint64_t first, uint64_t n, uint64_t seed, uint32_t flags,
                 const double* ray_o, const double* ray_d, const double* ray_p, const double* ray_wl = nullptr,
                 double wl_lo = 0.0, double wl_hi = 0.0) {
  const bool explicit_rays = ray_o != nullptr;
  if (!ctx->have_scene || !ctx->have_limits) return fail(ctx, ODW_ERR_NO_SCENE, "scene/limits not uploaded");
  if (!explicit_rays && !ctx->have_source) return fail(ctx, ODW_ERR_NO_SCENE, "source not uploaded");
  if (n == 0) return ODW_OK;
  const bool spectral = ray_wl != nullptr || (!explicit_rays && ctx->spec_n > 0);
  if (ctx->batch_launch && ctx->disp_on)
    return fail(ctx, ODW_ERR_UNSUPPORTED, "odw_trace_batch: a batch with a dispersion set (per-scene dispersion is out of scope)");
  if (ctx->batch_launch && ctx->band_n)
    return fail(ctx, ODW_ERR_UNSUPPORTED, "odw_trace_batch: a batch with detector bands set (band planes: batches carry no spectrum, and one detector "
                                          "cannot serve several scenes; clear them with odw_set_detector_bands(ctx, 0, NULL))");
  if (spectral) {
    if (ctx->batch_launch) return fail(ctx, ODW_ERR_UNSUPPORTED, "spectral launch: batches carry no spectrum (spectral batches are out of scope)");
    if (ctx->n_samplers > 0) return fail(ctx, ODW_ERR_UNSUPPORTED, "spectral launch: scenes with stochastic surfaces are not supported");
    if (!ray_wl && ctx->emitter_active) return fail(ctx, ODW_ERR_UNSUPPORTED, "spectral launch: surface sources carry no spectrum");
    if (ctx->disp_on) {
      std::string err;
      const int rc = disp_check_range(ctx->hs.n_groups, ctx->disp_kind, ctx->disp_coef, ray_wl ? wl_lo : ctx->spec_lo,
                                      ray_wl ? wl_hi : ctx->spec_hi, err);
      if (rc) return fail(ctx, rc, err);
    }
  } else {
    const int rc = fold_dispersion(ctx);
    if (rc) return rc;
  }
  const bool fresnel = ctx->fresnel_on;
  if (fresnel) {
    if (ctx->batch_launch) return fail(ctx, ODW_ERR_UNSUPPORTED, "odw_trace_batch: a batch with a Fresnel mode set (per-scene Fresnel modes are out of scope)");
    if (ctx->n_samplers > 0) return fail(ctx, ODW_ERR_UNSUPPORTED, "Fresnel launch: scenes with stochastic surfaces are not supported");
    if (ctx->fresnel_split && ctx->hs.seq_enabled)
      return fail(ctx, ODW_ERR_UNSUPPORTED, "Fresnel launch: 'Split' in a scene with a tracing sequence is not supported (a ghost has no place in the sequence)");
  }
  ctx->ph_valid = false;           // the hit list is about to change
  if (!ctx->batch_launch) {
    ctx->hit_ray_begin = ctx->hit_ray_end ? std::min<uint64_t>(ctx->hit_ray_begin, first) : first;
    ctx->hit_ray_end = std::max<uint64_t>(ctx->hit_ray_end, std::min<uint64_t>(first + n, 1ull << 48));
  }
  if (ctx->bvh_dirty) {
    int rc = build_bvh(ctx);
    if (rc) return rc;
  }
  // a launch that generates its rays takes the kernel compiled against its source's structure; explicit rays and
  // batches (whose rays come from buffers) run whatever is bound, and bind the source-free kernel if nothing is
  {
    uint64_t want = ctx->spec_source_key;
    if (!explicit_rays && !ctx->batch_launch) want = ctx->source_key;
    else if (ctx->spec_dirty) want = 0;
    if (want != ctx->spec_source_key) { ctx->spec_source_key = want; ctx->spec_dirty = true; }
  }
  if (ctx->spec_dirty) {
    // a scene kernel that cannot be built (no hiprtc on this machine, a compiler error) is not a reason to
    // stop tracing: the generic kernels run, odw_compile_scene / odw_last_error tell why
    if (spec_bind(ctx) != ODW_OK) ctx->spec_fn = nullptr;
  }
  if ((flags & ODW_TRACE_RECORD_HITS) && (ctx->batch_launch ? ctx->batch_seg_capacity : ctx->hit_capacity) == 0)
    return fail(ctx, ODW_ERR_CAPACITY, "ODW_TRACE_RECORD_HITS without odw_reserve_hits");
  if (flags & ODW_TRACE_RECORD_SEGMENTS) {
    if (ctx->seg_capacity == 0)
      return fail(ctx, ODW_ERR_CAPACITY, "ODW_TRACE_RECORD_SEGMENTS without odw_reserve_segments");
    if (first + n > ODW_SEG_MAX_RAY || ctx->P.lim.max_intersections > ODW_SEG_MAX_ORDINAL)
      return fail(ctx, ODW_ERR_INVALID, "ODW_TRACE_RECORD_SEGMENTS: ray index or max_intersections beyond the row tag");
  }
  if ((flags & ODW_TRACE_HISTOGRAM) && !ctx->P.det_enabled) flags &= ~ODW_TRACE_HISTOGRAM;
  // (the kernels add to the words behind the histogram under this flag: never without a plane there)
  if (!(flags & ODW_TRACE_HISTOGRAM) || !ctx->power_on) flags &= ~(uint32_t)ODW_TRACE_POWER_HISTOGRAM;
  // (likewise the band planes; a launch that asks for them and cannot fill them is refused, not run without)
  if (!(flags & ODW_TRACE_HISTOGRAM) || !ctx->band_n) flags &= ~(uint32_t)ODW_TRACE_BAND_HISTOGRAM;
  const bool bands = (flags & ODW_TRACE_BAND_HISTOGRAM) != 0;     // the BANDS kernels: DeviceBands in DeviceChroma's place
  if (bands) {
    if (!spectral) return fail(ctx, ODW_ERR_UNSUPPORTED, "band planes: the launch is monochromatic (no spectrum bound, no wavelength per ray): "
                                                         "its total plane is its one band's plane; bands for monochromatic launches are out of scope");
    if (flags & ODW_TRACE_RECORD_SEGMENTS) return fail(ctx, ODW_ERR_UNSUPPORTED, "band planes: a launch with ODW_TRACE_RECORD_SEGMENTS (record_segments) cannot fill them");
    if (!ctx->d_band_edges.p) return fail(ctx, ODW_ERR_DEVICE, "band planes without their edge table");
  }
  TraceParams& P = ctx->P;
  const bool batch = ctx->batch_launch;
  std::memset(&P.batch, 0, sizeof P.batch);
  if (batch) {
    // scenes of one structure side by side: flat kernels only (the scene the context holds is scene 0 of the batch)
    const bool rare = flat_but_for_rare_quadrics(ctx->hs, ctx->flat_limit);
    if (((P.scene.n_nodes || P.grid.nx > 0) && !rare) || ctx->n_samplers > 0 || explicit_rays || (flags & ODW_TRACE_RECORD_SEGMENTS))
      return fail(ctx, ODW_ERR_UNSUPPORTED, "odw_trace_batch: batches are traced by the flat kernels (analytic scenes of up to 64 "
                                            "primitives, no stochastic surfaces, no segment rows)");
    flags &= ~(uint32_t)(ODW_TRACE_HISTOGRAM | ODW_TRACE_POWER_HISTOGRAM);   // (one histogram cannot serve several scenes)
  }
  P.first_ray = first;
  P.n_rays = n;
  P.seed = seed;
  P.flags = flags;
  P.samplers = (const DeviceSurfaceSampler*)ctx->d_samplers.p;
  P.group_sampler = (const int32_t*)ctx->d_group_sampler.p;
  P.ray_origins = ray_o;
  P.ray_dirs = ray_d;
  P.ray_powers = ray_p;
  P.ray_stride = n;
  P.dbg = (unsigned long long*)ctx->dbg.p;
  P.out.hits = (odw_hit*)(batch ? ctx->batch_hits.p : ctx->hits.p);
  P.out.hit_capacity = batch ? ctx->batch_seg_slots : ctx->hit_slots;
  // block reservations need room for the unused slots they can leave behind: < 64 per block and the
  // last block of every wave of the grid
  P.out.hit_block = 0;
  P.out.hit_count = (unsigned long long*)(batch ? ctx->batch_hit_count.p : ctx->hit_count.p);
  P.out.hist = (unsigned long long*)ctx->hist.p;
  P.out.counters = (unsigned long long*)ctx->counters.p;
  P.out.chunk_counter = (unsigned long long*)ctx->chunk_counter.p;
  P.out.segs = (odw_segment*)ctx->segs.p;
  P.out.seg_capacity = ctx->seg_capacity;
  P.out.seg_count = (unsigned long long*)ctx->seg_count.p;
  P.out.row_of = (batch && ctx->batch_marked && (flags & ODW_TRACE_RECORD_HITS)) ? (uint32_t*)ctx->phb_row_of.p : nullptr;
  P.out.row_stride = batch ? (n + 31) / 32 * 32 : 0;
  P.out.pts = (P.out.row_of && ctx->batch_pts) ? (double*)ctx->phb_pts.p : nullptr;

  // persistent waves: one grid that fills the chip (4 blocks of 256 threads
  // per CU at 4 waves/SIMD, x2 so that a CU never waits for a block launch);
  // chunks of ODW_CHUNK rays are handed out dynamically inside the kernel
  constexpr int grid_mult = 8;
  const bool pw = (flags & ODW_TRACE_POWER_HISTOGRAM) != 0;     // the <..., POWER = true> instantiation of whichever kernel runs
  if (pw && !spectral && ctx->spec_fn && !ctx->spec_power_fn && !ctx->spec_power_failed &&
      !(ctx->spec_power_wait && !ctx->spec_power_wait->load())) {
    // the compiled kernel's POWER variant: bound on the first weighted launch of the structure (a compilation of its own,
    // cached like the other).  ODW_COMPILE_STRUCTURE: that launch waits for it.  ODW_COMPILE_AUTO: the structure has earned
    // its compilation already (its single-scene kernel is bound), so the variant's starts at once on a thread, weighted
    // launches run the generic POWER kernel and look at the job's flag only, and the first one after it has finished binds
    // it.  One attempt per binding: a variant that cannot be built is not asked for again, and its failure does not become
    // the error of a launch that succeeds on the generic kernel
    const std::string keep_err = ctx->err;
    const bool waited = ctx->spec_power_wait != nullptr;
    ctx->spec_power_wait = nullptr;
    if (spec_bind(ctx, kSpecPower) != ODW_OK || (!ctx->spec_power_fn && (waited || !ctx->spec_power_wait))) {
      ctx->spec_power_fn = nullptr;
      ctx->spec_power_failed = true;
      ctx->err = keep_err;
    }
  }
  if (batch && ctx->spec_fn && !ctx->spec_batch_fn && !ctx->spec_batch_failed && ctx->batch_img_off) {
    // the compiled kernel's BATCH variant: bound on the first batch launch of the structure (a compilation of its own,
    // cached like the other; odw_compile_scene's mode decides, as for single launches).  A variant that cannot be built
    // is not tried again for this binding, and its failure does not become the error of a launch that succeeds on the
    // generic kernel
    const std::string keep_err = ctx->err;
    if (spec_bind(ctx, kSpecBatch) != ODW_OK) {
      ctx->spec_batch_fn = nullptr;
      ctx->spec_batch_failed = true;
      ctx->err = keep_err;
    }
  }
  // The compiled kernel's CHROMA variant (its header carries the context's dispersion): bound on the first spectral launch
  // while the single-scene kernel is bound, ODW_COMPILE_STRUCTURE only; one attempt per binding, and a variant that cannot
  // be built does not become the error of a launch that succeeds on the tree
  const bool segments = (flags & ODW_TRACE_RECORD_SEGMENTS) != 0;
  if (bands && !fresnel && ctx->spec_fn && !ctx->spec_bands_fn[pw] && !ctx->spec_bands_failed) {
    // (its BANDS variant: on the first spectral launch with band planes, under the same rules)
    const std::string keep_err = ctx->err;
    if (spec_bind(ctx, pw ? kSpecBandsPower : kSpecBands) != ODW_OK) {
      ctx->spec_bands_fn[pw] = nullptr;
      ctx->spec_bands_failed = true;
      ctx->err = keep_err;
    }
  }
  if (spectral && !bands && !fresnel && !segments && ctx->spec_fn && !ctx->spec_chroma_fn[pw] && !ctx->spec_chroma_failed) {
    const std::string keep_err = ctx->err;
    if (spec_bind(ctx, pw ? kSpecChromaPower : kSpecChroma) != ODW_OK) {
      ctx->spec_chroma_fn[pw] = nullptr;
      ctx->spec_chroma_failed = true;
      ctx->err = keep_err;
    }
  }
  // The compiled kernel's FRESNEL variant (its header carries the context's modes): likewise, on the first monochromatic
  // launch with a mode set
  if (fresnel && !spectral && !segments && ctx->spec_fn && !ctx->spec_fresnel_fn[pw] && !ctx->spec_fresnel_failed) {
    const std::string keep_err = ctx->err;
    if (spec_bind(ctx, pw ? kSpecFresnelPower : kSpecFresnel) != ODW_OK) {
      ctx->spec_fresnel_fn[pw] = nullptr;
      ctx->spec_fresnel_failed = true;
      ctx->err = keep_err;
    }
  }
  // (after the bindings above: they decide `compiled`.)  A spectral launch goes to the compiled kernel when its CHROMA
  // variant is bound for the scene as it is, else to the binary tree -- never to the flat, grid or mesh kernel, which know
  // no wavelength per ray
  const hipFunction_t chroma_fn = bands ? ctx->spec_bands_fn[pw] : ctx->spec_chroma_fn[pw];
  const bool chroma_compiled = spectral && !fresnel && !segments && ctx->spec_fn && chroma_fn && ctx->spec_lean == ctx->hs.lean;
  // A launch with a Fresnel mode set: the compiled kernel's FRESNEL variant where it is bound for the scene as it is and the
  // launch is monochromatic, else the binary tree (spectral + Fresnel: always) -- never the flat, grid or mesh kernel
  const bool fresnel_compiled = fresnel && !spectral && !segments && ctx->spec_fn && ctx->spec_fresnel_fn[pw] && ctx->spec_lean == ctx->hs.lean;
  const TraceKernel kernel = fresnel ? (fresnel_compiled ? TraceKernel::compiled : TraceKernel::tree)
                             : spectral ? (chroma_compiled ? TraceKernel::compiled : TraceKernel::tree) : choose_kernel(ctx, flags, batch);
  DeviceBands chroma;                      // (the CHROMA kernels without BANDS take its DeviceChroma part)
  std::memset(&chroma, 0, sizeof chroma);
  if (bands) {
    chroma.band_edges = (const double*)ctx->d_band_edges.p;
    chroma.n_edges = ctx->band_n;
    chroma.n_bins = (int32_t)ctx->n_bins;
    chroma.count_off = ctx->n_bins * (ctx->power_on ? 2 : 1);
    chroma.power_off = chroma.count_off + ctx->n_bins * ctx->band_k();
  }
  const DeviceChroma& chroma_only = chroma;
  DeviceFresnel fresnel_arg;
  fresnel_arg.mode = (const int32_t*)ctx->d_fresnel_mode.p;
  const bool coated = fresnel && ctx->coat_on;
  DeviceCoat coat_arg;                     // the COAT kernels' argument: the modes and the stacks
  coat_arg.mode = fresnel_arg.mode;
  coat_arg.coat_n = coated ? (const int32_t*)ctx->d_coat_n.p : nullptr;
  coat_arg.coat = coated ? (const double*)ctx->d_coat.p : nullptr;
  if (fresnel && !fresnel_compiled) {
    int rc;
    if (!fresnel_arg.mode) return fail(ctx, ODW_ERR_DEVICE, "Fresnel launch without its mode table");
    if (coated && (!coat_arg.coat_n || !coat_arg.coat)) return fail(ctx, ODW_ERR_DEVICE, "coated launch without its layer tables");
    if (!P.scene.n_nodes && (rc = chroma_tree(ctx))) return rc;
  }
  TraceParams Pc;                          // the spectral launch's arguments: P, with the tree built for it where the scene has none
  if (spectral) {
    int rc;
    if (!ctx->d_disp_kind.p && (rc = upload_dispersion(ctx))) return rc;
    if (!chroma_compiled && !P.scene.n_nodes && (rc = chroma_tree(ctx))) return rc;
    chroma.ray_wl = ray_wl;
    chroma.spec_tab = ray_wl ? nullptr : (const double*)ctx->spec_tab.p;
    chroma.spec_n = ctx->spec_n;
    chroma.spec_mode = ctx->spec_mode;
    chroma.disp_kind = (const int32_t*)ctx->d_disp_kind.p;
    chroma.disp_coef = (const double*)ctx->d_disp_coef.p;
  }
  if (batch && kernel != TraceKernel::compiled && flat_but_for_rare_quadrics(ctx->hs, ctx->flat_limit))
    return fail(ctx, ODW_ERR_UNSUPPORTED, "odw_trace_batch: a batch with paraboloids or ellipsoids needs the kernel compiled against the scene, "
                                          "which is not bound (odw_compile_scene: ODW_COMPILE_STRUCTURE)");
  const bool use_spec = kernel == TraceKernel::compiled, use_grid = kernel == TraceKernel::grid, use_mesh = kernel == TraceKernel::mesh,
             use_tree = kernel == TraceKernel::tree;
  // Rays per hand-out unit.  A launch should hold many chunks per resident wave: with about one each -- 1e7 rays in
  // chunks of 2048 on 4096 resident waves -- the waves that get a second one set the launch's length.  Measured
  // (kernel ms at 1e7 / 1e8 rays): flat kernels 2048: 1.46 / 11.07, 1024: 1.44 / 10.93, 512: 1.39 / 10.97, 256: 1.43;
  // the ring kernels (grid, mesh: a ring fill is 64 rays whatever the chunk) 2048: 2.24 / 21.34, 512: 2.05 / 20.95,
  // 256: 1.96 / 20.86, and the mesh kernel at 1e7 rays and 6.5e4 facets 2048: 14.6, 256: 12.5, 64: 12.3.
  {
    const bool ring = use_grid || use_mesh;
    const uint64_t waves = (uint64_t)ctx->n_cu * 16;
    const uint64_t want = ring ? std::max<uint64_t>(64, std::min<uint64_t>(256, n / (waves * 32)))
                               : std::max<uint64_t>(512, std::min<uint64_t>(1024, n / (waves * 4)));
    P.chunk = (uint32_t)(want & ~(uint64_t)63);
  }
  uint64_t n_chunks = (n + P.chunk - 1) / P.chunk;
  if (batch) {
    // n = the rays of ONE scene; the launch hands out chunks_per_scene units per scene
    const uint64_t total = n * (uint64_t)ctx->batch_traced, waves = (uint64_t)ctx->n_cu * 16;
    P.chunk = (uint32_t)(std::max<uint64_t>(512, std::min<uint64_t>(1024, total / (waves * 4))) & ~(uint64_t)63);
    const uint64_t cps = (n + P.chunk - 1) / P.chunk;
    if (cps * (uint64_t)ctx->batch_traced >= (1ull << 32)) return fail(ctx, ODW_ERR_INVALID, "odw_trace_batch: too many hand-out units");
    P.batch.rays = n;
    P.batch.stride = ctx->batch_stride;
    P.batch.chunks_per_scene = (uint32_t)cps;
    P.batch.n_scenes = (uint32_t)ctx->batch_traced;
    n_chunks = cps * (uint64_t)ctx->batch_traced;
    // the batch's rays once, for all its scenes (from three scenes on: the pass writes 24 bytes per ray -- 48 where the
    // origins differ -- and every scene reads them; fewer scenes generate their own)
    P.batch.gen_dirs = P.batch.gen_origins = nullptr;
    P.batch.gen_stride = 0;
    if (ctx->batch_traced >= 3) {
      const bool one_origin = ctx->h_source.finite_focal && ctx->h_source.focal_length == 0.0;
      const uint64_t gs = (n + 31) / 32 * 32;
      const size_t bytes = (size_t)(gs * (one_origin ? 3 : 6) + 4) * sizeof(double);
      // (sized by odw_batch_reserve before a sweep; here only if nobody did: a launch without the pass is still right)
      if (ctx->batch_rays_buf.bytes >= bytes || ensure(ctx, ctx->batch_rays_buf, bytes) == ODW_OK) {
        double* dirs = (double*)ctx->batch_rays_buf.p;
        double* orgs = one_origin ? nullptr : dirs + 3 * gs + 4;
        P.batch.gen_dirs = dirs;                    // (the pass itself: below, inside the launch's timed interval)
        P.batch.gen_origins = orgs;
        P.batch.gen_stride = gs;
      } else {
        ctx->err.clear();
      }
    }
  }
  // Batch launches share the GPU with the post-hoc chains of other contexts (a sweep keeps several groups in flight): three
  // blocks per CU instead of all four leave a quarter of every SIMD's registers to their kernels and to the runtime's copy
  // kernels, which otherwise wait until a persistent block retires, i.e. for the whole launch (measured on the 64 x 1e7
  // sweep with 16 hardware queues: 98 ms -> 86 ms per sweep)
  constexpr int batch_mult = 3;
  const uint64_t cap = (uint64_t)ctx->n_cu * (batch ? batch_mult : grid_mult);
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n_chunks + 3) / 4, cap));
  const uint64_t grid_blocks = std::max<uint64_t>(1, std::min<uint64_t>((n_chunks + ODW_GRID_WAVES - 1) / ODW_GRID_WAVES, (uint64_t)ctx->n_cu));
  const uint64_t n_waves = use_grid ? grid_blocks * ODW_GRID_WAVES : (uint64_t)grid * 4;
  if (!use_tree && !ctx->swapping)   // compiled, flat, grid and mesh kernels only (see record_hit)
    for (uint32_t b = kHitBlock; b >= 128 && b >= kHitBlock / 4 && !P.out.hit_block; b /= 2)   // (a short list: smaller blocks before none)
      if (batch ? ctx->batch_seg_slots >= ctx->batch_seg_capacity + hit_block_room(ctx->batch_seg_capacity, n_waves, b)
                : ctx->hit_slots >= ctx->hit_capacity + hit_block_room(ctx->hit_capacity, n_waves, b)) P.out.hit_block = b;
  HIPCHK(ctx, hipMemsetAsync(ctx->chunk_counter.p, 0, sizeof(uint64_t), ctx->stream));
  const size_t lds = use_tree ? (size_t)ODW_BVH_STACK * 256 * sizeof(int) : 0;

  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  if (ctx->timing) {
    if (!ctx->free_events.empty()) {
      ev = ctx->free_events.back();
      ctx->free_events.pop_back();
    } else {
      HIPCHK(ctx, hipEventCreate(&ev.first));
      HIPCHK(ctx, hipEventCreate(&ev.second));
    }
    HIPCHK(ctx, hipEventRecord(ev.first, ctx->stream));
  }
  if (batch && P.batch.gen_dirs) {
    const unsigned gb = (unsigned)std::min<uint64_t>((n + 255) / 256, (uint64_t)ctx->n_cu * 16);
    hipLaunchKernelGGL(odw_batch_rays_kernel, dim3(gb), dim3(256), 0, ctx->stream, P.source, first, n, seed,
                       const_cast<double*>(P.batch.gen_dirs), const_cast<double*>(P.batch.gen_origins), P.batch.gen_stride);
  }
  const bool stoch = ctx->n_samplers > 0;
  const bool asph = P.asph != nullptr;       // the scene holds an asphere: the tree and grid instantiations of their own
  P.ray_order = nullptr;
  if (use_mesh && !explicit_rays) {
    int rc = presort_rays(ctx, first, n, seed);       // (inside the timed window: part of the launch's cost)
    if (rc) return rc;
  }
  if (fresnel_compiled) {
    int rc = spec_launch(ctx, grid, ctx->spec_fresnel_fn[pw], false, nullptr, true);
    if (rc) return rc;
  } else if (fresnel) {
    Pc = P;
    if (!P.scene.n_nodes) {
      Pc.scene.bvh_nodes = (const float*)ctx->chroma_nodes.p;
      Pc.scene.bvh_prims = (const int32_t*)ctx->chroma_prims.p;
      Pc.scene.n_nodes = ctx->chroma_n_nodes;
    }
    // (a coating on some group: the COAT instantiations; without, the kernels of before)
#define ODW_FRESNEL_LAUNCH(S, W, A, C) do { \
      if (coated) hipLaunchKernelGGL((odw_trace_coat_kernel<S, W, A, C>), dim3(grid), dim3(256), lds, ctx->stream, Pc, chroma_only, coat_arg); \
      else hipLaunchKernelGGL((odw_trace_fresnel_kernel<S, W, A, C>), dim3(grid), dim3(256), lds, ctx->stream, Pc, chroma_only, fresnel_arg); } while (0)
    // (band planes: spectral, no segment rows -- the BANDS kernels, POWER x ASPH)
#define ODW_FRESNEL_BANDS_LAUNCH(W, A) do { \
      if (coated) hipLaunchKernelGGL((odw_trace_coat_bands_kernel<W, A>), dim3(grid), dim3(256), lds, ctx->stream, Pc, chroma, coat_arg); \
      else hipLaunchKernelGGL((odw_trace_fresnel_bands_kernel<W, A>), dim3(grid), dim3(256), lds, ctx->stream, Pc, chroma, fresnel_arg); } while (0)
#define ODW_FRESNEL_LAUNCH_C(S, W, A) do { if (spectral) ODW_FRESNEL_LAUNCH(S, W, A, true); else ODW_FRESNEL_LAUNCH(S, W, A, false); } while (0)
#define ODW_FRESNEL_LAUNCH_A(S, W) do { if (asph) ODW_FRESNEL_LAUNCH_C(S, W, true); else ODW_FRESNEL_LAUNCH_C(S, W, false); } while (0)
    if (bands) {
      if (pw) { if (asph) ODW_FRESNEL_BANDS_LAUNCH(true, true); else ODW_FRESNEL_BANDS_LAUNCH(true, false); }
      else { if (asph) ODW_FRESNEL_BANDS_LAUNCH(false, true); else ODW_FRESNEL_BANDS_LAUNCH(false, false); }
    } else
    if (segments) { if (pw) ODW_FRESNEL_LAUNCH_A(true, true); else ODW_FRESNEL_LAUNCH_A(true, false); }
    else { if (pw) ODW_FRESNEL_LAUNCH_A(false, true); else ODW_FRESNEL_LAUNCH_A(false, false); }
#undef ODW_FRESNEL_BANDS_LAUNCH
#undef ODW_FRESNEL_LAUNCH_A
#undef ODW_FRESNEL_LAUNCH_C
#undef ODW_FRESNEL_LAUNCH
  } else if (chroma_compiled) {
    int rc = spec_launch(ctx, grid, chroma_fn, false, &chroma, false, bands ? sizeof(DeviceBands) : sizeof(DeviceChroma));
    if (rc) return rc;
  } else if (spectral) {
    Pc = P;
    if (!P.scene.n_nodes) {
      Pc.scene.bvh_nodes = (const float*)ctx->chroma_nodes.p;
      Pc.scene.bvh_prims = (const int32_t*)ctx->chroma_prims.p;
      Pc.scene.n_nodes = ctx->chroma_n_nodes;
    }
    const bool seg = (flags & ODW_TRACE_RECORD_SEGMENTS) != 0;
#define ODW_CHROMA_LAUNCH(S, W, A) hipLaunchKernelGGL((odw_trace_chroma_kernel<S, W, A>), dim3(grid), dim3(256), lds, ctx->stream, Pc, chroma_only)
#define ODW_CHROMA_BANDS_LAUNCH(W, A) hipLaunchKernelGGL((odw_trace_chroma_bands_kernel<W, A>), dim3(grid), dim3(256), lds, ctx->stream, Pc, chroma)
#define ODW_CHROMA_LAUNCH_A(S, W) do { if (asph) ODW_CHROMA_LAUNCH(S, W, true); else ODW_CHROMA_LAUNCH(S, W, false); } while (0)
    if (bands) {
      if (pw) { if (asph) ODW_CHROMA_BANDS_LAUNCH(true, true); else ODW_CHROMA_BANDS_LAUNCH(true, false); }
      else { if (asph) ODW_CHROMA_BANDS_LAUNCH(false, true); else ODW_CHROMA_BANDS_LAUNCH(false, false); }
    } else
    if (seg) { if (pw) ODW_CHROMA_LAUNCH_A(true, true); else ODW_CHROMA_LAUNCH_A(true, false); }
    else { if (pw) ODW_CHROMA_LAUNCH_A(false, true); else ODW_CHROMA_LAUNCH_A(false, false); }
#undef ODW_CHROMA_BANDS_LAUNCH
#undef ODW_CHROMA_LAUNCH_A
#undef ODW_CHROMA_LAUNCH
  } else if (use_spec) {
    int rc = spec_launch(ctx, grid, batch ? ctx->spec_batch_fn : pw ? ctx->spec_power_fn : ctx->spec_fn, batch);
    if (rc) return rc;
  } else if (batch) {
    if (ctx->hs.lean) hipLaunchKernelGGL((odw_trace_kernel<false, false, false, true, true>), dim3(grid), dim3(256), 0, ctx->stream, P);
    else hipLaunchKernelGGL((odw_trace_kernel<false, false, false, false, true>), dim3(grid), dim3(256), 0, ctx->stream, P);
  } else if (use_grid) {
    const dim3 gb((unsigned)grid_blocks);
    const size_t glds = P.grid.lds_bytes;
#define ODW_GRID_LAUNCH_(S, L, W, A)                                                                              \
    do {                                                                                                       \
      /* (once per device and instantiation: a second context on another GPU of the process needs its own) */  \
      static uint64_t attr_set = 0;                                                                            \
      const uint64_t dev_bit = 1ull << (ctx->device & 63);                                                     \
      if (!(attr_set & dev_bit)) {                                                                             \
        HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&odw_grid_kernel<S, L, W, A>),           \
                                        hipFuncAttributeMaxDynamicSharedMemorySize, 155 * 1024));   /* + 4.5 KB static */ \
        attr_set |= dev_bit;                                                                                   \
      }                                                                                                        \
      hipLaunchKernelGGL((odw_grid_kernel<S, L, W, A>), gb, dim3(ODW_GRID_THREADS), glds, ctx->stream, P);     \
    } while (0)
#define ODW_GRID_LAUNCH(S, L, A) do { if (pw) ODW_GRID_LAUNCH_(S, L, true, A); else ODW_GRID_LAUNCH_(S, L, false, A); } while (0)
    // (a scene with an asphere: the item branch's instantiations that know the kind)
    if (P.grid.spheres) { if (P.grid.in_lds) ODW_GRID_LAUNCH(true, true, false); else ODW_GRID_LAUNCH(true, false, false); }
    else if (asph) { if (P.grid.in_lds) ODW_GRID_LAUNCH(false, true, true); else ODW_GRID_LAUNCH(false, false, true); }
    else { if (P.grid.in_lds) ODW_GRID_LAUNCH(false, true, false); else ODW_GRID_LAUNCH(false, false, false); }
#undef ODW_GRID_LAUNCH
#undef ODW_GRID_LAUNCH_
  } else if (use_mesh) {
    const size_t mlds = (size_t)ODW_MESH_STACK * ODW_MESH_THREADS * 2 * sizeof(int) +
                        (size_t)ODW_MESH_BLOCK_WAVES * (ODW_MESH_WAVE_WORDS * sizeof(uint32_t) + ODW_MESH_RING_DOUBLES * sizeof(double));
#define ODW_TRACE_LAUNCH(lds_bytes, ...)                                                                                          \
    do {                                                                                                                        \
      if (pw) hipLaunchKernelGGL((odw_trace_kernel<__VA_ARGS__, false, true>), dim3(grid), dim3(256), lds_bytes, ctx->stream, P); \
      else hipLaunchKernelGGL((odw_trace_kernel<__VA_ARGS__, false, false>), dim3(grid), dim3(256), lds_bytes, ctx->stream, P);   \
    } while (0)
#define ODW_TRACE_LAUNCH_ASPH(lds_bytes, ...)                                                                                     \
    do {                                                                                                                        \
      if (pw) hipLaunchKernelGGL((odw_trace_kernel<__VA_ARGS__, false, true, true>), dim3(grid), dim3(256), lds_bytes, ctx->stream, P); \
      else hipLaunchKernelGGL((odw_trace_kernel<__VA_ARGS__, false, false, true>), dim3(grid), dim3(256), lds_bytes, ctx->stream, P);   \
    } while (0)
    if (stoch) { if (pw) hipLaunchKernelGGL((odw_mesh_kernel<true, true>), dim3(grid), dim3(ODW_MESH_THREADS), mlds, ctx->stream, P);
                 else hipLaunchKernelGGL((odw_mesh_kernel<true, false>), dim3(grid), dim3(ODW_MESH_THREADS), mlds, ctx->stream, P); }
    else { if (pw) hipLaunchKernelGGL((odw_mesh_kernel<false, true>), dim3(grid), dim3(ODW_MESH_THREADS), mlds, ctx->stream, P);
           else hipLaunchKernelGGL((odw_mesh_kernel<false, false>), dim3(grid), dim3(ODW_MESH_THREADS), mlds, ctx->stream, P); }
  } else if (flags & ODW_TRACE_RECORD_SEGMENTS) {
    if (use_tree && asph) {
      if (stoch) ODW_TRACE_LAUNCH_ASPH(lds, true, true, true, false);
      else ODW_TRACE_LAUNCH_ASPH(lds, true, false, true, false);
    } else if (use_tree) {
      if (stoch) ODW_TRACE_LAUNCH(lds, true, true, true, false);
      else ODW_TRACE_LAUNCH(lds, true, false, true, false);
    } else {
      if (stoch) ODW_TRACE_LAUNCH(0, false, true, true, false);
      else ODW_TRACE_LAUNCH(0, false, false, true, false);
    }
  } else if (use_tree && asph) {
    if (stoch) ODW_TRACE_LAUNCH_ASPH(lds, true, true, false, false);
    else ODW_TRACE_LAUNCH_ASPH(lds, true, false, false, false);
  } else if (use_tree) {
    if (stoch) ODW_TRACE_LAUNCH(lds, true, true, false, false);
    else ODW_TRACE_LAUNCH(lds, true, false, false, false);
  } else {
    if (stoch) ODW_TRACE_LAUNCH(0, false, true, false, false);
    else if (ctx->hs.lean) ODW_TRACE_LAUNCH(0, false, false, false, true);
    else ODW_TRACE_LAUNCH(0, false, false, false, false);
  }
#undef ODW_TRACE_LAUNCH
#undef ODW_TRACE_LAUNCH_ASPH
  HIPCHK(ctx, hipGetLastError());
  if (ctx->timing) {
    HIPCHK(ctx, hipEventRecord(ev.second, ctx->stream));
    ctx->events.push_back(ev);
  }
  if (!use_spec) spec_note_launch(ctx, n);
  return ODW_OK;
}

constexpr uint64_t kEmitChunk = 1ull << 24;

// component_major: 3 x n for the trace kernels; else n x 3 (odw_generate_rays hands that to the caller)
int emit_rays(odw_ctx* ctx, uint64_t first, uint64_t n, uint64_t seed, bool component_major = true) {
  int rc;
  if ((rc = ensure(ctx, ctx->em_o, std::min<uint64_t>(n, kEmitChunk) * 3 * sizeof(double)))) return rc;
  if ((rc = ensure(ctx, ctx->em_d, std::min<uint64_t>(n, kEmitChunk) * 3 * sizeof(double)))) return rc;
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (uint64_t)ctx->n_cu * 16));
  hipLaunchKernelGGL(odw_emit_kernel, dim3(grid), dim3(256), 0, ctx->stream, ctx->h_emitter, first, n, seed,
                     (double*)ctx->em_o.p, (double*)ctx->em_d.p, component_major ? n : (uint64_t)1,
                     component_major ? (uint64_t)1 : (uint64_t)3);
  HIPCHK(ctx, hipGetLastError());
  return ODW_OK;
}

}  // namespace

extern "C" {

int odw_abi_version(void) { return ODW_ABI_VERSION; }

const char* odw_last_error(const odw_ctx* ctx) { return ctx ? ctx->err.c_str() : g_error.c_str(); }

namespace {
int ensure_results(odw_ctx* ctx, uint64_t n_bins, uint64_t keep_words) {
  const size_t bins = n_bins > 2 ? (size_t)n_bins : 2;
  const size_t need = (kResultsHead + bins) * sizeof(uint64_t);
  if (!ctx->results.p || ctx->results.bytes < need) {
    DevBuf fresh;
    HIPCHK(ctx, hipMalloc(&fresh.p, need));
    fresh.bytes = need;
    if (ctx->results.p) {            // a launch may still be writing the old block; its counters move over
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
      const size_t keep = std::min((size_t)(kResultsHead + keep_words) * sizeof(uint64_t), ctx->results.bytes);
      HIPCHK(ctx, hipMemcpyAsync(fresh.p, ctx->results.p, keep, hipMemcpyDeviceToDevice, ctx->stream));
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
      release(ctx->results);
    } else {
      HIPCHK(ctx, hipMemsetAsync(fresh.p, 0, kResultsHead * sizeof(uint64_t), ctx->stream));
    }
    ctx->results = fresh;
  }
  ctx->counters.p = ctx->results.p;
  ctx->counters.bytes = ODW_CNT_COUNT * sizeof(uint64_t);
  ctx->hist.p = (uint64_t*)ctx->results.p + kResultsHead;
  ctx->hist.bytes = ctx->results.bytes - kResultsHead * sizeof(uint64_t);
  return ODW_OK;
}
}  // namespace

int odw_create(int device, odw_ctx** out) {
  if (!out) return fail(nullptr, ODW_ERR_INVALID, "odw_create: null out");
  *out = nullptr;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return fail(nullptr, ODW_ERR_DEVICE, std::string("no HIP device: ") + hipGetErrorString(e));
  if (device < 0 || device >= count) return fail(nullptr, ODW_ERR_INVALID, "odw_create: bad device index");
  odw_ctx* ctx = new (std::nothrow) odw_ctx();
  if (!ctx) return fail(nullptr, ODW_ERR_DEVICE, "out of host memory");
  ctx->device = device;
  if (const char* e = getenv("ODW_BVH_THRESHOLD")) ctx->flat_limit = atoi(e);
  if (const char* e = getenv("ODW_SPEC_HOT_RAYS")) ctx->spec_hot_rays = (uint64_t)atof(e);
  std::memset(&ctx->P, 0, sizeof ctx->P);
  ctx->P.wavelength = 500.0;
  std::memset(&ctx->det_desc, 0, sizeof ctx->det_desc);
  std::memset(&ctx->h_source, 0, sizeof ctx->h_source);
  std::memset(&ctx->h_det, 0, sizeof ctx->h_det);
  std::memset(&ctx->h_emitter, 0, sizeof ctx->h_emitter);
  if ((e = hipSetDevice(device)) != hipSuccess || (e = hipStreamCreate(&ctx->stream)) != hipSuccess) {
    fail(nullptr, ODW_ERR_DEVICE, std::string("odw_create: ") + hipGetErrorString(e));
    delete ctx;
    return ODW_ERR_DEVICE;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) ctx->n_cu = prop.multiProcessorCount;
  if (getenv("ODW_GRID_STATS")) {               // diagnostic builds of the grid kernel report here (odw_destroy prints)
    if (ensure(ctx, ctx->dbg, 32 * sizeof(uint64_t)) == ODW_OK) (void)hipMemset(ctx->dbg.p, 0, 32 * sizeof(uint64_t));
  }
  int rc = ensure_results(ctx, 0);
  if (!rc) rc = ensure(ctx, ctx->hit_count, 2 * sizeof(uint64_t));
  if (!rc) rc = ensure(ctx, ctx->chunk_counter, sizeof(uint64_t));
  if (!rc) rc = ensure(ctx, ctx->seg_count, sizeof(uint64_t));
  if (rc) { g_error = ctx->err; odw_destroy(ctx); return rc; }
  (void)hipMemsetAsync(ctx->results.p, 0, ctx->results.bytes, ctx->stream);
  (void)hipMemsetAsync(ctx->hit_count.p, 0, ctx->hit_count.bytes, ctx->stream);
  (void)hipMemsetAsync(ctx->seg_count.p, 0, ctx->seg_count.bytes, ctx->stream);
  *out = ctx;
  return ODW_OK;
}

void odw_destroy(odw_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  batch_unselect(ctx);
  if (ctx->dbg.p) {
    uint64_t v[32] = {0};
    (void)hipMemcpy(v, ctx->dbg.p, sizeof v, hipMemcpyDeviceToHost);
    const char* names[8] = {"A ring fills", "B segment setup", "C cell steps", "D all", "D resolve", "D interact", "candidates", "passed"};
    for (int k = 0; k < 8; ++k)
      fprintf(stderr, "[odw grid stats] %-16s runs %12llu  lanes %14llu  (%.1f per run)\n", names[k], (unsigned long long)v[2 * k],
              (unsigned long long)v[2 * k + 1], v[2 * k] ? (double)v[2 * k + 1] / (double)v[2 * k] : 0.0);
    // (mesh kernel, ODW_MESH_STATS: clock ticks of s_memtime every wave spent in each phase, waits included)
    uint64_t total = 0;
    for (int k = 16; k < 24; ++k) total += v[k];
    const char* phases[8] = {"A refill", "B setup", "C walk", "D leaves", "-", "D interact", "-", "-"};
    if (total)
      for (int k = 0; k < 6; ++k)
        fprintf(stderr, "[odw mesh time] %-16s %14llu ticks  %5.1f %%\n", phases[k], (unsigned long long)v[16 + k], 100.0 * (double)v[16 + k] / (double)total);
    // (flat kernels, ODW_FLAT_STATS: refill + generation / nearest-hit search / interaction and recording)
    if (v[28] + v[29] + v[30])
      for (int k = 0; k < 3; ++k)
        fprintf(stderr, "[odw flat time] %-28s %14llu ticks  %5.1f %%\n", k == 0 ? "refill + generation" : (k == 1 ? "nearest hit" : "interaction + recording"),
                (unsigned long long)v[28 + k], 100.0 * (double)v[28 + k] / (double)(v[28] + v[29] + v[30]));
    // (grid kernel, ODW_GRID_STATS: the same for its phases)
    uint64_t gtotal = 0;
    for (int k = 24; k < 28; ++k) gtotal += v[k];
    const char* gphases[4] = {"A refill", "B setup", "C cell steps", "D resolve+interact"};
    if (gtotal)
      for (int k = 0; k < 4; ++k)
        fprintf(stderr, "[odw grid time] %-18s %14llu ticks  %5.1f %%\n", gphases[k], (unsigned long long)v[24 + k], 100.0 * (double)v[24 + k] / (double)gtotal);
    release(ctx->dbg);
  }
  for (auto& ev : ctx->events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
  for (auto& ev : ctx->free_events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
  DevBuf* all[] = {&ctx->spec_image, &ctx->prim_f64, &ctx->prim_hdr, &ctx->prim_i32, &ctx->cond_i32, &ctx->group_f64, &ctx->group_i32,
                   &ctx->group_gdir, &ctx->seq_mask, &ctx->bvh_nodes, &ctx->bvh_prims, &ctx->bvh_leaf, &ctx->bvh_wide,
                   &ctx->phi_tab, &ctx->t_tab, &ctx->t_guide, &ctx->d_source, &ctx->d_det, &ctx->hits, &ctx->hit_count, &ctx->chunk_counter, &ctx->results,
                   &ctx->ray_o, &ctx->ray_d, &ctx->ray_p, &ctx->ray_aos, &ctx->samp_t, &ctx->samp_phi,
                   &ctx->sort_keys[0], &ctx->sort_keys[1], &ctx->sort_vals[0], &ctx->sort_vals[1],
                   &ctx->sort_tmp, &ctx->sorted_rows, &ctx->segs, &ctx->seg_count};
  for (DevBuf* b : all) release(*b);
  for (DevBuf* b : {&ctx->em_prim_f64, &ctx->em_prim_i32, &ctx->em_cond, &ctx->em_face_i32, &ctx->em_face_cdf,
                    &ctx->em_t_tab, &ctx->em_t_guide, &ctx->em_o, &ctx->em_d, &ctx->em_tri_nrm, &ctx->tri_nrm, &ctx->phi_guide, &ctx->asph})
    release(*b);
  for (DevBuf* b : {&ctx->d_disp_kind, &ctx->d_disp_coef, &ctx->spec_tab, &ctx->ray_wl, &ctx->wl_rays, &ctx->wl_out, &ctx->chroma_nodes,
                    &ctx->chroma_prims, &ctx->d_band_edges, &ctx->d_fresnel_mode, &ctx->fr_in, &ctx->fr_out, &ctx->d_coat_n, &ctx->d_coat, &ctx->coat_layers})
    release(*b);
  for (auto& sb : ctx->surf_bufs) { release(sb.phi_tab); release(sb.t_tab); release(sb.t_guide); }
  release(ctx->d_samplers);
  release(ctx->d_group_sampler);
  for (DevBuf* b : {&ctx->grid_bounds, &ctx->grid_cells, &ctx->grid_items}) release(*b);
  for (DevBuf* b : {&ctx->ph_bitmap, &ctx->ph_before, &ctx->ph_row_of}) release(*b);
  for (DevBuf* b : {&ctx->ph_sel_entering, &ctx->ph_flags, &ctx->ph_x, &ctx->ph_y, &ctx->ph_sorted, &ctx->ph_small,
                    &ctx->ph_part, &ctx->ph_edges, &ctx->ph_edges_b, &ctx->ph_counts, &ctx->ph_sel_hist, &ctx->ph_accel, &ctx->ph_wl})
    release(*b);
  release(ctx->archive);
  release(ctx->archive_count);
  release(ctx->batch_values);
  release(ctx->batch_rays_buf);
  release(ctx->batch_hits);
  release(ctx->batch_hit_count);
  if (ctx->phb_pin_p) (void)hipHostFree(ctx->phb_pin_p);
  if (ctx->up_pin) (void)hipHostFree(ctx->up_pin);
  if (ctx->phb_ev) (void)hipEventDestroy(ctx->phb_ev);
  for (DevBuf* b : {&ctx->phb_row_of, &ctx->phb_words, &ctx->phb_sel, &ctx->phb_small, &ctx->phb_rows, &ctx->phb_x, &ctx->phb_y,
                    &ctx->phb_part, &ctx->phb_sel_hist, &ctx->phb_cand, &ctx->phb_counts, &ctx->phb_scenes, &ctx->phb_hist, &ctx->phb_planes,
                    &ctx->phb_strides, &ctx->phb_origins, &ctx->phb_accel, &ctx->phb_pts})
    release(*b);
  release(ctx->alt_hits);
  release(ctx->alt_hit_count);
  if (ctx->alt_ready) (void)hipEventDestroy(ctx->alt_ready);
  if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}


int odw_upload_scene(odw_ctx* ctx, const odw_scene_desc* s) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_upload_scene: null argument");
  HostScene hs;
  std::string err;
  int rc = scene_host_tables(s, hs, err);
  if (rc) return fail(ctx, rc, err);     // (a refused descriptor leaves the uploaded scene as it was)
  ctx->hs = std::move(hs);
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int n = s->n_prims;
  const std::vector<int32_t>& cond = ctx->hs.cond;
  const std::vector<double>&gf = ctx->hs.group_f64, &gd = ctx->hs.group_gdir;
  const std::vector<int32_t>& gi = ctx->hs.group_i32;
  const std::vector<uint64_t>& seq = ctx->hs.seq;
  if ((rc = upload(ctx, ctx->prim_f64, ctx->hs.prim_f64.data(), ctx->hs.prim_f64.size() * sizeof(double)))) return rc;
  if ((rc = upload(ctx, ctx->prim_i32, ctx->hs.prim_i32.data(), ctx->hs.prim_i32.size() * sizeof(int32_t)))) return rc;
  if ((rc = upload(ctx, ctx->cond_i32, cond.data(), cond.size() * sizeof(int32_t)))) return rc;
  if ((rc = upload(ctx, ctx->group_f64, gf.data(), gf.size() * sizeof(double)))) return rc;
  if ((rc = upload(ctx, ctx->group_i32, gi.data(), gi.size() * sizeof(int32_t)))) return rc;
  if ((rc = upload(ctx, ctx->group_gdir, gd.data(), gd.size() * sizeof(double)))) return rc;
  if ((rc = upload(ctx, ctx->seq_mask, seq.data(), seq.size() * sizeof(uint64_t)))) return rc;
  if (s->tri_normals && n > 0) {
    if ((rc = upload(ctx, ctx->tri_nrm, s->tri_normals, (size_t)n * 9 * sizeof(double)))) return rc;
  }
  // (the asphere table: allocated only when the scene holds one)
  if (!ctx->hs.asph.empty() && (rc = upload(ctx, ctx->asph, ctx->hs.asph.data(), ctx->hs.asph.size() * sizeof(double)))) return rc;
  if ((rc = upload_done(ctx))) return rc;
  ctx->P.asph = ctx->hs.asph.empty() ? nullptr : (const double*)ctx->asph.p;
  DeviceScene& d = ctx->P.scene;
  d.n_prims = ctx->hs.n_prims;
  d.n_groups = ctx->hs.n_groups;
  d.n_nodes = 0;
  d.seq_enabled = ctx->hs.seq_enabled;
  d.seq_len = ctx->hs.seq_len;
  d.all_mask = ctx->hs.all_mask;
  d.ignore_mask = ctx->hs.ignore_mask;
  d.tri_nrm = (s->tri_normals && n > 0) ? (const double*)ctx->tri_nrm.p : nullptr;
  d.prim_f64 = (const double*)ctx->prim_f64.p;
  d.prim_i32 = (const int32_t*)ctx->prim_i32.p;
  d.cond_i32 = (const int32_t*)ctx->cond_i32.p;
  d.group_f64 = (const double*)ctx->group_f64.p;
  d.group_i32 = (const int32_t*)ctx->group_i32.p;
  d.group_gdir = (const double*)ctx->group_gdir.p;
  d.seq_mask = (const uint64_t*)ctx->seq_mask.p;
  ctx->have_scene = true;
  ctx->bvh_dirty = true;
  ctx->spec_dirty = true;
  ctx->spec_fn = nullptr;
  ctx->n_samplers = 0;   // surface samplers belong to the previous scene's groups
  ctx->batch_n = 0;      // an uploaded batch belonged to the previous scene (odw_upload_scene_batch sets it again after this call)
  // ... and so did a dispersion: cleared; the tables just uploaded hold the groups' constants
  ctx->base_ior.assign((size_t)ctx->hs.n_groups, 1.0);
  for (int g = 0; g < ctx->hs.n_groups; ++g) ctx->base_ior[(size_t)g] = ctx->hs.group_f64[4 * (size_t)g];
  ctx->fold_dirty = false;
  ctx->chroma_n_nodes = 0;
  if (ctx->disp_on) {
    ctx->disp_on = false;
    std::memset(ctx->disp_kind, 0, sizeof ctx->disp_kind);
    std::memset(ctx->disp_coef, 0, sizeof ctx->disp_coef);
    if (ctx->d_disp_kind.p && (rc = upload_dispersion(ctx))) return rc;
  }
  // ... and Fresnel modes
  ctx->fresnel_on = ctx->fresnel_split = false;
  std::memset(ctx->fresnel_mode, 0, sizeof ctx->fresnel_mode);
  // ... and coatings
  ctx->coat_on = false;
  std::memset(ctx->coat_n, 0, sizeof ctx->coat_n);
  return ODW_OK;
}

int odw_set_fresnel(odw_ctx* ctx, int32_t n_groups, const int32_t* mode) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_set_fresnel: null ctx");
  if (n_groups == 0) {
    if (!ctx->fresnel_on && !ctx->coat_on) return ODW_OK;
  } else {
    if (!ctx->have_scene) return fail(ctx, ODW_ERR_NO_SCENE, "odw_set_fresnel before odw_upload_scene");
    if (n_groups != ctx->hs.n_groups) return fail(ctx, ODW_ERR_INVALID, "odw_set_fresnel: n_groups is not the scene's");
    std::string err;
    const int rc = fresnel_validate(n_groups, mode, ctx->hs.group_i32.data(), err);
    if (rc) return fail(ctx, rc, err);
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::memset(ctx->fresnel_mode, 0, sizeof ctx->fresnel_mode);
  ctx->fresnel_on = ctx->fresnel_split = false;
  ctx->coat_on = false;                    // (a coating belongs to the modes it was set under: odw_set_coating follows)
  std::memset(ctx->coat_n, 0, sizeof ctx->coat_n);
  for (int g = 0; g < n_groups; ++g) {
    ctx->fresnel_mode[g] = mode[g];
    ctx->fresnel_on |= mode[g] != ODW_FRESNEL_NONE;
    ctx->fresnel_split |= mode[g] == ODW_FRESNEL_SPLIT;
  }
  // (the modes are part of the compiled FRESNEL variant's header: bound again by the next launch that needs it)
  ctx->spec_fresnel_fn[0] = ctx->spec_fresnel_fn[1] = nullptr;
  ctx->spec_fresnel_failed = false;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));        // a running launch may still read the old table
  return upload(ctx, ctx->d_fresnel_mode, ctx->fresnel_mode, sizeof ctx->fresnel_mode);
}

int odw_set_coating(odw_ctx* ctx, int32_t n_groups, const int32_t* n_layers, const double* layers) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_set_coating: null ctx");
  if (n_groups == 0) {
    if (!ctx->coat_on) return ODW_OK;
  } else {
    if (!ctx->have_scene) return fail(ctx, ODW_ERR_NO_SCENE, "odw_set_coating before odw_upload_scene");
    if (n_groups != ctx->hs.n_groups) return fail(ctx, ODW_ERR_INVALID, "odw_set_coating: n_groups is not the scene's");
    std::string err;
    const int rc = coating_validate(n_groups, n_layers, layers, ctx->fresnel_mode, err);
    if (rc) return fail(ctx, rc, err);
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::memset(ctx->coat_n, 0, sizeof ctx->coat_n);
  std::memset(ctx->coat, 0, sizeof ctx->coat);
  ctx->coat_on = false;
  for (int g = 0; g < n_groups; ++g) {
    ctx->coat_n[g] = n_layers[g];
    ctx->coat_on |= n_layers[g] > 0;
    for (int k = 0; k < 2 * n_layers[g]; ++k) ctx->coat[2 * ODW_COAT_LAYERS * (size_t)g + k] = layers[2 * ODW_COAT_LAYERS * (size_t)g + k];
  }
  // (the layer counts are part of the compiled FRESNEL variant's header, the layers of its image: bound again by the next
  //  launch that needs it)
  ctx->spec_fresnel_fn[0] = ctx->spec_fresnel_fn[1] = nullptr;
  ctx->spec_fresnel_failed = false;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));        // a running launch may still read the old tables
  if (!ctx->coat_on) return ODW_OK;
  const int rc = upload(ctx, ctx->d_coat_n, ctx->coat_n, sizeof ctx->coat_n);
  return rc ? rc : upload(ctx, ctx->d_coat, ctx->coat, sizeof ctx->coat);
}

int odw_coating_check(int32_t n_groups, const int32_t* n_layers, const double* layers, const int32_t* mode) {
  std::string err;
  const int rc = coating_validate(n_groups, n_layers, layers, mode, err);
  return rc ? fail(nullptr, rc, err) : ODW_OK;
}

int odw_coated_reflectance(odw_ctx* ctx, double n1, double n2, int32_t entering, int32_t n_layers, const double* layers,
                           double wavelength_nm, uint64_t n, const double* cos_i, double* R, int32_t device) {
  if ((n && (!cos_i || !R)) || (!ctx && device) || !(n1 > 0) || !(n2 > 0) || !std::isfinite(n1) || !std::isfinite(n2) ||
      !(wavelength_nm > 0) || !std::isfinite(wavelength_nm))
    return fail(ctx, ODW_ERR_INVALID, "odw_coated_reflectance: bad argument");
  {
    // (one group's stack: the mode is not asked about)
    double row[2 * ODW_COAT_LAYERS] = {};
    if (n_layers > 0 && n_layers <= ODW_COAT_LAYERS && layers) std::memcpy(row, layers, 2 * (size_t)n_layers * sizeof(double));
    std::string err;
    const int rc = coating_validate(1, &n_layers, n_layers > 0 && !layers ? nullptr : row, nullptr, err);
    if (rc) return fail(ctx, rc, err);
  }
  if (!device) {
    for (uint64_t i = 0; i < n; ++i) R[i] = coated_reflectance(n1, n2, cos_i[i], entering != 0, n_layers, layers, wavelength_nm);
    return ODW_OK;
  }
  if (n == 0) return ODW_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  int rc;
  if ((rc = ensure(ctx, ctx->fr_in, n * sizeof(double)))) return rc;
  if ((rc = ensure(ctx, ctx->fr_out, n * sizeof(double)))) return rc;
  if ((rc = ensure(ctx, ctx->coat_layers, 2 * ODW_COAT_LAYERS * sizeof(double)))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->fr_in.p, cos_i, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (n_layers > 0)
    HIPCHK(ctx, hipMemcpyAsync(ctx->coat_layers.p, layers, 2 * (size_t)n_layers * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (uint64_t)ctx->n_cu * 16));
  hipLaunchKernelGGL(odw_coating_kernel, dim3(grid), dim3(256), 0, ctx->stream, n1, n2, (int)(entering != 0), (int)n_layers,
                     (const double*)ctx->coat_layers.p, wavelength_nm, (const double*)ctx->fr_in.p, n, (double*)ctx->fr_out.p);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(R, ctx->fr_out.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return ODW_OK;
}

int odw_compiled_fresnel_info(odw_ctx* ctx, int32_t* bound) {
  if (!ctx || !bound) return fail(ctx, ODW_ERR_INVALID, "odw_compiled_fresnel_info: bad argument");
  *bound = (ctx->fresnel_on && ctx->spec_fn && (ctx->spec_fresnel_fn[0] || ctx->spec_fresnel_fn[1]) && !ctx->spec_dirty && !ctx->bvh_dirty)
               ? ctx->compile_mode : 0;
  return ODW_OK;
}

int odw_fresnel_check(int32_t n_groups, const int32_t* mode, const int32_t* group_type) {
  std::string err;
  std::vector<int32_t> gi;
  if (group_type && n_groups > 0 && n_groups <= ODW_MAX_GROUPS) {
    gi.assign((size_t)n_groups * 4, 0);
    for (int g = 0; g < n_groups; ++g) gi[4 * (size_t)g] = group_type[g];
  }
  const int rc = fresnel_validate(n_groups, mode, gi.empty() ? nullptr : gi.data(), err);
  return rc ? fail(nullptr, rc, err) : ODW_OK;
}

int odw_fresnel_reflectance(odw_ctx* ctx, double n1, double n2, uint64_t n, const double* cos_i, double* R, int32_t device) {
  if ((n && (!cos_i || !R)) || (!ctx && device) || !(n1 > 0) || !(n2 > 0) || !std::isfinite(n1) || !std::isfinite(n2))
    return fail(ctx, ODW_ERR_INVALID, "odw_fresnel_reflectance: bad argument");
  if (!device) {
    for (uint64_t i = 0; i < n; ++i) R[i] = fresnel_reflectance(n1, n2, cos_i[i]);
    return ODW_OK;
  }
  if (n == 0) return ODW_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  int rc;
  if ((rc = ensure(ctx, ctx->fr_in, n * sizeof(double)))) return rc;
  if ((rc = ensure(ctx, ctx->fr_out, n * sizeof(double)))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->fr_in.p, cos_i, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (uint64_t)ctx->n_cu * 16));
  hipLaunchKernelGGL(odw_fresnel_kernel, dim3(grid), dim3(256), 0, ctx->stream, n1, n2, (const double*)ctx->fr_in.p, n, (double*)ctx->fr_out.p);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(R, ctx->fr_out.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return ODW_OK;
}

namespace {
// odw_compile_check_fresnel, and with n_layers odw_compile_check_coating
int compile_check_fresnel(const char* who, const odw_scene_desc* scene, const odw_limits* limits, const char* arch, const odw_source_desc* source,
                          const int32_t* mode, const int32_t* n_layers, const double* layers, char* header_out, uint64_t header_capacity,
                          uint64_t* code_bytes) {
  if (!scene || !limits || !mode) return fail(nullptr, ODW_ERR_INVALID, std::string(who) + ": bad argument");
  HostScene tmp;
  std::string refusal;
  int rc = scene_host_tables(scene, tmp, refusal);
  if (rc) return fail(nullptr, rc, refusal);
  if ((rc = fresnel_validate(tmp.n_groups, mode, tmp.group_i32.data(), refusal))) return fail(nullptr, rc, refusal);
  if (n_layers && (rc = coating_validate(tmp.n_groups, n_layers, layers, mode, refusal))) return fail(nullptr, rc, refusal);
  std::vector<Box> boxes;
  compute_boxes(tmp, limits->dist_tol, boxes);
  const std::string why = spec_ineligible(tmp);
  if (!why.empty()) return fail(nullptr, ODW_ERR_UNSUPPORTED, std::string(who) + ": " + why);
  const std::string text = spec_text(tmp, 0, nullptr, mode, n_layers) +
      (source ? spec_source_text(spec_source_key(source->xform, source->n_t_rows, true, std::isfinite(source->focal_length))) : "");
  if (header_out && header_capacity) {
    const size_t k = std::min<size_t>(text.size(), (size_t)header_capacity - 1);
    std::memcpy(header_out, text.data(), k);
    header_out[k] = 0;
  }
  std::vector<char> code;
  std::string err;
  if (!spec_compile(text, arch && *arch ? arch : "gfx950", code, err)) return fail(nullptr, ODW_ERR_DEVICE, err);
  if (code_bytes) *code_bytes = code.size();
  return ODW_OK;
}
}  // namespace

int odw_compile_check_fresnel(const odw_scene_desc* scene, const odw_limits* limits, const char* arch, const odw_source_desc* source,
                              const int32_t* mode, char* header_out, uint64_t header_capacity, uint64_t* code_bytes) {
  return compile_check_fresnel("odw_compile_check_fresnel", scene, limits, arch, source, mode, nullptr, nullptr, header_out, header_capacity,
                               code_bytes);
}

int odw_compile_check_coating(const odw_scene_desc* scene, const odw_limits* limits, const char* arch, const odw_source_desc* source,
                              const int32_t* mode, const int32_t* n_layers, const double* layers, char* header_out,
                              uint64_t header_capacity, uint64_t* code_bytes) {
  if (!n_layers) return fail(nullptr, ODW_ERR_INVALID, "odw_compile_check_coating: bad argument");
  return compile_check_fresnel("odw_compile_check_coating", scene, limits, arch, source, mode, n_layers, layers, header_out, header_capacity,
                               code_bytes);
}

int odw_set_dispersion(odw_ctx* ctx, int32_t n_groups, const int32_t* kind, const double* coef) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_set_dispersion: null ctx");
  if (n_groups == 0) {
    if (!ctx->disp_on) return ODW_OK;
  } else {
    if (!ctx->have_scene) return fail(ctx, ODW_ERR_NO_SCENE, "odw_set_dispersion before odw_upload_scene");
    if (n_groups != ctx->hs.n_groups) return fail(ctx, ODW_ERR_INVALID, "odw_set_dispersion: n_groups is not the scene's");
    std::string err;
    const int rc = disp_validate(n_groups, kind, coef, ctx->hs.group_i32.data(), err);
    if (rc) return fail(ctx, rc, err);
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::memset(ctx->disp_kind, 0, sizeof ctx->disp_kind);
  std::memset(ctx->disp_coef, 0, sizeof ctx->disp_coef);
  ctx->disp_on = false;
  for (int g = 0; g < n_groups; ++g) {
    ctx->disp_kind[g] = kind[g];
    if (kind[g]) {
      ctx->disp_on = true;
      std::memcpy(ctx->disp_coef + ODW_DISP_COEFS * g, coef + ODW_DISP_COEFS * g, ODW_DISP_COEFS * sizeof(double));
    }
  }
  ctx->fold_dirty = true;
  // (the groups' formulas are part of the compiled CHROMA variant's header: bound again by the next spectral launch)
  ctx->spec_chroma_fn[0] = ctx->spec_chroma_fn[1] = nullptr;
  ctx->spec_chroma_failed = false;
  ctx->spec_bands_fn[0] = ctx->spec_bands_fn[1] = nullptr;
  ctx->spec_bands_failed = false;
  return upload_dispersion(ctx);
}

int odw_compiled_chroma_info(odw_ctx* ctx, int32_t* bound) {
  if (!ctx || !bound) return fail(ctx, ODW_ERR_INVALID, "odw_compiled_chroma_info: bad argument");
  *bound = (ctx->spec_fn && (ctx->spec_chroma_fn[0] || ctx->spec_chroma_fn[1]) && !ctx->spec_dirty && !ctx->bvh_dirty) ? ctx->compile_mode : 0;
  return ODW_OK;
}

int odw_compiled_bands_info(odw_ctx* ctx, int32_t* bound) {
  if (!ctx || !bound) return fail(ctx, ODW_ERR_INVALID, "odw_compiled_bands_info: bad argument");
  *bound = (ctx->spec_fn && (ctx->spec_bands_fn[0] || ctx->spec_bands_fn[1]) && !ctx->spec_dirty && !ctx->bvh_dirty) ? ctx->compile_mode : 0;
  return ODW_OK;
}

namespace {
// odw_compile_check_chroma (bands = false: its header and kernel as ever) and odw_compile_check_bands
int compile_check_chroma(const odw_scene_desc* scene, const odw_limits* limits, const char* arch, const odw_source_desc* source,
                         const int32_t* disp_kind, bool bands, bool power, char* header_out, uint64_t header_capacity, uint64_t* code_bytes);
}  // namespace

int odw_compile_check_chroma(const odw_scene_desc* scene, const odw_limits* limits, const char* arch, const odw_source_desc* source,
                             const int32_t* disp_kind, char* header_out, uint64_t header_capacity, uint64_t* code_bytes) {
  return compile_check_chroma(scene, limits, arch, source, disp_kind, false, false, header_out, header_capacity, code_bytes);
}

int odw_compile_check_bands(const odw_scene_desc* scene, const odw_limits* limits, const char* arch, const odw_source_desc* source,
                            const int32_t* disp_kind, int32_t power, char* header_out, uint64_t header_capacity, uint64_t* code_bytes) {
  return compile_check_chroma(scene, limits, arch, source, disp_kind, true, power != 0, header_out, header_capacity, code_bytes);
}

namespace {
int compile_check_chroma(const odw_scene_desc* scene, const odw_limits* limits, const char* arch, const odw_source_desc* source,
                         const int32_t* disp_kind, bool bands, bool power, char* header_out, uint64_t header_capacity, uint64_t* code_bytes) {
  if (!scene || !limits || !disp_kind) return fail(nullptr, ODW_ERR_INVALID, "odw_compile_check_chroma: bad argument");
  HostScene tmp;
  std::string refusal;
  int rc = scene_host_tables(scene, tmp, refusal);
  if (rc) return fail(nullptr, rc, refusal);
  std::vector<Box> boxes;
  compute_boxes(tmp, limits->dist_tol, boxes);
  const std::string why = spec_ineligible(tmp);
  if (!why.empty()) return fail(nullptr, ODW_ERR_UNSUPPORTED, "odw_compile_check_chroma: " + why);
  const std::string text = spec_text(tmp, 0, disp_kind, nullptr, nullptr, bands) +
      (source ? spec_source_text(spec_source_key(source->xform, source->n_t_rows, true, std::isfinite(source->focal_length))) : "") +
      (power ? "#define ODW_SPEC_POWER true\n" : "");
  if (header_out && header_capacity) {
    const size_t k = std::min<size_t>(text.size(), (size_t)header_capacity - 1);
    std::memcpy(header_out, text.data(), k);
    header_out[k] = 0;
  }
  std::vector<char> code;
  std::string err;
  if (!spec_compile(text, arch && *arch ? arch : "gfx950", code, err)) return fail(nullptr, ODW_ERR_DEVICE, err);
  if (code_bytes) *code_bytes = code.size();
  return ODW_OK;
}
}  // namespace

int odw_set_spectrum(odw_ctx* ctx, int32_t mode, int32_t n_knots, const double* wavelength_nm, const double* cdf) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_set_spectrum: null ctx");
  if (n_knots == 0) { ctx->spec_n = 0; ctx->spec_mode = 0; return ODW_OK; }
  std::string err;
  int rc = spectrum_validate(mode, n_knots, wavelength_nm, cdf, err);
  if (rc) return fail(ctx, rc, err);
  if (!ctx->have_source || ctx->emitter_active)
    return fail(ctx, ctx->emitter_active ? ODW_ERR_UNSUPPORTED : ODW_ERR_NO_SCENE,
                ctx->emitter_active ? "odw_set_spectrum: surface sources carry no spectrum" : "odw_set_spectrum before odw_upload_source");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::vector<double> tab;
  spectrum_table(n_knots, wavelength_nm, cdf, tab);
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));        // a running launch may still read the old table
  if ((rc = upload(ctx, ctx->spec_tab, tab.data(), tab.size() * sizeof(double)))) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));        // (tab goes out of scope)
  ctx->spec_n = n_knots;
  ctx->spec_mode = mode;
  ctx->spec_lo = wavelength_nm[0];
  ctx->spec_hi = wavelength_nm[n_knots - 1];
  return ODW_OK;
}

int odw_spectrum_check(int32_t mode, int32_t n_knots, const double* wavelength_nm, const double* cdf) {
  std::string err;
  const int rc = spectrum_validate(mode, n_knots, wavelength_nm, cdf, err);
  return rc ? fail(nullptr, rc, err) : ODW_OK;
}

int odw_dispersion_check(int32_t n_groups, const int32_t* kind, const double* coef, double lo_nm, double hi_nm) {
  std::string err;
  int rc = disp_validate(n_groups, kind, coef, nullptr, err);
  if (!rc) rc = disp_check_range(n_groups, kind, coef, lo_nm, hi_nm, err);
  return rc ? fail(nullptr, rc, err) : ODW_OK;
}

int odw_dispersion_index(odw_ctx* ctx, int32_t group, int32_t kind, const double* coef, uint64_t n,
                         const double* wavelength_nm, double* out, int32_t on_device) {
  if ((n && (!wavelength_nm || !out)) || (!ctx && on_device)) return fail(ctx, ODW_ERR_INVALID, "odw_dispersion_index: bad argument");
  double constant = 1.0;
  if (ctx) {
    if (!ctx->have_scene || group < 0 || group >= ctx->hs.n_groups) return fail(ctx, ODW_ERR_INVALID, "odw_dispersion_index: group out of range");
    kind = ctx->disp_kind[group];
    coef = ctx->disp_coef + ODW_DISP_COEFS * group;
    constant = ctx->base_ior[(size_t)group];
  } else {
    int32_t k1 = kind;
    std::string err;
    const int rc = kind == ODW_DISP_NONE ? ODW_ERR_INVALID : disp_validate(1, &k1, coef, nullptr, err);
    if (rc) return fail(nullptr, rc, kind == ODW_DISP_NONE ? "odw_dispersion_index: a glass without a context needs a dispersion kind" : err);
  }
  if (kind == ODW_DISP_NONE) {
    for (uint64_t i = 0; i < n; ++i) out[i] = constant;
    return ODW_OK;
  }
  if (!on_device) {
    for (uint64_t i = 0; i < n; ++i) out[i] = disp_index(kind, coef, wavelength_nm[i]);
    return ODW_OK;
  }
  if (n == 0) return ODW_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));        // (the staging buffers are shared with odw_ray_wavelengths)
  int rc;
  if ((rc = ensure(ctx, ctx->wl_rays, n * sizeof(double)))) return rc;
  if ((rc = ensure(ctx, ctx->wl_out, n * sizeof(double)))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->wl_rays.p, wavelength_nm, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  DispCoefs dc;
  std::memcpy(dc.c, coef, sizeof dc.c);
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (uint64_t)ctx->n_cu * 16));
  hipLaunchKernelGGL(odw_disp_index_kernel, dim3(grid), dim3(256), 0, ctx->stream, (int)kind, dc, (const double*)ctx->wl_rays.p, n,
                     (double*)ctx->wl_out.p);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(out, ctx->wl_out.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return ODW_OK;
}

int odw_ray_wavelengths(odw_ctx* ctx, uint64_t n, const uint64_t* rays, uint64_t seed, double* out) {
  if (!ctx || (n && (!rays || !out))) return fail(ctx, ODW_ERR_INVALID, "odw_ray_wavelengths: bad argument");
  if (ctx->spec_n <= 0) return fail(ctx, ODW_ERR_INVALID, "odw_ray_wavelengths: no spectrum bound (odw_set_spectrum)");
  if (n == 0) return ODW_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  int rc;
  if ((rc = ensure(ctx, ctx->wl_rays, n * sizeof(uint64_t)))) return rc;
  if ((rc = ensure(ctx, ctx->wl_out, n * sizeof(double)))) return rc;
  HIPCHK(ctx, hipMemcpyAsync(ctx->wl_rays.p, rays, n * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (uint64_t)ctx->n_cu * 16));
  hipLaunchKernelGGL(odw_ray_wavelengths_kernel, dim3(grid), dim3(256), 0, ctx->stream, (const double*)ctx->spec_tab.p, (int)ctx->spec_n,
                     (int)ctx->spec_mode, (const uint64_t*)ctx->wl_rays.p, n, seed, (double*)ctx->wl_out.p);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(out, ctx->wl_out.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return ODW_OK;
}

int odw_compile_scene(odw_ctx* ctx, int32_t mode) {
  if (!ctx || mode < ODW_COMPILE_OFF || mode > ODW_COMPILE_AUTO) return fail(ctx, ODW_ERR_INVALID, "odw_compile_scene: bad argument");
  ctx->compile_mode = mode;
  ctx->spec_dirty = true;
  ctx->spec_fn = nullptr;
  ctx->spec_source_key = ctx->source_key;      // (none yet: the source-free kernel; the launch after odw_upload_source binds again)
  if (mode == ODW_COMPILE_OFF || !ctx->have_scene || !ctx->have_limits) return ODW_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (ctx->bvh_dirty) {
    int rc = build_bvh(ctx);
    if (rc) return rc;
  }
  return spec_bind(ctx);
}

int odw_compiled_info(odw_ctx* ctx, int32_t* bound, double* compile_seconds, int32_t* cache_hit) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_compiled_info: null context");
  if (bound) *bound = (ctx->spec_fn && !ctx->spec_dirty && !ctx->bvh_dirty) ? ctx->compile_mode : 0;
  if (compile_seconds) *compile_seconds = ctx->spec_seconds;
  if (cache_hit) *cache_hit = ctx->spec_cache_hit;
  return ODW_OK;
}

int odw_compiled_source_info(odw_ctx* ctx, uint64_t* structure) {
  if (!ctx || !structure) return fail(ctx, ODW_ERR_INVALID, "odw_compiled_source_info: bad argument");
  *structure = (ctx->spec_fn && !ctx->spec_dirty && !ctx->bvh_dirty) ? ctx->spec_source_key : 0;
  return ODW_OK;
}

int odw_compiled_power_info(odw_ctx* ctx, int32_t* bound) {
  if (!ctx || !bound) return fail(ctx, ODW_ERR_INVALID, "odw_compiled_power_info: bad argument");
  *bound = (ctx->spec_fn && ctx->spec_power_fn && !ctx->spec_dirty && !ctx->bvh_dirty) ? ctx->compile_mode : 0;
  return ODW_OK;
}

int odw_compile_check(const odw_scene_desc* scene, const odw_limits* limits, int32_t mode, const char* arch,
                      char* header_out, uint64_t header_capacity, uint64_t* code_bytes) {
  return odw_compile_check_source(scene, limits, mode, arch, nullptr, header_out, header_capacity, code_bytes);
}

// source: the kernel a launch that generates its rays from `source` binds (header with `struct SpecSource`, as
// odw_upload_source keys it: guides present); NULL: the source-free kernel of explicit rays and batches
int odw_compile_check_source(const odw_scene_desc* scene, const odw_limits* limits, int32_t mode, const char* arch,
                             const odw_source_desc* source, char* header_out, uint64_t header_capacity,
                             uint64_t* code_bytes) {
  if (!scene || !limits || mode != ODW_COMPILE_STRUCTURE)
    return fail(nullptr, ODW_ERR_INVALID, "odw_compile_check: bad argument");
  HostScene tmp;
  std::string refusal;
  int rc = scene_host_tables(scene, tmp, refusal);
  if (rc) return fail(nullptr, rc, refusal);
  std::vector<Box> boxes;
  compute_boxes(tmp, limits->dist_tol, boxes);
  const std::string why = spec_ineligible(tmp);
  if (!why.empty()) return fail(nullptr, ODW_ERR_UNSUPPORTED, "odw_compile_check: " + why);
  const std::string text = spec_text(tmp, 0) +
      (source ? spec_source_text(spec_source_key(source->xform, source->n_t_rows, true, std::isfinite(source->focal_length))) : "");
  if (header_out && header_capacity) {
    const size_t k = std::min<size_t>(text.size(), (size_t)header_capacity - 1);
    std::memcpy(header_out, text.data(), k);
    header_out[k] = 0;
  }
  std::vector<char> code;
  std::string err;
  if (!spec_compile(text, arch && *arch ? arch : "gfx950", code, err))
    return fail(nullptr, ODW_ERR_DEVICE, err);
  if (code_bytes) *code_bytes = code.size();
  return ODW_OK;
}

// The value image of a compiled kernel and its layout, without a device: the functions (odw_build.h) a launch of the
// compiled kernel runs, for callers that hold them against the operations written out (tests/test_spec_image.py).
int odw_spec_image(const odw_scene_desc* scene, const odw_limits* limits, double* image, uint64_t image_capacity,
                   uint64_t* image_size, int32_t* offsets, uint64_t offsets_capacity, double* boxes,
                   int32_t* in_arguments) {
  if (!scene || !limits) return fail(nullptr, ODW_ERR_INVALID, "odw_spec_image: null argument");
  if (!(limits->dist_tol > 0) || !(limits->max_ray_length > 0)) return fail(nullptr, ODW_ERR_INVALID, "odw_spec_image: limits out of range");
  HostScene tmp;
  std::string refusal;
  int rc = scene_host_tables(scene, tmp, refusal);
  if (rc) return fail(nullptr, rc, refusal);
  std::vector<Box> built;
  compute_boxes(tmp, limits->dist_tol, built);
  const std::string why = spec_ineligible(tmp);
  if (!why.empty()) return fail(nullptr, ODW_ERR_UNSUPPORTED, "odw_spec_image: " + why);
  const SpecLayout L = spec_image_layout(tmp);
  // (the doubles: the mask of isolated solids, the one word behind them, is no double and not counted)
  if (image_size) *image_size = (uint64_t)L.size;
  if (in_arguments) *in_arguments = L.fits(sizeof(TraceParams)) ? 1 : 0;
  if (image) {
    if (image_capacity < (uint64_t)L.size) return fail(nullptr, ODW_ERR_CAPACITY, "odw_spec_image: image_capacity too small");
    DeviceLimits lim;
    lim.max_ray_length = limits->max_ray_length;
    lim.dist_tol = limits->dist_tol;
    lim.power_tol = limits->power_tol;
    lim.max_intersections = limits->max_intersections;
    std::vector<double> whole((size_t)L.words());
    spec_image_build(tmp, lim, L, whole.data(), nullptr, true);
    // (a caller with room for one word more gets the mask too, as the kernel finds it: 64 bits in image[*image_size])
    std::memcpy(image, whole.data(), (size_t)std::min<uint64_t>(image_capacity, (uint64_t)L.words()) * sizeof(double));
  }
  if (boxes)
    for (int p = 0; p < L.n; ++p) std::memcpy(boxes + 6 * (size_t)p, &tmp.prim_hdr[8 * (size_t)p], 6 * sizeof(double));
  if (offsets) {
    if (offsets_capacity < 3 + 5 * (uint64_t)L.n) return fail(nullptr, ODW_ERR_CAPACITY, "odw_spec_image: offsets_capacity too small");
    offsets[0] = L.gf; offsets[1] = L.gd; offsets[2] = L.gi;
    for (int p = 0; p < L.n; ++p) {
      int32_t* o = offsets + 3 + 5 * p;
      o[0] = L.frame[p]; o[1] = L.par[p]; o[2] = L.box[p]; o[3] = L.der[p]; o[4] = L.box_of[p];
    }
  }
  return ODW_OK;
}

// What a scene will be traced with, and how large its structures are, without a device: descriptor -> HostScene
// (validation, host tables) -> boxes -> SceneAccel, the very functions (odw_build.h) a context runs at its first launch,
// minus the upload.  For callers that want the answer before a GPU is there; the builders themselves run under a CPU
// sanitizer in tests/native/build_tables_main.hip, this entry with the library in tests/test_native_sanitized.py.
// structure: 0 flat loop, 1 grid, 2 binary tree, 3 eight-wide tree (facets) -- the kernel a plain launch takes
// (accel_kind); sizes: [primitives, tree nodes, grid cells, grid items, bytes of dynamic LDS of a grid block,
// dead primitives].
int odw_build_check(const odw_scene_desc* scene, const odw_limits* limits, int32_t* structure, uint64_t* sizes) {
  if (!scene || !limits) return fail(nullptr, ODW_ERR_INVALID, "odw_build_check: null argument");
  if (!(limits->dist_tol > 0) || limits->max_intersections < 0 || !(limits->max_ray_length > 0))
    return fail(nullptr, ODW_ERR_INVALID, "odw_build_check: limits out of range");
  int flat_limit = kBvhThreshold;
  if (const char* e = getenv("ODW_BVH_THRESHOLD")) flat_limit = atoi(e);
  HostScene tmp;
  SceneAccel A;
  std::string err;
  int rc = scene_host_tables(scene, tmp, err);
  if (!rc) {
    std::vector<Box> boxes;
    compute_boxes(tmp, limits->dist_tol, boxes);
    rc = build_accel(tmp, std::move(boxes), limits->dist_tol, flat_limit, build_options(), A, err);
  }
  if (rc) return fail(nullptr, rc, err);
  if (structure) *structure = A.kind();
  if (sizes) {
    uint64_t dead = 0;
    for (char d : tmp.dead) dead += d ? 1 : 0;
    sizes[0] = (uint64_t)tmp.n_prims;
    sizes[1] = (uint64_t)A.nodes.size();
    sizes[2] = (uint64_t)A.grid.nx * (uint64_t)A.grid.ny * (uint64_t)A.grid.nz;
    sizes[3] = (uint64_t)A.grid.n_items;
    sizes[4] = (uint64_t)A.grid.lds_bytes;
    sizes[5] = dead;
  }
  return ODW_OK;
}

// The slopes append_slopes (odw_build.h) puts behind the pairs of an uploaded table, for a caller without a device:
// the same function on the same interleaved layout.
int odw_table_slopes(const double* cdf, const double* edges, int32_t n_tables, int32_t n_knots, double* slopes) {
  if (!cdf || !edges || !slopes || n_tables < 1 || n_knots < 2)
    return fail(nullptr, ODW_ERR_INVALID, "odw_table_slopes: bad argument");
  const size_t nt = (size_t)n_tables, nk = (size_t)n_knots;
  std::vector<double> tab(nt * nk * 2);
  for (size_t t = 0; t < nt; ++t)
    for (size_t j = 0; j < nk; ++j) { tab[2 * (t * nk + j)] = cdf[t * nk + j]; tab[2 * (t * nk + j) + 1] = edges[j]; }
  append_slopes(tab, nt, nk);
  std::memcpy(slopes, tab.data() + 2 * nt * nk, nt * nk * sizeof(double));
  return ODW_OK;
}

// What sample_tables (odw_kernels.hip) takes for granted of an azimuth table, beyond cdf[0] = 0 and cdf[np - 1] = 1:
// nullptr, or what is wrong with it.
//  - The cdf does not decrease: the guide and the binary search both assume a sorted column.
//  - With one theta table per azimuth cell (rows > 1) the edges are those of numpy.linspace(e0, e1, np).  The row of a
//    ray is argmin_i |mid_i - phi| (first minimum); the kernel evaluates that rule on the cell r = floor((phi - e0) /
//    (e1 - e0) * rows) and its two neighbours only.  With U = ulp(max(|e0|, |e1|)), edges within 4 U of e0 + i w
//    (w = (e1 - e0) / rows) and |w| >= 64 U: phi lies in a cell c of the table, so (phi - e0) / w is in [c - 4 U / |w|,
//    c + 1 + 4 U / |w|]; the subtraction adds at most U / |w| to that, the division and the product 3 * 2^-53 * rows
//    (< 1e-6 for any int32 count), so the computed value is within 5/64 + 1e-6 of [c, c + 1] and r is c - 1, c or
//    c + 1.  r = c - 1 only for phi within 9/64 |w| of the edge e_c, where the nearest mid-point is that of c - 1 or of
//    c: both in the window c - 2 .. c; likewise r = c + 1 only next to e_(c+1), nearest mid-point c or c + 1.  For
//    r = c the window c - 1 .. c + 1 holds the nearest mid-point of any phi in cell c.  (mid-points of equidistant
//    cells lie w apart up to 9 U, so no cell further off can win.)  Edges spaced otherwise -- geometrically, say --
//    put the nearest mid-point anywhere: such a table is refused here, not searched there.
static const char* azimuth_table_fault(const double* edges, const double* cdf, size_t np, size_t rows) {
  for (size_t j = 1; j < np; ++j)
    if (!(cdf[j] >= cdf[j - 1])) return "phi_cdf decreases";
  if (rows <= 1) return nullptr;
  const double e0 = edges[0], e1 = edges[np - 1];
  if (!std::isfinite(e0) || !std::isfinite(e1) || e0 == e1)
    return "phi_edges: with one theta table per azimuth cell the edges must be finite and span an interval";
  const double m = std::fmax(std::fabs(e0), std::fabs(e1));
  const double ulp = std::fmax(std::ldexp(1.0, std::ilogb(m) - 52), 4.9406564584124654e-324);
  const double w = (e1 - e0) / (double)(np - 1);
  if (!(std::fabs(w) >= 64.0 * ulp))
    return "phi_edges: with one theta table per azimuth cell the cells must be at least 64 ulp of the larger end wide";
  for (size_t i = 0; i < np; ++i)
    if (!(std::fabs(edges[i] - ((double)i * w + e0)) <= 4.0 * ulp))
      return "phi_edges: with one theta table per azimuth cell the edges must be equidistant (numpy.linspace) within 4 ulp";
  return nullptr;
}

int odw_upload_surface_samplers(odw_ctx* ctx, const odw_surface_sampler_desc* samplers, int32_t n) {
  if (!ctx || n < 0 || (n && !samplers)) return fail(ctx, ODW_ERR_INVALID, "odw_upload_surface_samplers: bad argument");
  if (!ctx->have_scene) return fail(ctx, ODW_ERR_NO_SCENE, "odw_upload_surface_samplers before odw_upload_scene");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (n == 0 && ctx->n_samplers == 0) return ODW_OK;   // (none before, none now: nothing to wait for, nothing to bind again)
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // a running launch may still read the old tables
  ctx->n_samplers = 0;
  ctx->spec_dirty = true;                           // (a compiled scene: the kernel variant with / without scatter())
  if (n == 0) return ODW_OK;
  std::vector<int32_t> gs(ODW_MAX_GROUPS * 2, -1);
  std::vector<DeviceSurfaceSampler> ds((size_t)n);
  if ((int)ctx->surf_bufs.size() < n) ctx->surf_bufs.resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    const odw_surface_sampler_desc& s = samplers[i];
    if (s.group < 0 || s.group >= ctx->P.scene.n_groups || s.kind < ODW_SURF_PRIMARY || s.kind > ODW_SURF_MODIFY)
      return fail(ctx, ODW_ERR_INVALID, "surface sampler: group/kind out of range");
    // several samplers of one (group, kind): told apart by mu (a chain: group_sampler -> first, DeviceSurfaceSampler::next)
    for (int j = gs[2 * s.group + s.kind]; j >= 0; j = ds[(size_t)j].next)
      if (ds[(size_t)j].mu == s.mu) return fail(ctx, ODW_ERR_INVALID, "surface sampler: duplicate (group, kind, mu)");
    if (s.n_atoms < 0 || s.n_atoms > ODW_SURF_MAX_ATOMS || (s.n_atoms && (!s.atom_mass || !s.atom_theta || !s.atom_phi)))
      return fail(ctx, ODW_ERR_INVALID, "surface sampler: atoms");
    for (int k = 0; k < s.n_family * s.n_atoms; ++k)
      if (!(s.atom_mass[k] >= 0.0 && s.atom_mass[k] <= 1.0)) return fail(ctx, ODW_ERR_INVALID, "surface sampler: atom probability outside [0, 1]");
    if (s.n_family < 1 || s.family_axis < ODW_SURF_AXIS_NONE || s.family_axis > ODW_SURF_AXIS_THETA_REFL ||
        (s.family_axis == ODW_SURF_AXIS_NONE && s.n_family != 1) ||
        (s.n_family > 1 && !(s.family_hi > s.family_lo)))
      return fail(ctx, ODW_ERR_INVALID, "surface sampler: family");
    if (s.n_phi_knots < 2 || s.n_t_knots < 2 || s.n_t_rows < 1 ||
        (s.n_t_rows != 1 && s.n_t_rows != s.n_phi_knots - 1))
      return fail(ctx, ODW_ERR_INVALID, "surface sampler: table shape");
    if (!s.phi_edges || !s.phi_cdf || !s.t_edges || !s.t_cdf)
      return fail(ctx, ODW_ERR_INVALID, "surface sampler: null table pointer");
    const size_t np = (size_t)s.n_phi_knots, nt = (size_t)s.n_t_knots, rows = (size_t)s.n_t_rows, nf = (size_t)s.n_family;
    std::vector<double> ptab(nf * np * 2), ttab(nf * rows * nt * 2);
    std::vector<int32_t> guide(nf * rows * (kSurfaceGuide + 1));
    for (size_t k = 0; k < nf; ++k) {
      const double* pc = s.phi_cdf + k * np;
      if (pc[0] != 0.0 || pc[np - 1] != 1.0) return fail(ctx, ODW_ERR_INVALID, "surface sampler: phi cdf must run from 0 to 1");
      if (const char* fault = azimuth_table_fault(s.phi_edges, pc, np, rows))
        return fail(ctx, ODW_ERR_INVALID, std::string("surface sampler: ") + fault);
      for (size_t j = 0; j < np; ++j) {
        ptab[(k * np + j) * 2] = pc[j];
        ptab[(k * np + j) * 2 + 1] = s.phi_edges[j];
      }
      for (size_t r = 0; r < rows; ++r) {
        const double* cdf = s.t_cdf + (k * rows + r) * nt;
        if (cdf[0] != 0.0 || cdf[nt - 1] != 1.0) return fail(ctx, ODW_ERR_INVALID, "surface sampler: theta cdf rows must run from 0 to 1");
        double* dst = ttab.data() + (k * rows + r) * nt * 2;
        for (size_t j = 0; j < nt; ++j) {
          if (j && cdf[j] < cdf[j - 1]) return fail(ctx, ODW_ERR_INVALID, "surface sampler: cdf not monotone");
          dst[2 * j] = cdf[j];
          dst[2 * j + 1] = s.t_edges[j];
        }
        int32_t* g = guide.data() + (k * rows + r) * (kSurfaceGuide + 1);
        size_t j = 0;
        for (int q = 0; q <= kSurfaceGuide; ++q) {
          const double x = (double)q / (double)kSurfaceGuide;
          while (j + 1 < nt && cdf[j + 1] <= x) ++j;
          g[q] = (int32_t)j;
        }
      }
    }
    append_slopes(ptab, nf, np);
    append_slopes(ttab, nf * rows, nt);
    odw_ctx::SurfaceBufs& sb = ctx->surf_bufs[(size_t)i];
    int rc;
    if ((rc = upload(ctx, sb.phi_tab, ptab.data(), ptab.size() * sizeof(double)))) return rc;
    if ((rc = upload(ctx, sb.t_tab, ttab.data(), ttab.size() * sizeof(double)))) return rc;
    if ((rc = upload(ctx, sb.t_guide, guide.data(), guide.size() * sizeof(int32_t)))) return rc;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // staging vectors go out of scope
    DeviceSurfaceSampler& d = ds[(size_t)i];
    d.phi_tab = (const double*)sb.phi_tab.p;
    d.t_tab = (const double*)sb.t_tab.p;
    d.t_guide = (const int32_t*)sb.t_guide.p;
    d.n_phi_knots = s.n_phi_knots;
    d.n_t_knots = s.n_t_knots;
    d.n_t_rows = s.n_t_rows;
    d.n_guide = kSurfaceGuide;
    d.axis = s.family_axis;
    d.n_family = s.n_family;
    d.lo = s.family_lo;
    d.inv_step = s.n_family > 1 ? (double)(s.n_family - 1) / (s.family_hi - s.family_lo) : 0.0;
    d.mu = s.mu;
    d.n_atoms = s.n_atoms;
    d.atom_mass = nullptr;
    std::memset(d.atom_theta, 0, sizeof d.atom_theta);
    std::memset(d.atom_phi, 0, sizeof d.atom_phi);
    if (s.n_atoms) {
      if ((rc = upload(ctx, sb.atom_mass, s.atom_mass, (size_t)s.n_family * (size_t)s.n_atoms * sizeof(double)))) return rc;
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
      d.atom_mass = (const double*)sb.atom_mass.p;
      for (int j = 0; j < s.n_atoms; ++j)
        for (int c = 0; c < 3; ++c) { d.atom_theta[j][c] = s.atom_theta[3 * j + c]; d.atom_phi[j][c] = s.atom_phi[3 * j + c]; }
    }
    d.next = gs[2 * s.group + s.kind];       // (the chain runs from the last one uploaded to the first)
    gs[2 * s.group + s.kind] = i;
  }
  int rc;
  if ((rc = upload(ctx, ctx->d_samplers, ds.data(), ds.size() * sizeof(DeviceSurfaceSampler)))) return rc;
  if ((rc = upload(ctx, ctx->d_group_sampler, gs.data(), gs.size() * sizeof(int32_t)))) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->n_samplers = n;
  return ODW_OK;
}

int odw_set_wavelength(odw_ctx* ctx, double wavelength_nm) {
  if (!ctx || !(wavelength_nm > 0)) return fail(ctx, ODW_ERR_INVALID, "odw_set_wavelength: bad argument");
  ctx->P.wavelength = wavelength_nm;
  return ODW_OK;
}

int odw_set_surface_seed(odw_ctx* ctx, uint64_t seed) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_set_surface_seed: null ctx");
  ctx->surface_seed = seed;
  return ODW_OK;
}

static int upload_source(odw_ctx* ctx, const odw_source_desc* s, bool guides);

int odw_upload_source(odw_ctx* ctx, const odw_source_desc* s) { return upload_source(ctx, s, true); }

int odw_upload_source_unguided(odw_ctx* ctx, const odw_source_desc* s) { return upload_source(ctx, s, false); }

// guides = false: no azimuth guide and a theta guide of one cell, i.e. plain binary searches over the whole tables --
// the same knots are found, the same rays come out (odw_upload_source_unguided, tests/test_gpu_spec_source.py)
static int upload_source(odw_ctx* ctx, const odw_source_desc* s, bool guides) {
  if (!ctx || !s) return fail(ctx, ODW_ERR_INVALID, "odw_upload_source: null argument");
  if (s->n_phi_knots < 2 || s->n_t_knots < 2 || s->n_t_rows < 1 ||
      (s->n_t_rows != 1 && s->n_t_rows != s->n_phi_knots - 1))
    return fail(ctx, ODW_ERR_INVALID, "odw_upload_source: table shape");
  if (!s->phi_edges || !s->phi_cdf || !s->t_edges || !s->t_cdf)
    return fail(ctx, ODW_ERR_INVALID, "odw_upload_source: null table pointer");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const int np = s->n_phi_knots, nt = s->n_t_knots, rows = s->n_t_rows;
  if (s->phi_cdf[0] != 0.0 || s->phi_cdf[np - 1] != 1.0)
    return fail(ctx, ODW_ERR_INVALID, "phi cdf must run from 0 to 1");
  if (const char* fault = azimuth_table_fault(s->phi_edges, s->phi_cdf, (size_t)np, (size_t)rows))
    return fail(ctx, ODW_ERR_INVALID, std::string("odw_upload_source: ") + fault);
  std::vector<double> ptab((size_t)np * 2), ttab((size_t)rows * nt * 2);
  for (int i = 0; i < np; ++i) { ptab[2 * i] = s->phi_cdf[i]; ptab[2 * i + 1] = s->phi_edges[i]; }
  const int n_guide = guides ? kGuide : 1;
  std::vector<int32_t> guide((size_t)rows * (n_guide + 1));
  for (int r = 0; r < rows; ++r) {
    const double* cdf = s->t_cdf + (size_t)r * nt;
    if (cdf[0] != 0.0 || cdf[nt - 1] != 1.0) return fail(ctx, ODW_ERR_INVALID, "theta cdf rows must run from 0 to 1");
    double* dst = ttab.data() + (size_t)r * nt * 2;
    for (int i = 0; i < nt; ++i) {
      if (i && cdf[i] < cdf[i - 1]) return fail(ctx, ODW_ERR_INVALID, "cdf not monotone");
      dst[2 * i] = cdf[i];
      dst[2 * i + 1] = s->t_edges[i];
    }
    // guide[k] = last knot with cdf <= k/G: brackets the search for any u in
    // [k/G, (k+1)/G) without changing which knot is found
    int32_t* g = guide.data() + (size_t)r * (n_guide + 1);
    int j = 0;
    for (int k = 0; k <= n_guide; ++k) {
      const double x = (double)k / (double)n_guide;
      while (j + 1 < nt && cdf[j + 1] <= x) ++j;
      g[k] = j;
    }
  }
  append_slopes(ptab, 1, (size_t)np);
  append_slopes(ttab, (size_t)rows, (size_t)nt);
  int rc;
  if ((rc = upload(ctx, ctx->phi_tab, ptab.data(), ptab.size() * sizeof(double)))) return rc;
  if ((rc = upload(ctx, ctx->t_tab, ttab.data(), ttab.size() * sizeof(double)))) return rc;
  if ((rc = upload(ctx, ctx->t_guide, guide.data(), guide.size() * sizeof(int32_t)))) return rc;
  std::vector<int32_t> pguide(kPhiGuide + 1);
  for (int k = 0, j = 0; k <= kPhiGuide; ++k) {
    const double x = (double)k / (double)kPhiGuide;
    while (j + 1 < np && s->phi_cdf[j + 1] <= x) ++j;
    pguide[k] = j;
  }
  if ((rc = upload(ctx, ctx->phi_guide, pguide.data(), pguide.size() * sizeof(int32_t)))) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  DeviceSource& d = ctx->h_source;
  std::memcpy(d.m, s->xform, sizeof d.m);
  d.focal_length = s->focal_length;
  d.finite_focal = std::isfinite(s->focal_length) ? 1 : 0;
  d.wavelength = s->wavelength;
  d.power = s->power;
  d.phi_tab = (const double*)ctx->phi_tab.p;
  d.t_tab = (const double*)ctx->t_tab.p;
  d.t_guide = (const int32_t*)ctx->t_guide.p;
  d.phi_guide = guides ? (const int32_t*)ctx->phi_guide.p : nullptr;
  d.n_phi_guide = guides ? kPhiGuide : 0;
  d.n_phi_knots = np;
  d.n_t_knots = nt;
  d.n_t_rows = rows;
  d.n_guide = n_guide;
  if ((rc = upload(ctx, ctx->d_source, &ctx->h_source, sizeof(DeviceSource)))) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->P.source = (const DeviceSource*)ctx->d_source.p;
  ctx->P.wavelength = s->wavelength;
  ctx->have_source = true;
  ctx->emitter_active = false;
  ctx->spec_n = ctx->spec_mode = 0;        // (a spectrum belonged to the previous source)
  ctx->source_key = spec_source_key(ctx->h_source);
  if (ctx->spec_source_key && ctx->spec_source_key != ctx->source_key) ctx->spec_dirty = true;   // a source of another structure
  return ODW_OK;
}

int odw_upload_surface_source(odw_ctx* ctx, const odw_surface_source_desc* s) {
  if (!ctx || !s) return fail(ctx, ODW_ERR_INVALID, "odw_upload_surface_source: null argument");
  if (s->n_prims < 1 || s->n_faces < 1 || s->n_conds < 0 || s->n_t_knots < 2 || !(s->dist_tol > 0))
    return fail(ctx, ODW_ERR_INVALID, "odw_upload_surface_source: counts out of range");
  if (!s->prim_type || !s->prim_flags || !s->prim_xform || !s->prim_params || !s->prim_cond_off || !s->face_prim ||
      !s->face_id || !s->face_area || !s->t_edges || !s->t_cdf || (s->n_conds > 0 && (!s->cond_prim || !s->cond_inside)))
    return fail(ctx, ODW_ERR_INVALID, "odw_upload_surface_source: null table pointer");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  const int n = s->n_prims;
  std::vector<double> pf((size_t)n * 16);
  std::vector<int32_t> pi((size_t)n * 4);
  for (int p = 0; p < n; ++p) {
    if (s->prim_type[p] < ODW_PRIM_BOX || s->prim_type[p] > ODW_PRIM_ASPHERE)
      return fail(ctx, ODW_ERR_UNSUPPORTED, "surface source: unknown primitive kind");
    // (nor asphere code)
    if (s->prim_type[p] == ODW_PRIM_ASPHERE)
      return fail(ctx, ODW_ERR_UNSUPPORTED, "surface source: an asphere is not built, neither as emitting faces nor as a trimming operand");
    // (nor conicoid code: the emitter rides along in every compiled code object and stays what it is)
    if (s->prim_type[p] == ODW_PRIM_CONICOID)
      return fail(ctx, ODW_ERR_UNSUPPORTED, "surface source: a conicoid is not built, neither as emitting faces nor as a trimming operand");
    // (the emitter kernel carries no ellipsoid code: neither an emitting face nor an operand of a trimming list)
    if (s->prim_type[p] == ODW_PRIM_ELLIPSOID)
      return fail(ctx, ODW_ERR_UNSUPPORTED, "surface source: ellipsoids are not built, neither as emitting faces nor as trimming operands");
    const int off = s->prim_cond_off[p], cnt = s->prim_cond_off[p + 1] - off;
    if (s->prim_type[p] == ODW_PRIM_TRIANGLE && cnt != 0)
      return fail(ctx, ODW_ERR_INVALID, "surface source: facets cannot carry trimming conditions");
    if (off < 0 || cnt < 0 || off + cnt > s->n_conds) return fail(ctx, ODW_ERR_INVALID, "surface source: bad condition offsets");
    std::memcpy(&pf[16 * (size_t)p], s->prim_xform + 12 * (size_t)p, 12 * sizeof(double));
    std::memcpy(&pf[16 * (size_t)p + 12], s->prim_params + 4 * (size_t)p, 4 * sizeof(double));
    pi[4 * p] = s->prim_type[p];
    pi[4 * p + 1] = s->prim_flags[p];
    pi[4 * p + 2] = off;
    pi[4 * p + 3] = cnt;
  }
  std::vector<int32_t> cond((size_t)std::max(1, s->n_conds), 0);
  for (int c = 0; c < s->n_conds; ++c) {
    if (s->cond_prim[c] < 0 || s->cond_prim[c] >= n || s->cond_prim[c] >= (1 << 30) ||
        s->prim_type[s->cond_prim[c]] == ODW_PRIM_TRIANGLE)
      return fail(ctx, ODW_ERR_INVALID, "surface source: condition primitive out of range");
    if (s->cond_inside[c] < 0 || s->cond_inside[c] > 3)
      return fail(ctx, ODW_ERR_INVALID, "surface source: cond_inside: bit 0 inside, bit 1 opens a clause; nothing else");
    cond[c] = pack_cond(s->cond_prim[c], s->cond_inside[c]);
  }
  if (!clauses_marked(s->prim_cond_off, n, cond))
    return fail(ctx, ODW_ERR_INVALID, "surface source: a trimming list of several clauses must mark its first condition too");
  static const int n_faces_of[10] = {6, 1, 3, 3, 1, 1, 0, 0, 0, 0};  // (paraboloid faces do not emit: rejected below; ellipsoids, conicoids, aspheres: above)
  std::vector<int32_t> fi((size_t)s->n_faces * 2);
  std::vector<double> fc((size_t)s->n_faces + 1, 0.0);
  double total = 0;
  for (int f = 0; f < s->n_faces; ++f) {
    const int p = s->face_prim[f];
    if (p < 0 || p >= n || s->face_id[f] < 0 || s->face_id[f] >= n_faces_of[s->prim_type[p]] || !(s->face_area[f] >= 0))
      return fail(ctx, ODW_ERR_INVALID, "surface source: face out of range");
    fi[2 * f] = p;
    fi[2 * f + 1] = s->face_id[f];
    total += s->face_area[f];
  }
  if (!(total > 0)) return fail(ctx, ODW_ERR_INVALID, "surface source: emitting faces have no area");
  double run = 0;
  for (int f = 0; f < s->n_faces; ++f) { run += s->face_area[f]; fc[f + 1] = run / total; }
  fc[s->n_faces] = 1.0;
  const int nt = s->n_t_knots;
  if (s->t_cdf[0] != 0.0 || s->t_cdf[nt - 1] != 1.0) return fail(ctx, ODW_ERR_INVALID, "surface source: theta cdf must run from 0 to 1");
  std::vector<double> ttab((size_t)nt * 2);
  for (int i = 0; i < nt; ++i) {
    if (i && s->t_cdf[i] < s->t_cdf[i - 1]) return fail(ctx, ODW_ERR_INVALID, "surface source: cdf not monotone");
    ttab[2 * i] = s->t_cdf[i];
    ttab[2 * i + 1] = s->t_edges[i];
  }
  append_slopes(ttab, 1, (size_t)nt);
  std::vector<int32_t> guide((size_t)kGuide + 1);
  for (int k = 0, j = 0; k <= kGuide; ++k) {
    const double x = (double)k / (double)kGuide;
    while (j + 1 < nt && s->t_cdf[j + 1] <= x) ++j;
    guide[k] = j;
  }
  int rc;
  if ((rc = upload(ctx, ctx->em_prim_f64, pf.data(), pf.size() * sizeof(double)))) return rc;
  if ((rc = upload(ctx, ctx->em_prim_i32, pi.data(), pi.size() * sizeof(int32_t)))) return rc;
  if ((rc = upload(ctx, ctx->em_cond, cond.data(), cond.size() * sizeof(int32_t)))) return rc;
  if ((rc = upload(ctx, ctx->em_face_i32, fi.data(), fi.size() * sizeof(int32_t)))) return rc;
  if ((rc = upload(ctx, ctx->em_face_cdf, fc.data(), fc.size() * sizeof(double)))) return rc;
  if ((rc = upload(ctx, ctx->em_t_tab, ttab.data(), ttab.size() * sizeof(double)))) return rc;
  if ((rc = upload(ctx, ctx->em_t_guide, guide.data(), guide.size() * sizeof(int32_t)))) return rc;
  if (s->tri_normals && (rc = upload(ctx, ctx->em_tri_nrm, s->tri_normals, (size_t)n * 9 * sizeof(double)))) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  DeviceEmitter& e = ctx->h_emitter;
  e.tri_nrm = s->tri_normals ? (const double*)ctx->em_tri_nrm.p : nullptr;
  e.prim_f64 = (const double*)ctx->em_prim_f64.p;
  e.prim_i32 = (const int32_t*)ctx->em_prim_i32.p;
  e.cond_i32 = (const int32_t*)ctx->em_cond.p;
  e.face_i32 = (const int32_t*)ctx->em_face_i32.p;
  e.face_cdf = (const double*)ctx->em_face_cdf.p;
  e.t_tab = (const double*)ctx->em_t_tab.p;
  e.t_guide = (const int32_t*)ctx->em_t_guide.p;
  e.n_faces = s->n_faces;
  e.n_t_knots = nt;
  e.n_guide = kGuide;
  e.dist_tol = s->dist_tol;
  e.wavelength = s->wavelength;
  e.power = s->power;
  ctx->P.wavelength = s->wavelength;
  ctx->have_source = true;
  ctx->emitter_active = true;
  ctx->spec_n = ctx->spec_mode = 0;        // (a spectrum belonged to the previous source; surface sources carry none)
  ctx->source_key = 0;                   // (emitted rays reach the trace kernels through buffers, like explicit ones)
  return ODW_OK;
}

int odw_generate_rays(odw_ctx* ctx, uint64_t first_ray, uint64_t n_rays, uint64_t seed, double* origins,
                      double* directions) {
  if (!ctx || !origins || !directions) return fail(ctx, ODW_ERR_INVALID, "odw_generate_rays: bad argument");
  if (!ctx->have_source) return fail(ctx, ODW_ERR_NO_SCENE, "source not uploaded");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  for (uint64_t off = 0; off < n_rays; off += kEmitChunk) {
    const uint64_t m = std::min<uint64_t>(kEmitChunk, n_rays - off);
    int rc;
    if (ctx->emitter_active) {
      if ((rc = emit_rays(ctx, first_ray + off, m, seed, false))) return rc;
    } else {
      if ((rc = ensure(ctx, ctx->em_o, m * 3 * sizeof(double)))) return rc;
      if ((rc = ensure(ctx, ctx->em_d, m * 3 * sizeof(double)))) return rc;
      const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((m + 255) / 256, (uint64_t)ctx->n_cu * 16));
      hipLaunchKernelGGL(odw_make_rays_kernel, dim3(grid), dim3(256), 0, ctx->stream, ctx->P.source, first_ray + off,
                         m, seed, (double*)ctx->em_o.p, (double*)ctx->em_d.p);
      HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipMemcpyAsync(origins + 3 * off, ctx->em_o.p, m * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(directions + 3 * off, ctx->em_d.p, m * 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return ODW_OK;
}

int odw_set_limits(odw_ctx* ctx, const odw_limits* l) {
  if (!ctx || !l) return fail(ctx, ODW_ERR_INVALID, "odw_set_limits: null argument");
  if (!(l->dist_tol > 0) || l->max_intersections < 0 || !(l->max_ray_length > 0))
    return fail(ctx, ODW_ERR_INVALID, "odw_set_limits: values out of range");
  if (!ctx->have_limits || ctx->P.lim.dist_tol != l->dist_tol) {
    ctx->bvh_dirty = true;   // (the boxes carry the tolerance; a compiled scene is bound again after the rebuild)
    ctx->batch_n = 0;        // (and so do the boxes of an uploaded batch: it has to be uploaded again)
  }
  ctx->P.lim.max_ray_length = l->max_ray_length;
  ctx->P.lim.max_intersections = l->max_intersections;
  ctx->P.lim.dist_tol = l->dist_tol;
  ctx->P.lim.power_tol = l->power_tol;
  ctx->have_limits = true;
  return ODW_OK;
}

int odw_set_detector(odw_ctx* ctx, const odw_detector_desc* det) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_set_detector: null ctx");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  DeviceDetector& d = ctx->h_det;
  ctx->power_on = false;                 // (the power plane belongs to one detector: enabled again after every call)
  ctx->band_n = 0;                       // (... and so do the band planes)
  if (!det) { d.enabled = 0; ctx->P.det_enabled = 0; ctx->n_bins = 0; return ODW_OK; }
  if (det->nx <= 0 || det->ny <= 0 || !(det->x_hi > det->x_lo) || !(det->y_hi > det->y_lo))
    return fail(ctx, ODW_ERR_INVALID, "odw_set_detector: bad window");
  ctx->det_desc = *det;
  for (int k = 0; k < 3; ++k) { d.origin[k] = det->origin[k]; d.ex[k] = det->ex[k]; d.ey[k] = det->ey[k]; }
  d.x_lo = det->x_lo;
  d.y_lo = det->y_lo;
  d.x_scale = det->nx / (det->x_hi - det->x_lo);
  d.y_scale = det->ny / (det->y_hi - det->y_lo);
  d.nx = det->nx;
  d.ny = det->ny;
  d.nx_f = (double)det->nx;
  d.ny_f = (double)det->ny;
  d.group = det->group;
  d.enabled = 1;
  ctx->n_bins = (uint64_t)det->nx * (uint64_t)det->ny;
  int rc = ensure_results(ctx, ctx->n_bins);
  if (rc) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // a running launch may still read the old block
  if ((rc = upload(ctx, ctx->d_det, &ctx->h_det, sizeof(DeviceDetector)))) return rc;
  ctx->P.det = (const DeviceDetector*)ctx->d_det.p;
  ctx->P.det_enabled = 1;
  HIPCHK(ctx, hipMemsetAsync(ctx->hist.p, 0, ctx->n_bins * sizeof(uint64_t), ctx->stream));
  return ODW_OK;
}

int odw_reserve_hits(odw_ctx* ctx, uint64_t capacity) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_reserve_hits: null ctx");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  batch_unselect(ctx);
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (capacity == 0) { release(ctx->hits); ctx->hit_capacity = ctx->hit_slots = 0; return ODW_OK; }
  if (capacity > ctx->hit_capacity) {
    release(ctx->hits);
    ctx->hit_capacity = ctx->hit_slots = 0;
    // big lists get slack for block reservations (launch_trace): an eighth (unused slots at block
    // changes) + one block per wave of the largest grid
    uint64_t slots = capacity;
    // (a short list is filled by short launches: a wave per 256 rows, the largest grid at most)
    if (capacity >= kHitBlockMinRows)
      slots += hit_block_room(capacity, std::min<uint64_t>((uint64_t)ctx->n_cu * 8 * 4, std::max<uint64_t>(64, capacity / 256)), kHitBlock);
    int rc = ensure(ctx, ctx->hits, slots * sizeof(odw_hit));
    if (rc) return rc;
    ctx->hit_capacity = capacity;
    ctx->hit_slots = slots;
    // a new buffer: rows recorded so far are gone
    HIPCHK(ctx, hipMemsetAsync(ctx->hit_count.p, 0, 2 * sizeof(uint64_t), ctx->stream));
  }
  return ODW_OK;
}

int odw_reserve_segments(odw_ctx* ctx, uint64_t capacity) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_reserve_segments: null ctx");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  if (capacity == 0) { release(ctx->segs); ctx->seg_capacity = 0; return ODW_OK; }
  if (capacity > 0x7FFFFFFFull) return fail(ctx, ODW_ERR_CAPACITY, "odw_reserve_segments: more than 2^31 rows");
  if (capacity > ctx->seg_capacity) {
    release(ctx->segs);
    ctx->seg_capacity = 0;
    int rc = ensure(ctx, ctx->segs, capacity * sizeof(odw_segment));
    if (rc) return rc;
    ctx->seg_capacity = capacity;
    HIPCHK(ctx, hipMemsetAsync(ctx->seg_count.p, 0, sizeof(uint64_t), ctx->stream));
  }
  return ODW_OK;
}

int odw_trace(odw_ctx* ctx, uint64_t first_ray, uint64_t n_rays, uint64_t seed, uint32_t flags) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_trace: null ctx");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  batch_unselect(ctx);
  if (!ctx->emitter_active) return launch_trace(ctx, first_ray, n_rays, seed, flags, nullptr, nullptr, nullptr);
  // surface source: initial conditions are generated into a staging buffer,
  // kEmitChunk rays at a time, and traced as explicit rays (same stream: the
  // next chunk's generation waits for the previous chunk's trace)
  for (uint64_t off = 0; off < n_rays; off += kEmitChunk) {
    const uint64_t m = std::min<uint64_t>(kEmitChunk, n_rays - off);
    int rc = emit_rays(ctx, first_ray + off, m, seed);
    if (rc) return rc;
    rc = launch_trace(ctx, first_ray + off, m, seed, flags, (const double*)ctx->em_o.p,
                      (const double*)ctx->em_d.p, nullptr);
    if (rc) return rc;
  }
  return ODW_OK;
}

// ---- batches: scenes of one structure in one launch (v9) ---------------------------------------------------------
namespace {
void batch_unselect(odw_ctx* ctx) {
  if (ctx->batch_selected < 0 && !ctx->archive_selected) return;
  ctx->archive_selected = false;
  ctx->hits = ctx->own_hits;
  ctx->hit_count = ctx->own_hit_count;
  ctx->hit_capacity = ctx->own_capacity;
  ctx->hit_slots = ctx->own_slots;
  ctx->hit_ray_begin = ctx->own_ray_begin;
  ctx->hit_ray_end = ctx->own_ray_end;
  ctx->own_hits = DevBuf();
  ctx->own_hit_count = DevBuf();
  ctx->batch_selected = -1;
  ctx->ph_valid = false;
}

// the part of a scene's host tables that is STRUCTURE (what scenes of a batch must share)
bool same_structure(const HostScene& a, const HostScene& b, std::string& why) {
  if (a.n_prims != b.n_prims || a.n_groups != b.n_groups) { why = "primitive or group count"; return false; }
  for (size_t i = 0; i < a.prim_i32.size(); ++i) {
    const int32_t mask = (i % 4 == 2) ? ~(int32_t)ODW_FLAG_ISOLATED : ~0;       // (a matter of the boxes' values)
    if ((a.prim_i32[i] & mask) != (b.prim_i32[i] & mask)) { why = "primitive kinds, groups, flags or trimming lists"; return false; }
  }
  if (a.cond != b.cond) { why = "trimming conditions"; return false; }
  if (a.group_i32 != b.group_i32) { why = "optical types / recording switches / grating kinds"; return false; }
  if (a.seq != b.seq || a.seq_enabled != b.seq_enabled || a.seq_len != b.seq_len || a.ignore_mask != b.ignore_mask) { why = "tracing sequence / ignored groups"; return false; }
  if (a.lean != b.lean) { why = "gratings or absorbing media in some scenes only"; return false; }
  return true;
}
}  // namespace

int odw_upload_scene_batch(odw_ctx* ctx, const odw_scene_desc* scenes, int32_t n_scenes) {
  if (!ctx || !scenes || n_scenes < 1) return fail(ctx, ODW_ERR_INVALID, "odw_upload_scene_batch: bad argument");
  if (!ctx->have_limits) return fail(ctx, ODW_ERR_NO_SCENE, "odw_upload_scene_batch before odw_set_limits (the boxes carry the tolerance)");
  if (ctx->fresnel_on)
    return fail(ctx, ODW_ERR_UNSUPPORTED, "odw_upload_scene_batch: a batch with a Fresnel mode set (per-scene Fresnel modes are out of scope; "
                                          "odw_set_fresnel with n_groups = 0 clears it)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  ctx->batch_n = 0;
  ctx->batch_traced = 0;
  ctx->batch_rows_ok = false;
  ctx->phb_valid = ctx->phb_projected = false;
  // scene 0 becomes the context's scene (shared integer tables, kernel choice, the compiled kernel's structure)
  int rc = odw_upload_scene(ctx, &scenes[0]);
  if (rc) return rc;
  if ((rc = build_bvh(ctx))) return rc;
  const bool compiled = ctx->compile_mode != ODW_COMPILE_OFF && spec_ineligible(ctx->hs).empty();
  // (a scene that has structures only because of its paraboloids or ellipsoids: the generic flat kernel does not know
  //  them, the kernel compiled against the scene does -- such a batch needs ODW_COMPILE_STRUCTURE, which binds it before
  //  the launch)
  const bool rare_compiled = flat_but_for_rare_quadrics(ctx->hs, ctx->flat_limit) && compiled && ctx->compile_mode == ODW_COMPILE_STRUCTURE;
  if ((ctx->P.scene.n_nodes || ctx->P.grid.nx > 0) && !rare_compiled)
    return fail(ctx, ODW_ERR_UNSUPPORTED, "odw_upload_scene_batch: batches are traced by the flat kernels (analytic scenes of up to 64 primitives; "
                                          "with paraboloids, ellipsoids, conicoids or aspheres: by the compiled one, ODW_COMPILE_STRUCTURE)");
  // (the header text of a scene a compiled kernel could take, whatever the mode is now: it also says whether the
  //  scenes share the layout of the value image)
  const bool eligible = spec_ineligible(ctx->hs).empty();
  const std::string text0 = eligible ? spec_text(ctx->hs, ctx->n_samplers) : std::string();
  const SpecLayout L0 = eligible ? spec_image_layout(ctx->hs) : SpecLayout();
  bool images = eligible;
  const size_t n = (size_t)ctx->P.scene.n_prims;
  // one block of doubles per scene: prim_f64 (16 n) | prim_hdr (8 n) | group_f64 (4 x 64) | group_gdir (3 x 64) |
  // the value image of the compiled kernel's BATCH variant (odw_build.h: spec_image_build)
  const size_t o_hdr = 16 * n, o_gf = o_hdr + 8 * n, o_gd = o_gf + ODW_MAX_GROUPS * 4, o_img = o_gd + ODW_MAX_GROUPS * 3,
               stride = o_img + (size_t)(eligible ? L0.words() : 0);
  std::vector<double> blocks(stride * (size_t)n_scenes, 0.0);
  for (int k = 0; k < n_scenes; ++k) {
    HostScene tmp;
    std::string why;
    if ((rc = scene_host_tables(&scenes[k], tmp, why))) return fail(ctx, rc, why);
    if (!same_structure(ctx->hs, tmp, why))
      return fail(ctx, ODW_ERR_UNSUPPORTED, "odw_upload_scene_batch: scene " + std::to_string(k) + " differs from scene 0 in structure (" + why + ")");
    std::vector<Box> boxes;
    compute_boxes(tmp, ctx->P.lim.dist_tol, boxes);
    if (eligible && spec_text(tmp, ctx->n_samplers) != text0) {
      if (compiled)
        return fail(ctx, ODW_ERR_UNSUPPORTED, "odw_upload_scene_batch: scene " + std::to_string(k) + " differs from scene 0 in the structure a "
                                              "compiled kernel is built from (which frame entries are 0 / +1 / -1, shared boxes)");
      images = false;                                  // (generic kernels only for this batch)
    }
    double* b = blocks.data() + stride * (size_t)k;
    if (images) spec_image_build(tmp, ctx->P.lim, L0, b + o_img, nullptr, true);
    std::memcpy(b, tmp.prim_f64.data(), 16 * n * sizeof(double));
    std::memcpy(b + o_hdr, tmp.prim_hdr.data(), 8 * n * sizeof(double));
    // (the isolated-solid shortcut depends on the boxes' values; it never changes a result: left out of batches)
    for (size_t p = 0; p < n; ++p) {
      int32_t w[4];
      std::memcpy(w, b + o_hdr + 8 * p + 6, sizeof w);
      w[2] &= ~ODW_FLAG_ISOLATED;
      std::memcpy(b + o_hdr + 8 * p + 6, w, sizeof w);
    }
    std::memcpy(b + o_gf, tmp.group_f64.data(), ODW_MAX_GROUPS * 4 * sizeof(double));
    std::memcpy(b + o_gd, tmp.group_gdir.data(), ODW_MAX_GROUPS * 3 * sizeof(double));
  }
  if ((rc = upload(ctx, ctx->batch_values, blocks.data(), blocks.size() * sizeof(double)))) return rc;
  // the shared integer tables without the isolated-solid flag
  std::vector<int32_t> pi = ctx->hs.prim_i32;
  for (size_t p = 0; p < n; ++p) pi[4 * p + 2] &= ~ODW_FLAG_ISOLATED;
  if (n && (rc = upload(ctx, ctx->prim_i32, pi.data(), pi.size() * sizeof(int32_t)))) return rc;
  if ((rc = upload_done(ctx))) return rc;
  ctx->hs.prim_i32 = pi;
  ctx->batch_n = n_scenes;
  ctx->batch_prims = n;
  ctx->batch_stride = stride;
  ctx->batch_img_off = images ? o_img : 0;
  ctx->batch_spec_text = compiled ? text0 : std::string();
  return ODW_OK;
}

namespace {
// slots of a scene's segment: the rows asked for + the slack of block reservations
uint64_t batch_slots(odw_ctx* ctx, uint64_t rows_per_scene) {
  uint64_t slots = rows_per_scene;
  if (rows_per_scene >= kHitBlockMinRows)
    slots += hit_block_room(rows_per_scene, std::min<uint64_t>((uint64_t)ctx->n_cu * 8 * 4, std::max<uint64_t>(64, rows_per_scene / 256)), kHitBlock);
  return slots;
}
}  // namespace

// Room for batch launches of up to n_scenes scenes x rays_per_scene rays x rows_per_scene rows and for their post-hoc
// chain, allocated NOW: a buffer that has to grow in the middle of a sweep is released and allocated again, which waits for
// every stream of the device (and a hit list of 13 GB takes half a second to allocate).
int odw_batch_reserve(odw_ctx* ctx, int32_t n_scenes, uint64_t rays_per_scene, uint64_t rows_per_scene) {
  if (!ctx || n_scenes < 1 || rays_per_scene == 0) return fail(ctx, ODW_ERR_INVALID, "odw_batch_reserve: bad argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const uint64_t S = (uint64_t)n_scenes, slots = batch_slots(ctx, rows_per_scene);
  if (slots > 0x7FFFFFFFull) return fail(ctx, ODW_ERR_CAPACITY, "odw_batch_reserve: more than 2^31 rows per scene");
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  int rc = ODW_OK;
  if (rows_per_scene) {
    rc = ensure(ctx, ctx->batch_hits, S * slots * sizeof(odw_hit));
    if (!rc) rc = ensure(ctx, ctx->batch_hit_count, S * 4 * sizeof(uint64_t));
  }
  if (!rc) rc = phb_reserve(ctx, (int)S, rays_per_scene, slots);
  if (!rc && rows_per_scene && rays_per_scene <= (1ull << 28))
    rc = ensure(ctx, ctx->phb_pts, S * slots * 3 * sizeof(double));
  // (the rays generated once per launch, DeviceBatch.gen_dirs: with origins, whatever the source will be)
  if (!rc && S >= 3) rc = ensure(ctx, ctx->batch_rays_buf, (size_t)((rays_per_scene + 31) / 32 * 32 * 6 + 4) * sizeof(double));
  return rc;
}

int odw_trace_batch(odw_ctx* ctx, uint64_t first_ray, uint64_t rays_per_scene, uint64_t seed, uint32_t flags,
                    uint64_t rows_per_scene) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_trace_batch: null ctx");
  if (ctx->batch_n < 1)
    return fail(ctx, ODW_ERR_NO_SCENE, "odw_trace_batch before odw_upload_scene_batch (odw_upload_scene and a new dist_tol discard an uploaded batch)");
  // the batch's tables stand beside the single-scene tables build_bvh() writes: a rebuild now would hand the BATCH kernel
  // a one-scene box table (odw_upload_scene_batch leaves everything built)
  if (ctx->bvh_dirty || (size_t)ctx->P.scene.n_prims != ctx->batch_prims)
    return fail(ctx, ODW_ERR_NO_SCENE, "odw_trace_batch: the scene changed after odw_upload_scene_batch");
  if (ctx->emitter_active) return fail(ctx, ODW_ERR_UNSUPPORTED, "odw_trace_batch: point sources only");
  if (rays_per_scene == 0) return ODW_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  batch_unselect(ctx);
  ctx->batch_rows_ok = false;            // (until this launch has been issued: a failed one leaves nothing to select)
  const uint64_t S = (uint64_t)ctx->batch_n;
  if (flags & ODW_TRACE_RECORD_HITS) {
    if (rows_per_scene == 0) return fail(ctx, ODW_ERR_CAPACITY, "odw_trace_batch: ODW_TRACE_RECORD_HITS with rows_per_scene = 0");
    const uint64_t slots = batch_slots(ctx, rows_per_scene);
    if (slots > 0x7FFFFFFFull) return fail(ctx, ODW_ERR_CAPACITY, "odw_trace_batch: more than 2^31 rows per scene");
    // (a list that has to grow is released first, which waits for the device; one that is large enough is written by
    //  this stream's next launch, behind whatever this stream still does with it)
    int rc = ensure(ctx, ctx->batch_hits, S * slots * sizeof(odw_hit));
    if (!rc) rc = ensure(ctx, ctx->batch_hit_count, S * 4 * sizeof(uint64_t));
    if (rc) return rc;
    ctx->batch_seg_slots = slots;
    ctx->batch_seg_capacity = rows_per_scene;
    HIPCHK(ctx, hipMemsetAsync(ctx->batch_hit_count.p, 0, S * 4 * sizeof(uint64_t), ctx->stream));
    // every recorded row notes its slot at its ray's place (DeviceOutputs.row_of): the table starts out as "no row"
    ctx->batch_marked = false;
    ctx->batch_pts = false;
    if (rays_per_scene <= (1ull << 28)) {
      const uint64_t rays_pad = (rays_per_scene + 31) / 32 * 32;
      rc = ensure(ctx, ctx->phb_row_of, S * rays_pad * sizeof(uint32_t));
      if (rc) return rc;
      HIPCHK(ctx, hipMemsetAsync(ctx->phb_row_of.p, 0xff, S * rays_pad * sizeof(uint32_t), ctx->stream));
      ctx->batch_marked = true;
      // (the points alone, by slot: 24 bytes more per row; without them the projection reads the rows)
      ctx->batch_pts = ensure(ctx, ctx->phb_pts, S * slots * 3 * sizeof(double)) == ODW_OK;
    }
  }
  // the value tables of scene 0 stand where the kernels' pointers point; scene s lies s strides further
  const size_t n = (size_t)ctx->P.scene.n_prims;
  const double* base = (const double*)ctx->batch_values.p;
  DeviceScene saved = ctx->P.scene;
  ctx->P.scene.prim_f64 = base;
  ctx->P.scene.prim_hdr = base + 16 * n;
  ctx->P.scene.group_f64 = base + 24 * n;
  ctx->P.scene.group_gdir = base + 24 * n + ODW_MAX_GROUPS * 4;
  ctx->batch_launch = true;
  ctx->phb_valid = ctx->phb_projected = false;
  ctx->batch_traced = ctx->batch_n;
  ctx->batch_rays = rays_per_scene;
  ctx->batch_first = first_ray;
  const int rc = launch_trace(ctx, first_ray, rays_per_scene, seed, flags, nullptr, nullptr, nullptr);
  ctx->batch_launch = false;
  ctx->batch_rows_ok = rc == ODW_OK && (flags & ODW_TRACE_RECORD_HITS) != 0;
  if (rc) ctx->batch_traced = 0;
  const bool dirty = ctx->bvh_dirty;     // (launch_trace may have rebuilt boxes: keep what it set, restore the pointers only)
  (void)dirty;
  ctx->P.scene.prim_f64 = saved.prim_f64;
  ctx->P.scene.prim_hdr = saved.prim_hdr;
  ctx->P.scene.group_f64 = saved.group_f64;
  ctx->P.scene.group_gdir = saved.group_gdir;
  return rc;
}

int odw_batch_select(odw_ctx* ctx, int32_t scene) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_batch_select: null ctx");
  if (scene < 0 || ctx->archive_selected) batch_unselect(ctx);
  if (scene < 0) return ODW_OK;
  if (!ctx->batch_rows_ok || scene >= ctx->batch_traced || !ctx->batch_hits.p || !ctx->batch_seg_slots)
    return fail(ctx, ODW_ERR_INVALID, "odw_batch_select: no such segment (odw_trace_batch with ODW_TRACE_RECORD_HITS first)");
  if (ctx->batch_selected < 0) {
    ctx->own_hits = ctx->hits;
    ctx->own_hit_count = ctx->hit_count;
    ctx->own_capacity = ctx->hit_capacity;
    ctx->own_slots = ctx->hit_slots;
    ctx->own_ray_begin = ctx->hit_ray_begin;
    ctx->own_ray_end = ctx->hit_ray_end;
  }
  ctx->hits.p = (odw_hit*)ctx->batch_hits.p + (size_t)scene * ctx->batch_seg_slots;
  ctx->hits.bytes = ctx->batch_seg_slots * sizeof(odw_hit);
  ctx->hit_count.p = (uint64_t*)ctx->batch_hit_count.p + 4 * (size_t)scene;
  ctx->hit_count.bytes = 2 * sizeof(uint64_t);
  ctx->hit_capacity = ctx->batch_seg_capacity;
  ctx->hit_slots = ctx->batch_seg_slots;
  ctx->hit_ray_begin = ctx->batch_first;
  ctx->hit_ray_end = std::min<uint64_t>(ctx->batch_first + ctx->batch_rays, 1ull << 48);
  ctx->batch_selected = scene;
  ctx->ph_valid = false;
  return ODW_OK;
}

int odw_batch_rows(odw_ctx* ctx, uint64_t* rows, uint64_t* wanted, int32_t n) {
  if (!ctx || !rows || n < 0) return fail(ctx, ODW_ERR_INVALID, "odw_batch_rows: bad argument");
  if (n > 0 && !ctx->batch_rows_ok) return fail(ctx, ODW_ERR_INVALID, "odw_batch_rows: no batch was traced with hit rows");
  if (n > ctx->batch_traced) return fail(ctx, ODW_ERR_INVALID, "odw_batch_rows: more scenes than the batch traced");
  if (n == 0) return ODW_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::vector<uint64_t> v(4 * (size_t)n, 0);
  HIPCHK(ctx, hipMemcpyAsync(v.data(), ctx->batch_hit_count.p, v.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (int k = 0; k < n; ++k) {
    const uint64_t used = std::min<uint64_t>(v[4 * k], ctx->batch_seg_slots);
    rows[k] = used > v[4 * k + 1] ? used - v[4 * k + 1] : 0;
    if (wanted) wanted[k] = v[4 * k];          // slots asked for (above the segment's room: rows were dropped)
  }
  return ODW_OK;
}

static int hit_slots_used(odw_ctx* ctx, uint64_t* used, uint64_t* rows);

// ---- a run's rows kept in HBM (v9) ---------------------------------------------------------------------------------
int odw_archive_append(odw_ctx* ctx, odw_ctx* src, uint64_t* total_rows) {
  if (!ctx || !src) return fail(ctx, ODW_ERR_INVALID, "odw_archive_append: null context");
  if (ctx->device != src->device) return fail(ctx, ODW_ERR_INVALID, "odw_archive_append: the contexts live on different devices");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  batch_unselect(ctx);
  if (src != ctx) batch_unselect(src);
  uint64_t used = 0, rows = 0;
  int rc = hit_slots_used(src, &used, &rows);          // (waits for src's stream: its launch has finished)
  if (rc) { ctx->err = src->err; return rc; }
  if (used) {
    const uint64_t need = ctx->archive_slots + used;
    if (need > 0x7FFFFFFFull) return fail(ctx, ODW_ERR_CAPACITY, "odw_archive_append: more than 2^31 rows");
    if (ctx->archive.bytes < need * sizeof(odw_hit)) {
      // grow by doubling: the rows kept so far move once per doubling
      DevBuf bigger;
      const uint64_t cap = std::max<uint64_t>(need, std::max<uint64_t>(1ull << 22, 2 * ctx->archive.bytes / sizeof(odw_hit)));
      HIPCHK(ctx, hipMalloc(&bigger.p, cap * sizeof(odw_hit)));
      bigger.bytes = cap * sizeof(odw_hit);
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
      if (ctx->archive_slots)
        HIPCHK(ctx, hipMemcpyAsync(bigger.p, ctx->archive.p, ctx->archive_slots * sizeof(odw_hit), hipMemcpyDeviceToDevice, ctx->stream));
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
      release(ctx->archive);
      ctx->archive = bigger;
    }
    // the spectrum the rows were drawn under travels with them to a context that has no source of its own (a run's
    // archive): odw_hits_bin_bands draws the rows' wavelengths again from (seed, ray number) under it
    if (src != ctx && src->spec_n > 0 && !ctx->have_source) {
      if ((rc = ensure(ctx, ctx->spec_tab, src->spec_tab.bytes))) return rc;
      HIPCHK(ctx, hipMemcpyAsync(ctx->spec_tab.p, src->spec_tab.p, src->spec_tab.bytes, hipMemcpyDeviceToDevice, ctx->stream));
      ctx->spec_n = src->spec_n;
      ctx->spec_mode = src->spec_mode;
      ctx->spec_lo = src->spec_lo;
      ctx->spec_hi = src->spec_hi;
    }
    // (slots tagged unused travel along: every pass over a hit list skips them)
    HIPCHK(ctx, hipMemcpyAsync((odw_hit*)ctx->archive.p + ctx->archive_slots, src->hits.p, used * sizeof(odw_hit),
                               hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));    // (src's list may be recycled as soon as this returns)
    ctx->archive_ray_begin = ctx->archive_slots ? std::min(ctx->archive_ray_begin, src->hit_ray_begin) : src->hit_ray_begin;
    ctx->archive_ray_end = ctx->archive_slots ? std::max(ctx->archive_ray_end, src->hit_ray_end) : src->hit_ray_end;
    ctx->archive_slots = need;
    ctx->archive_unused += used - rows;
  }
  if (total_rows) *total_rows = ctx->archive_slots - ctx->archive_unused;
  return ODW_OK;
}

int odw_archive_select(odw_ctx* ctx, int32_t on) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_archive_select: null ctx");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  batch_unselect(ctx);
  if (!on) return ODW_OK;
  if (!ctx->archive_slots) return fail(ctx, ODW_ERR_INVALID, "odw_archive_select: nothing was archived");
  int rc = ensure(ctx, ctx->archive_count, 2 * sizeof(uint64_t));
  if (rc) return rc;
  const uint64_t count[2] = {ctx->archive_slots, ctx->archive_unused};
  HIPCHK(ctx, hipMemcpyAsync(ctx->archive_count.p, count, sizeof count, hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  ctx->own_hits = ctx->hits;
  ctx->own_hit_count = ctx->hit_count;
  ctx->own_capacity = ctx->hit_capacity;
  ctx->own_slots = ctx->hit_slots;
  ctx->own_ray_begin = ctx->hit_ray_begin;
  ctx->own_ray_end = ctx->hit_ray_end;
  ctx->hits.p = ctx->archive.p;
  ctx->hits.bytes = ctx->archive_slots * sizeof(odw_hit);
  ctx->hit_count.p = ctx->archive_count.p;
  ctx->hit_count.bytes = 2 * sizeof(uint64_t);
  ctx->hit_capacity = ctx->hit_slots = ctx->archive_slots;
  ctx->hit_ray_begin = ctx->archive_ray_begin;
  ctx->hit_ray_end = ctx->archive_ray_end;
  ctx->archive_selected = true;
  ctx->ph_valid = false;
  return ODW_OK;
}

int odw_archive_reset(odw_ctx* ctx) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_archive_reset: null ctx");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  batch_unselect(ctx);
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  release(ctx->archive);
  ctx->archive_slots = ctx->archive_unused = 0;
  return ODW_OK;
}

static int trace_rays(odw_ctx* ctx, uint64_t first_ray, uint64_t n_rays, const double* origins, const double* directions,
                      const double* powers, const double* wavelengths, double wl_lo, double wl_hi, uint32_t flags);

int odw_trace_rays(odw_ctx* ctx, uint64_t first_ray, uint64_t n_rays, const double* origins,
                   const double* directions, const double* powers, uint32_t flags) {
  if (!ctx || !origins || !directions) return fail(ctx, ODW_ERR_INVALID, "odw_trace_rays: null argument");
  return trace_rays(ctx, first_ray, n_rays, origins, directions, powers, nullptr, 0.0, 0.0, flags);
}

int odw_trace_rays_spectral(odw_ctx* ctx, uint64_t first_ray, uint64_t n_rays, const double* origins,
                            const double* directions, const double* powers, const double* wavelengths, uint32_t flags) {
  if (!ctx || !origins || !directions || !wavelengths) return fail(ctx, ODW_ERR_INVALID, "odw_trace_rays_spectral: null argument");
  double lo = INFINITY, hi = -INFINITY;
  for (uint64_t i = 0; i < n_rays; ++i) {
    if (!(wavelengths[i] > 0) || !std::isfinite(wavelengths[i])) return fail(ctx, ODW_ERR_INVALID, "odw_trace_rays_spectral: wavelengths must be finite and > 0");
    lo = std::min(lo, wavelengths[i]);
    hi = std::max(hi, wavelengths[i]);
  }
  return trace_rays(ctx, first_ray, n_rays, origins, directions, powers, wavelengths, lo, hi, flags);
}

static int trace_rays(odw_ctx* ctx, uint64_t first_ray, uint64_t n_rays, const double* origins, const double* directions,
                      const double* powers, const double* wavelengths, double wl_lo, double wl_hi, uint32_t flags) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  batch_unselect(ctx);
  if (n_rays == 0) return ODW_OK;
  // the previous launch may still read the staging buffers
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  int rc;
  // the caller's n x 3 arrays are staged as they are, then turned component-major on the device (the kernels'
  // lanes read consecutive rays: unit-stride loads instead of 24-byte strides)
  if ((rc = ensure(ctx, ctx->ray_aos, n_rays * 6 * sizeof(double)))) return rc;
  if ((rc = ensure(ctx, ctx->ray_o, n_rays * 3 * sizeof(double)))) return rc;
  if ((rc = ensure(ctx, ctx->ray_d, n_rays * 3 * sizeof(double)))) return rc;
  double* aos = (double*)ctx->ray_aos.p;
  HIPCHK(ctx, hipMemcpyAsync(aos, origins, n_rays * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(aos + 3 * n_rays, directions, n_rays * 3 * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  {
    const unsigned tgrid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((3 * n_rays + 255) / 256, (uint64_t)ctx->n_cu * 16));
    hipLaunchKernelGGL(odw_rays_to_components_kernel, dim3(tgrid), dim3(256), 0, ctx->stream, (const double*)aos,
                       (const double*)(aos + 3 * n_rays), n_rays, (double*)ctx->ray_o.p, (double*)ctx->ray_d.p);
    HIPCHK(ctx, hipGetLastError());
  }
  if (powers) {
    if ((rc = upload(ctx, ctx->ray_p, powers, n_rays * sizeof(double)))) return rc;
  }
  if (wavelengths) {
    if ((rc = upload(ctx, ctx->ray_wl, wavelengths, n_rays * sizeof(double)))) return rc;
  }
  rc = launch_trace(ctx, first_ray, n_rays, ctx->surface_seed, flags, (const double*)ctx->ray_o.p,
                    (const double*)ctx->ray_d.p, powers ? (const double*)ctx->ray_p.p : nullptr,
                    wavelengths ? (const double*)ctx->ray_wl.p : nullptr, wl_lo, wl_hi);
  if (rc) return rc;
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // caller's arrays may go away
  return ODW_OK;
}

int odw_sync(odw_ctx* ctx) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_sync: null ctx");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return ODW_OK;
}

int odw_reset_results(odw_ctx* ctx) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_reset_results: null ctx");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  batch_unselect(ctx);
  ctx->ph_valid = false;
  ctx->hit_ray_end = 0;
  HIPCHK(ctx, hipMemsetAsync(ctx->counters.p, 0, ODW_CNT_COUNT * sizeof(uint64_t), ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(ctx->hit_count.p, 0, 2 * sizeof(uint64_t), ctx->stream));
  HIPCHK(ctx, hipMemsetAsync(ctx->seg_count.p, 0, sizeof(uint64_t), ctx->stream));
  if (ctx->n_bins) HIPCHK(ctx, hipMemsetAsync(ctx->hist.p, 0, ctx->plane_words() * sizeof(uint64_t), ctx->stream));
  return ODW_OK;
}

int odw_reset_segments(odw_ctx* ctx) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_reset_segments: null ctx");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemsetAsync(ctx->seg_count.p, 0, sizeof(uint64_t), ctx->stream));
  return ODW_OK;
}

int odw_reset_hits(odw_ctx* ctx) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_reset_hits: null ctx");
  batch_unselect(ctx);
  ctx->ph_valid = false;
  ctx->hit_ray_end = 0;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemsetAsync(ctx->hit_count.p, 0, 2 * sizeof(uint64_t), ctx->stream));
  return ODW_OK;
}

int odw_fetch_counters(odw_ctx* ctx, uint64_t* out, int32_t n) {
  if (!ctx || !out || n < 0) return fail(ctx, ODW_ERR_INVALID, "odw_fetch_counters: bad argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  uint64_t tmp[ODW_CNT_COUNT];
  HIPCHK(ctx, hipMemcpyAsync(tmp, ctx->counters.p, sizeof tmp, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (int i = 0; i < n && i < ODW_CNT_COUNT; ++i) out[i] = tmp[i];
  return ODW_OK;
}

// slots handed out (clamped to the buffer) and how many of them hold rows
static int hit_slots_used(odw_ctx* ctx, uint64_t* used, uint64_t* rows) {
  HIPCHK(ctx, hipSetDevice(ctx->device));
  uint64_t v[2] = {0, 0};
  HIPCHK(ctx, hipMemcpyAsync(v, ctx->hit_count.p, sizeof v, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  *used = std::min<uint64_t>(v[0], ctx->hit_slots);
  *rows = *used > v[1] ? *used - v[1] : 0;
  return ODW_OK;
}

int odw_hit_count(odw_ctx* ctx, uint64_t* n) {
  if (!ctx || !n) return fail(ctx, ODW_ERR_INVALID, "odw_hit_count: bad argument");
  uint64_t used = 0;
  return hit_slots_used(ctx, &used, n);
}

int odw_fetch_hits(odw_ctx* ctx, odw_hit* out, uint64_t capacity, uint64_t* n) {
  if (!ctx || !n) return fail(ctx, ODW_ERR_INVALID, "odw_fetch_hits: bad argument");
  uint64_t used = 0, have = 0;
  int rc = hit_slots_used(ctx, &used, &have);
  if (rc) return rc;
  *n = have;
  if (!out || capacity == 0) return ODW_OK;
  if (have > capacity) return fail(ctx, ODW_ERR_CAPACITY, "odw_fetch_hits: output buffer too small");
  ctx->ph_valid = false;           // the sort buffers are shared with odw_hits_select
  if (have) {
    // append order is scheduling dependent; a ray's own rows are appended in
    // bounce order, so a STABLE sort by ray index gives (ray, bounce) order.
    // Done on the device: LSD radix sort of (ray index -> slot number) pairs
    // (hipCUB, stable; unused slots of block reservations sort to the end),
    // then a gather of the 64-byte rows, then one D2H copy.
    if (used > 0x7FFFFFFFull) return fail(ctx, ODW_ERR_CAPACITY, "odw_fetch_hits: more than 2^31 rows per fetch");
    for (int k = 0; k < 2; ++k) {
      if ((rc = ensure(ctx, ctx->sort_keys[k], used * sizeof(uint64_t)))) return rc;
      if ((rc = ensure(ctx, ctx->sort_vals[k], used * sizeof(uint32_t)))) return rc;
    }
    if ((rc = ensure(ctx, ctx->sorted_rows, have * sizeof(odw_hit)))) return rc;
    uint64_t* k_in = (uint64_t*)ctx->sort_keys[0].p;
    uint64_t* k_out = (uint64_t*)ctx->sort_keys[1].p;
    uint32_t* v_in = (uint32_t*)ctx->sort_vals[0].p;
    uint32_t* v_out = (uint32_t*)ctx->sort_vals[1].p;
    const unsigned blocks = (unsigned)((used + 255) / 256);
    // (only the bits ray indices of this list can have, + 1 for the sentinel: see odw_hits_select)
    int bits = 48;
    if (ctx->hit_ray_end && ctx->hit_ray_end < (1ull << 48)) { bits = 1; while ((1ull << bits) < ctx->hit_ray_end) ++bits; }
    const bool spare = ctx->hit_ray_end && ctx->hit_ray_end < (1ull << bits);
    const uint64_t sentinel = spare ? (1ull << bits) - 1 : 1ull << bits;
    if (spare) --bits;
    hipLaunchKernelGGL(hit_keys_kernel, dim3(blocks), dim3(256), 0, ctx->stream, (const odw_hit*)ctx->hits.p,
                       used, sentinel, k_in, v_in);
    HIPCHK(ctx, hipGetLastError());
    size_t tmp_bytes = 0;
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, k_in, k_out, v_in, v_out, (int)used, 0, bits + 1,
                                                   ctx->stream));
    if ((rc = ensure(ctx, ctx->sort_tmp, tmp_bytes))) return rc;
    HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairs(ctx->sort_tmp.p, tmp_bytes, k_in, k_out, v_in, v_out, (int)used,
                                                   0, bits + 1, ctx->stream));
    const unsigned gblocks = (unsigned)((have * 4 + 255) / 256);
    hipLaunchKernelGGL(hit_gather_kernel, dim3(gblocks), dim3(256), 0, ctx->stream, (const odw_hit*)ctx->hits.p,
                       v_out, have, (odw_hit*)ctx->sorted_rows.p);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out, ctx->sorted_rows.p, have * sizeof(odw_hit), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  }
  return ODW_OK;
}

int odw_swap_hit_lists(odw_ctx* ctx) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_swap_hit_lists: null ctx");
  batch_unselect(ctx);
  if (ctx->hit_capacity == 0) return fail(ctx, ODW_ERR_CAPACITY, "odw_swap_hit_lists without odw_reserve_hits");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  ctx->ph_valid = false;
  if (!ctx->copy_stream) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
  if (!ctx->alt_ready) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->alt_ready, hipEventDisableTiming));
  if (ctx->alt_slots < ctx->hit_slots) {     // the other list gets the same room
    HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
    release(ctx->alt_hits);
    int rc = ensure(ctx, ctx->alt_hits, ctx->hit_slots * sizeof(odw_hit));
    if (!rc) rc = ensure(ctx, ctx->alt_hit_count, 2 * sizeof(uint64_t));
    if (rc) return rc;
    ctx->alt_capacity = ctx->hit_capacity;
    ctx->alt_slots = ctx->hit_slots;
    HIPCHK(ctx, hipMemsetAsync(ctx->alt_hit_count.p, 0, 2 * sizeof(uint64_t), ctx->stream));
  }
  // everything launched so far wrote into the list that is put aside now
  HIPCHK(ctx, hipEventRecord(ctx->alt_ready, ctx->stream));
  std::swap(ctx->hits, ctx->alt_hits);
  std::swap(ctx->hit_count, ctx->alt_hit_count);
  std::swap(ctx->hit_capacity, ctx->alt_capacity);
  std::swap(ctx->hit_slots, ctx->alt_slots);
  std::swap(ctx->hit_ray_end, ctx->alt_hit_ray_end);
  std::swap(ctx->hit_ray_begin, ctx->alt_hit_ray_begin);
  ctx->swapping = true;
  return ODW_OK;
}

int odw_host_alloc(odw_ctx* ctx, uint64_t bytes, void** out) {
  if (!ctx || !out || bytes == 0) return fail(ctx, ODW_ERR_INVALID, "odw_host_alloc: bad argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  *out = nullptr;
  HIPCHK(ctx, hipHostMalloc(out, bytes, hipHostMallocDefault));
  return ODW_OK;
}

int odw_mem_info(odw_ctx* ctx, uint64_t* free_bytes, uint64_t* total_bytes) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_mem_info: null ctx");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  size_t f = 0, t = 0;
  HIPCHK(ctx, hipMemGetInfo(&f, &t));
  if (free_bytes) *free_bytes = (uint64_t)f;
  if (total_bytes) *total_bytes = (uint64_t)t;
  return ODW_OK;
}

int odw_host_free(odw_ctx* ctx, void* p) {
  // (ctx may be null: page-locked arrays handed to the caller can outlive the context that allocated them)
  if (p) HIPCHK(ctx, hipHostFree(p));
  return ODW_OK;
}

int odw_release_swapped_hits(odw_ctx* ctx) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_release_swapped_hits: null ctx");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (ctx->copy_stream) HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  release(ctx->alt_hits);
  ctx->alt_capacity = ctx->alt_slots = 0;
  ctx->swapping = false;           // launches reserve hit-list blocks again
  return ODW_OK;
}

int odw_fetch_swapped_hits(odw_ctx* ctx, odw_hit* out, uint64_t capacity, uint64_t* n) {
  if (!ctx || !n) return fail(ctx, ODW_ERR_INVALID, "odw_fetch_swapped_hits: bad argument");
  if (!ctx->swapping || !ctx->copy_stream) return fail(ctx, ODW_ERR_INVALID, "odw_fetch_swapped_hits: odw_swap_hit_lists first");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // the copy stream waits for the launches that filled the list, not for what runs on the trace
  // stream since: the next launch proceeds while these rows cross PCIe
  HIPCHK(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->alt_ready, 0));
  uint64_t v[2] = {0, 0};
  HIPCHK(ctx, hipMemcpyAsync(v, ctx->alt_hit_count.p, sizeof v, hipMemcpyDeviceToHost, ctx->copy_stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
  const uint64_t have = std::min<uint64_t>(v[0], ctx->alt_slots);    // dense: no unused slots in swapped lists
  *n = have;
  if (!out || capacity == 0 || have == 0) return ODW_OK;
  if (have > capacity) return fail(ctx, ODW_ERR_CAPACITY, "odw_fetch_swapped_hits: output buffer too small");
  HIPCHK(ctx, hipMemcpyAsync(out, ctx->alt_hits.p, have * sizeof(odw_hit), hipMemcpyDeviceToHost, ctx->copy_stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));
  return ODW_OK;
}

int odw_segment_count(odw_ctx* ctx, uint64_t* n, uint64_t* dropped) {
  if (!ctx || !n) return fail(ctx, ODW_ERR_INVALID, "odw_segment_count: bad argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  uint64_t wanted = 0;
  HIPCHK(ctx, hipMemcpyAsync(&wanted, ctx->seg_count.p, sizeof wanted, hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  *n = std::min<uint64_t>(wanted, ctx->seg_capacity);
  if (dropped) *dropped = wanted - *n;
  return ODW_OK;
}

int odw_fetch_segments(odw_ctx* ctx, odw_segment* out, uint64_t capacity, uint64_t* n) {
  if (!ctx || !n) return fail(ctx, ODW_ERR_INVALID, "odw_fetch_segments: bad argument");
  ctx->ph_valid = false;           // the sort buffers are shared with odw_hits_select
  uint64_t have = 0;
  int rc = odw_segment_count(ctx, &have, nullptr);
  if (rc) return rc;
  *n = have;
  if (!out || capacity == 0 || have == 0) return ODW_OK;
  if (have > capacity) return fail(ctx, ODW_ERR_CAPACITY, "odw_fetch_segments: output buffer too small");
  // same device-side ordering as the hit list, with the explicit key (ray, ordinal)
  static_assert(sizeof(odw_segment) == sizeof(odw_hit), "rows share the gather kernel");
  for (int k = 0; k < 2; ++k) {
    if ((rc = ensure(ctx, ctx->sort_keys[k], have * sizeof(uint64_t)))) return rc;
    if ((rc = ensure(ctx, ctx->sort_vals[k], have * sizeof(uint32_t)))) return rc;
  }
  if ((rc = ensure(ctx, ctx->sorted_rows, have * sizeof(odw_segment)))) return rc;
  uint64_t* k_in = (uint64_t*)ctx->sort_keys[0].p;
  uint64_t* k_out = (uint64_t*)ctx->sort_keys[1].p;
  uint32_t* v_in = (uint32_t*)ctx->sort_vals[0].p;
  uint32_t* v_out = (uint32_t*)ctx->sort_vals[1].p;
  hipLaunchKernelGGL(seg_keys_kernel, dim3((unsigned)((have + 255) / 256)), dim3(256), 0, ctx->stream,
                     (const odw_segment*)ctx->segs.p, have, k_in, v_in);
  HIPCHK(ctx, hipGetLastError());
  size_t tmp_bytes = 0;
  HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, k_in, k_out, v_in, v_out, (int)have, 0, 52,
                                                 ctx->stream));
  if ((rc = ensure(ctx, ctx->sort_tmp, tmp_bytes))) return rc;
  HIPCHK(ctx, hipcub::DeviceRadixSort::SortPairs(ctx->sort_tmp.p, tmp_bytes, k_in, k_out, v_in, v_out, (int)have, 0,
                                                 52, ctx->stream));
  hipLaunchKernelGGL(hit_gather_kernel, dim3((unsigned)((have * 4 + 255) / 256)), dim3(256), 0, ctx->stream,
                     (const odw_hit*)ctx->segs.p, v_out, have, (odw_hit*)ctx->sorted_rows.p);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(out, ctx->sorted_rows.p, have * sizeof(odw_segment), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return ODW_OK;
}

int odw_fetch_histogram(odw_ctx* ctx, uint64_t* out, uint64_t n_bins) {
  if (!ctx || !out) return fail(ctx, ODW_ERR_INVALID, "odw_fetch_histogram: bad argument");
  if (n_bins != ctx->n_bins || n_bins == 0) return fail(ctx, ODW_ERR_INVALID, "odw_fetch_histogram: bin count mismatch");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemcpyAsync(out, ctx->hist.p, n_bins * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return ODW_OK;
}

int odw_enable_power_histogram(odw_ctx* ctx, int on) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_enable_power_histogram: null ctx");
  if (!on) {
    // (with bands the band count planes move up into the power plane's place: laid out again, zeroed)
    if (ctx->power_on && ctx->band_n) {
      HIPCHK(ctx, hipSetDevice(ctx->device));
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
      HIPCHK(ctx, hipMemsetAsync((uint64_t*)ctx->hist.p + ctx->n_bins, 0, ctx->n_bins * ctx->band_k() * sizeof(uint64_t), ctx->stream));
    }
    ctx->power_on = false;
    return ODW_OK;
  }
  if (!ctx->P.det_enabled || ctx->n_bins == 0) return fail(ctx, ODW_ERR_INVALID, "odw_enable_power_histogram: odw_set_detector first");
  if (ctx->n_bins >= (1ull << 31)) return fail(ctx, ODW_ERR_INVALID, "odw_enable_power_histogram: a power plane takes fewer than 2^31 bins");
  if (2 * ctx->n_bins * (1 + ctx->band_k()) >= (1ull << 31))
    return fail(ctx, ODW_ERR_INVALID, "odw_enable_power_histogram: with the detector's bands the results block would take 2^31 words or more");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // a running launch may still write the old block
  int rc = ensure_results(ctx, 2 * ctx->n_bins * (1 + ctx->band_k()), ctx->n_bins);
  if (rc) return rc;
  // (the power plane, and with bands every band plane: the block is laid out again)
  HIPCHK(ctx, hipMemsetAsync((uint64_t*)ctx->hist.p + ctx->n_bins, 0, ctx->n_bins * (1 + 2 * ctx->band_k()) * sizeof(uint64_t), ctx->stream));
  ctx->power_on = true;
  return ODW_OK;
}

int odw_fetch_power_histogram(odw_ctx* ctx, uint64_t* out, uint64_t n_bins) {
  if (!ctx || !out) return fail(ctx, ODW_ERR_INVALID, "odw_fetch_power_histogram: bad argument");
  if (!ctx->power_on) return fail(ctx, ODW_ERR_INVALID, "odw_fetch_power_histogram: no power plane (odw_enable_power_histogram)");
  if (n_bins != ctx->n_bins || n_bins == 0) return fail(ctx, ODW_ERR_INVALID, "odw_fetch_power_histogram: bin count mismatch");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::vector<uint64_t> counts(n_bins);
  HIPCHK(ctx, hipMemcpyAsync(counts.data(), ctx->hist.p, n_bins * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(out, (uint64_t*)ctx->hist.p + n_bins, n_bins * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  // a bin of >= 2^32 hits may hold more than 2^64 quanta: its sum may have wrapped, nothing is handed out
  for (uint64_t k = 0; k < n_bins; ++k)
    if (counts[k] >> 32) {
      std::memset(out, 0, n_bins * sizeof(uint64_t));
      return fail(ctx, ODW_ERR_CAPACITY, "odw_fetch_power_histogram: bin " + std::to_string(k) + " holds " + std::to_string(counts[k]) +
                  " hits (>= 2^32): its power sum may have wrapped");
    }
  return ODW_OK;
}

int odw_set_detector_bands(odw_ctx* ctx, int32_t n_edges, const double* edges_nm) {
  // (without a context: the check of the edges alone, as odw_dispersion_check checks a dispersion)
  if (n_edges != 0) {
    std::string err;
    const int rc = bands_validate("odw_set_detector_bands", n_edges, edges_nm, err);
    if (rc) return fail(ctx, rc, err);
  }
  if (!ctx) return n_edges ? ODW_OK : fail(ctx, ODW_ERR_INVALID, "odw_set_detector_bands: null ctx");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (n_edges == 0) {
    if (ctx->band_n) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->band_n = 0;
    return ODW_OK;
  }
  if (!ctx->P.det_enabled || ctx->n_bins == 0) return fail(ctx, ODW_ERR_INVALID, "odw_set_detector_bands: bands need a detector (odw_set_detector first)");
  const uint64_t K = (uint64_t)n_edges - 1, planes = (ctx->power_on ? 2 : 1) * (1 + K);
  if (ctx->n_bins * planes >= (1ull << 31)) {
    char buf[200];
    std::snprintf(buf, sizeof buf, "odw_set_detector_bands: %llu planes of %llu bins: the results block must stay below 2^31 words "
                  "(the kernels index it with 32-bit products)", (unsigned long long)planes, (unsigned long long)ctx->n_bins);
    return fail(ctx, ODW_ERR_INVALID, buf);
  }
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // a running launch may still write the old block / read the old edges
  const uint64_t front = ctx->n_bins * (ctx->power_on ? 2 : 1);
  int rc = ensure_results(ctx, ctx->n_bins * planes, front);
  if (rc) return rc;
  if ((rc = upload(ctx, ctx->d_band_edges, edges_nm, (size_t)n_edges * sizeof(double)))) return rc;
  std::memcpy(ctx->band_edges, edges_nm, (size_t)n_edges * sizeof(double));
  ctx->band_n = n_edges;
  HIPCHK(ctx, hipMemsetAsync((uint64_t*)ctx->hist.p + front, 0, (ctx->n_bins * planes - front) * sizeof(uint64_t), ctx->stream));
  return ODW_OK;
}

int odw_fetch_band_histogram(odw_ctx* ctx, uint64_t* out, uint64_t n_words) {
  if (!ctx || !out) return fail(ctx, ODW_ERR_INVALID, "odw_fetch_band_histogram: bad argument");
  if (!ctx->band_n || !ctx->n_bins) return fail(ctx, ODW_ERR_INVALID, "odw_fetch_band_histogram: no bands (odw_set_detector_bands)");
  if (n_words != ctx->band_k() * ctx->n_bins) return fail(ctx, ODW_ERR_INVALID, "odw_fetch_band_histogram: word count mismatch (K * nx * ny)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const uint64_t* src = (const uint64_t*)ctx->hist.p + ctx->n_bins * (ctx->power_on ? 2 : 1);
  HIPCHK(ctx, hipMemcpyAsync(out, src, n_words * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return ODW_OK;
}

int odw_fetch_band_power_histogram(odw_ctx* ctx, uint64_t* out, uint64_t n_words) {
  if (!ctx || !out) return fail(ctx, ODW_ERR_INVALID, "odw_fetch_band_power_histogram: bad argument");
  if (!ctx->band_n || !ctx->n_bins) return fail(ctx, ODW_ERR_INVALID, "odw_fetch_band_power_histogram: no bands (odw_set_detector_bands)");
  if (!ctx->power_on) return fail(ctx, ODW_ERR_INVALID, "odw_fetch_band_power_histogram: no power plane (odw_enable_power_histogram)");
  if (n_words != ctx->band_k() * ctx->n_bins) return fail(ctx, ODW_ERR_INVALID, "odw_fetch_band_power_histogram: word count mismatch (K * nx * ny)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  std::vector<uint64_t> counts(n_words);
  const uint64_t* src = (const uint64_t*)ctx->hist.p + 2 * ctx->n_bins;
  HIPCHK(ctx, hipMemcpyAsync(counts.data(), src, n_words * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(out, src + n_words, n_words * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  // (odw_fetch_power_histogram's rule, per band plane)
  for (uint64_t k = 0; k < n_words; ++k)
    if (counts[k] >> 32) {
      std::memset(out, 0, n_words * sizeof(uint64_t));
      return fail(ctx, ODW_ERR_CAPACITY, "odw_fetch_band_power_histogram: band " + std::to_string(k / ctx->n_bins) + ", bin " + std::to_string(k % ctx->n_bins) +
                  " holds " + std::to_string(counts[k]) + " hits (>= 2^32): its power sum may have wrapped");
    }
  return ODW_OK;
}

int odw_band_index(const double* edges_nm, int32_t n_edges, const double* wavelengths_nm, uint64_t n, int32_t* out_i32, int32_t on_device) {
  std::string err;
  const int vrc = bands_validate("odw_band_index", n_edges, edges_nm, err);
  if (vrc) return fail(nullptr, vrc, err);
  if (n && (!wavelengths_nm || !out_i32)) return fail(nullptr, ODW_ERR_INVALID, "odw_band_index: bad argument");
  if (!on_device) {
    for (uint64_t i = 0; i < n; ++i) out_i32[i] = band_index(edges_nm, n_edges, wavelengths_nm[i]);
    return ODW_OK;
  }
  if (n == 0) return ODW_OK;
  // (context-free: buffers of its own on the current device, the null stream)
  odw_ctx* const ctx = nullptr;
  DevBuf e, w, o;
  hipError_t he = hipMalloc(&e.p, (size_t)n_edges * sizeof(double));
  if (he == hipSuccess) he = hipMalloc(&w.p, n * sizeof(double));
  if (he == hipSuccess) he = hipMalloc(&o.p, n * sizeof(int32_t));
  if (he == hipSuccess) he = hipMemcpy(e.p, edges_nm, (size_t)n_edges * sizeof(double), hipMemcpyHostToDevice);
  if (he == hipSuccess) he = hipMemcpy(w.p, wavelengths_nm, n * sizeof(double), hipMemcpyHostToDevice);
  if (he == hipSuccess) {
    const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 4096));
    hipLaunchKernelGGL(odw_band_index_kernel, dim3(grid), dim3(256), 0, nullptr, (const double*)e.p, (int)n_edges, (const double*)w.p, n, (int32_t*)o.p);
    he = hipGetLastError();
  }
  if (he == hipSuccess) he = hipMemcpy(out_i32, o.p, n * sizeof(int32_t), hipMemcpyDeviceToHost);
  for (DevBuf* b : {&e, &w, &o}) if (b->p) (void)hipFree(b->p);
  HIPCHK(ctx, he);
  return ODW_OK;
}

int odw_device_band_histogram(odw_ctx* ctx, void** dptr, uint64_t* n_words) {
  if (!ctx || !dptr || !n_words) return fail(ctx, ODW_ERR_INVALID, "odw_device_band_histogram: bad argument");
  const bool on = ctx->band_n && ctx->n_bins;
  const uint64_t front = ctx->n_bins * (ctx->power_on ? 2 : 1);
  *dptr = on ? (void*)((uint64_t*)ctx->hist.p + front) : nullptr;
  *n_words = on ? ctx->plane_words() - front : 0;
  return ODW_OK;
}

int odw_sample(odw_ctx* ctx, uint64_t first_ray, uint64_t n_rays, uint64_t seed, double* theta_out,
               double* phi_out) {
  if (!ctx || !theta_out || !phi_out) return fail(ctx, ODW_ERR_INVALID, "odw_sample: bad argument");
  if (!ctx->have_source || ctx->emitter_active) return fail(ctx, ODW_ERR_NO_SCENE, "point source not uploaded");
  if (n_rays == 0) return ODW_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int rc;
  if ((rc = ensure(ctx, ctx->samp_t, n_rays * sizeof(double)))) return rc;
  if ((rc = ensure(ctx, ctx->samp_phi, n_rays * sizeof(double)))) return rc;
  const unsigned grid = (unsigned)std::min<uint64_t>((n_rays + 255) / 256, (uint64_t)ctx->n_cu * 8);
  hipLaunchKernelGGL(odw_sample_kernel, dim3(grid), dim3(256), 0, ctx->stream, ctx->P.source, first_ray,
                     n_rays, seed, (double*)ctx->samp_t.p, (double*)ctx->samp_phi.p);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(theta_out, ctx->samp_t.p, n_rays * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipMemcpyAsync(phi_out, ctx->samp_phi.p, n_rays * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  return ODW_OK;
}

int odw_device_results(odw_ctx* ctx, void** dptr, uint64_t* n_words, uint64_t* hist_offset_words) {
  if (!ctx || !dptr || !n_words || !hist_offset_words) return fail(ctx, ODW_ERR_INVALID, "odw_device_results: bad argument");
  *dptr = ctx->results.p;
  *n_words = kResultsHead + ctx->plane_words();
  *hist_offset_words = kResultsHead;
  return ODW_OK;
}

int odw_device_histogram(odw_ctx* ctx, void** dptr, uint64_t* n_bins) {
  if (!ctx || !dptr || !n_bins) return fail(ctx, ODW_ERR_INVALID, "odw_device_histogram: bad argument");
  *dptr = ctx->n_bins ? ctx->hist.p : nullptr;
  *n_bins = ctx->n_bins;
  return ODW_OK;
}

int odw_device_power_histogram(odw_ctx* ctx, void** dptr, uint64_t* n_bins) {
  if (!ctx || !dptr || !n_bins) return fail(ctx, ODW_ERR_INVALID, "odw_device_power_histogram: bad argument");
  const bool on = ctx->power_on && ctx->n_bins;
  *dptr = on ? (void*)((uint64_t*)ctx->hist.p + ctx->n_bins) : nullptr;
  *n_bins = on ? ctx->n_bins : 0;
  return ODW_OK;
}

int odw_device_counters(odw_ctx* ctx, void** dptr, uint64_t* n) {
  if (!ctx || !dptr || !n) return fail(ctx, ODW_ERR_INVALID, "odw_device_counters: bad argument");
  *dptr = ctx->counters.p;
  *n = ODW_CNT_COUNT;
  return ODW_OK;
}

int odw_stream(odw_ctx* ctx, void** hip_stream) {
  if (!ctx || !hip_stream) return fail(ctx, ODW_ERR_INVALID, "odw_stream: bad argument");
  *hip_stream = (void*)ctx->stream;
  return ODW_OK;
}

int odw_timing_enable(odw_ctx* ctx, int on) {
  if (!ctx) return fail(ctx, ODW_ERR_INVALID, "odw_timing_enable: null ctx");
  ctx->timing = on != 0;
  return ODW_OK;
}

int odw_timing_read(odw_ctx* ctx, double* total_ms, uint64_t* launches) {
  if (!ctx || !total_ms || !launches) return fail(ctx, ODW_ERR_INVALID, "odw_timing_read: bad argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
  for (auto& ev : ctx->events) {
    float ms = 0;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ev.first, ev.second));
    ctx->timing_ms += ms;
    ctx->timing_launches += 1;
    ctx->free_events.push_back(ev);
  }
  ctx->events.clear();
  *total_ms = ctx->timing_ms;
  *launches = ctx->timing_launches;
  ctx->timing_ms = 0;
  ctx->timing_launches = 0;
  return ODW_OK;
}

}  // extern "C"

#include "odw_posthoc.hip"
#include "odw_posthoc_batch.hip"
