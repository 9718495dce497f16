// icpk_ctx.h -- the context object behind the opaque icpk_ctx of include/icpk.h and the host helpers more than one
// host-side translation unit calls (icpk_api.cpp: context and clouds; icpk_sweep.cpp: NN sweeps and reductions;
// icpk_align.cpp: the alignment loops; icpk_batch.cpp: the frame-batch mode; icpk_frames_batch.cpp: its depth-stream
// entry; icpk_frontend.cpp: depth images;
// icpk_comm.cpp, icpk_map.cpp, icpk_fast.cpp, icpk_voxel.cpp, icpk_normals.cpp, icpk_filter.cpp, icpk_gicp.cpp,
// icpk_score.cpp, icpk_fpfh.cpp, icpk_global.cpp, icpk_posegraph.cpp, icpk_tsdf.cpp, icpk_projective.cpp, icpk_fern.cpp,
// icpk_brief.cpp, icpk_cluster.cpp, icpk_plane.cpp).  Not
// part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <thread>
#include <vector>

#include "icpk.h"
#include "icpk_internal.h"

struct icpk_ctx;

namespace icpk {

inline int hip_failure(icpk_ctx* ctx, const char* what, hipError_t e);  // ctx->err = what: <HIP's message>; ICPK_E_HIP

struct DeviceMem {
  static constexpr const char* name = "hipMalloc";
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static hipError_t free(void* p) { return hipFree(p); }
};
template <unsigned Flags>
struct PinnedMem {  // hipHostMalloc with these flags
  static constexpr const char* name = "hipHostMalloc";
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, Flags); }
  static hipError_t free(void* p) { return hipHostFree(p); }
};

// The one owner of a device or pinned allocation: a pointer and its capacity in elements.  reserve() grows it (the
// contents are lost: the old memory is freed before the new is allocated); the destructor frees it.  After a failed
// reserve the buffer is empty with capacity 0, so that the next call allocates again.  Movable, not copyable; it
// converts to T* so that it is handed to the launchers as the raw pointer.
template <class T, class Mem>
class Buf {
 public:
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) {
      (void)release();
      p_ = o.p_, cap_ = o.cap_;
      o.p_ = nullptr, o.cap_ = 0;
    }
    return *this;
  }
  ~Buf() { (void)release(); }

  operator T*() const { return p_; }
  T* get() const { return p_; }
  size_t capacity() const { return cap_; }

  // room for n elements: nothing happens while n <= capacity().  *grown (optional) is set when the old memory was
  // given up, whether or not the new allocation succeeded.
  int reserve(icpk_ctx* ctx, size_t n, bool* grown = nullptr) {
    if (n <= cap_) return ICPK_OK;
    if (grown) *grown = true;
    hipError_t e = release();
    if (e == hipSuccess) e = Mem::alloc(reinterpret_cast<void**>(&p_), n * sizeof(T));
    if (e != hipSuccess) {
      p_ = nullptr;
      return hip_failure(ctx, Mem::name, e);
    }
    cap_ = n;
    return ICPK_OK;
  }
  // frees the memory; the buffer is empty whatever HIP says
  hipError_t release() {
    const hipError_t e = p_ ? Mem::free(p_) : hipSuccess;
    p_ = nullptr;
    cap_ = 0;
    return e;
  }

 private:
  T* p_ = nullptr;
  size_t cap_ = 0;
};

template <class T>
using DevBuf = Buf<T, DeviceMem>;
template <class T, unsigned Flags = hipHostMallocDefault>
using PinnedBuf = Buf<T, PinnedMem<Flags>>;
template <class T>
using MappedBuf = PinnedBuf<T, hipHostMallocMapped>;  // pinned, and read by the device where it lies
template <class T>
using CoherentBuf = PinnedBuf<T, hipHostMallocMapped | hipHostMallocCoherent>;  // words the host and the device both watch

template <class B>
struct Need {
  B& buf;
  size_t n;
};
template <class B>
Need<B> need(B& buf, size_t n) { return {buf, n}; }

// Buffers that grow together: when any member is short, EVERY member is freed before any is allocated again (the peak
// is the new set alone, as it was the old set alone).  *grown as for Buf::reserve.
template <class... B>
int reserve_group(icpk_ctx* ctx, bool* grown, Need<B>... m) {
  if (((m.n <= m.buf.capacity()) && ...)) return ICPK_OK;
  if (grown) *grown = true;
  hipError_t e = hipSuccess;
  for (const hipError_t r : {m.buf.release()...})
    if (e == hipSuccess) e = r;
  int rc = e == hipSuccess ? ICPK_OK : hip_failure(ctx, "hipFree", e);
  ((rc = rc ? rc : m.buf.reserve(ctx, m.n)), ...);
  return rc;
}

struct Cloud {
  DevBuf<float> base;
  int n = 0;
  int cap = 0;  // floats per plane, multiple of NN_TILE
  float* x() const { return base; }
  float* y() const { return base + cap; }
  float* z() const { return base + 2 * (size_t)cap; }
};

inline int round_up(int v, int m) { return ((v + m - 1) / m) * m; }

// K1d's index of one cloud (kernels_grid.hip): the grid's geometry, the partial boxes it is made from, the cell table
// and the cloud's two float4 copies.  index_cloud (icpk_sweep.cpp) is the one place that builds into it; kernels that
// walk it take view().
struct GridIndex {
  DevBuf<GridInfo> info;
  DevBuf<float> bounds;    // GRID_BOUNDS_PARTS x 6
  DevBuf<int> cell_start;  // grid_max_cells + 1
  DevBuf<float4> t4;       // the cloud sorted by cell (x, y, z, original index)
  DevBuf<float4> o4;       // the cloud in the CALLER's order as (x, y, z, 0): K2's gather of the matched point is one 16-byte load
  GridView view() const { return GridView{t4, cell_start, info}; }
  // room for the index of n points: t4 / o4 hold round_up(n, NN_TILE) + 64 points and grow as a group; *grown
  // (optional) is set when their old contents are gone
  int reserve(icpk_ctx* ctx, int n, bool* grown = nullptr);
};

// The environment knobs, read once by icpk_create (tuning_from_env) and inherited whole by the
// frame-batch slots.  Every "diagnostic" knob selects a reference path the tests compare the default one against.
struct Tuning {
  int target_blocks = 16384;  // ICPK_NN_TARGET_BLOCKS: exact / filtered scan, blocks the target chunking aims at
  int q_per_lane = 0;         // ICPK_NN_Q: filtered scan, queries per lane (0 = auto)
  int slices = 0;             // ICPK_NN_SLICES: pruned scan, lanes per query (0 = by cloud size)
  float grid_ppc = 8.f;       // ICPK_GRID_PPC: aimed-at targets per occupied cell (measured best on configs 2, 3 and the dense pair: 8)
  int grid_xdiv = 4;          // ICPK_GRID_XDIV: cells are this many times finer along x (measured best on config 2: 4)
  int grid_slices = 0;        // ICPK_GRID_SLICES: lanes per query (0 = by cloud size)
  int merged_setup = 1;       // ICPK_MERGED_SETUP=0: a fresh pair's two counting sorts one after the other
  int batch_group = 16;       // ICPK_BATCH_GROUP: pairs advancing in lock step (<= BATCH_MAX)
  int batch_threads = 4;      // ICPK_BATCH_THREADS: host threads sharing a group's set-up calls
  int batch_setup = 1;        // ICPK_BATCH_SETUP: 0 per-pair set-up launches on the slots' own streams; 2 batched launches
                              //   for single-group host-pointer batches too; 3 as 2, replayed pair by pair (test hook)
  bool pristine_skip = true;     // ICPK_PRISTINE_SKIP=0: always copy the committed source (diagnostic)
  bool pixel_seeds = true;       // ICPK_PIXEL_SEEDS=0: the reference's literal seed (diagnostic)
  bool lazy_unpack = true;       // ICPK_LAZY_UNPACK=0: unpack the records at the end of every device loop (diagnostic)
  bool image_order = true;       // ICPK_IMAGE_ORDER=0: sort the queries of an image-ordered source by cell like any other (diagnostic)
  bool zero_copy_upload = true;  // ICPK_ZERO_COPY_UPLOAD=0: copy-engine transfer from the staging buffer instead (diagnostic)
  bool result_mirror = true;     // ICPK_RESULT_MIRROR=0: copy the state back and wait for the stream instead (diagnostic)
  int loop_ahead = 1;            // ICPK_LOOP_AHEAD: iterations kept enqueued ahead of the device in a loop that may exit
                                 //   early (0: enqueue every iteration up front)
};

// icpk_align_frames_batch: one depth stream's resident frame, kept by the parent context (slots rotate between the
// two slot sets, a stream does not).  As icpk_backproject_pair's own: two image slots of rows x cols in raw and
// filtered form, the new frame goes where the resident one is not.
struct FrameStream {
  DevBuf<uint16_t> raw, flt;
  int slot = -1;  // -1: no resident frame
  int rows = 0, cols = 0;
  int filter[6] = {0, 0, 0, 0, 0, 0};  // settings the resident filtered copy was made with (as icpk_ctx::frame_filter)
  unsigned long long sub_images = 0;   // images of this stream since icpk_set_subsample (its subsample keys)
};
// icpk_get_frames_trace's record of one job of the last icpk_align_frames_batch call
struct FrameTrace {
  std::vector<float> R, t, mse;
  std::vector<int32_t> pairs;
};

}  // namespace icpk

using icpk::nn_key_t;
using icpk::LoopState;
using icpk::GridInfo;
using icpk::NSUM;

struct icpk_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  icpk::Tuning tune;
  icpk::Cloud tgt, src0, src;
  icpk::Cloud nrm;  // target normals (point-to-plane), same indexing as tgt
  bool have_normals = false;
  icpk::Cloud dec;  // every NN_SEED_STRIDE-th target (seeding pre-pass of the filtered NN)
  bool have_tgt = false, have_src = false, have_assoc = false;
  bool have_dec = false;   // dec matches tgt
  bool have_boxes = false; // boxes match tgt
  icpk::DevBuf<float> boxes;  // [6][tbox_stride] tile boxes then [6][sbox_stride] sub-tile boxes
  int boxes_tiles_cap = 0;
  // pruned scan: Morton-ordered copy of the target, its permutation, the query order
  icpk::Cloud sorted;
  icpk::DevBuf<int> tperm;
  icpk::DevBuf<unsigned> tkeys;    // sorted Morton codes of the target (first-sweep seeding)
  icpk::DevBuf<int> qperm;
  bool have_qperm = false;
  icpk::DevBuf<float> bounds;      // 6 floats: lo xyz, hi xyz of the target
  icpk::DevBuf<unsigned> sort_keys;  // 2 x sort_cap
  icpk::DevBuf<int> sort_vals;       // sort_cap
  int sort_cap = 0;
  icpk::DevBuf<GridInfo> morton_table;  // the table size of the Morton counting sort (pruned scan), for launch_grid_scan
  bool have_seed = false;  // `best` holds matches of a previous sweep of the same clouds
  icpk::DevBuf<nn_key_t> best, seed;  // the association set (ensure_assoc): these six grow together
  icpk::DevBuf<nn_key_t> best_m, seed_m;  // pruned scan: results / seeds in query Morton order
  bool have_seed_m = false;    // best_m holds the matches of the previous sweep under the current qperm
  icpk::DevBuf<int32_t> idx;
  icpk::DevBuf<float> dist;
  icpk::DevBuf<double> partial;
  icpk::DevBuf<int> pcount;
  icpk::DevBuf<double> red_out;      // 20 x 8 bytes
  icpk::PinnedBuf<double> red_host;  // 20 x 8 bytes
  icpk::DevBuf<LoopState> st_dev_mem;      // this context's own loop state (released by a frame-batch slot) ...
  icpk::PinnedBuf<LoopState> st_host_mem;  // ... and its staging copy
  LoopState* st_dev = nullptr;   // views, not owners: the device-side loop state (st_dev_mem, or a slot's place in
  LoopState* st_host = nullptr;  //   the parent's slot_states) and its staging copy (st_host_mem, or slot_states_host)
  icpk::CoherentBuf<int> progress;  // LoopState::progress of a throttled loop (see there)
  int* progress_dev = nullptr;    // view: the same words as the device addresses them
  int loop_epoch = 0;             // tag of the current throttled loop in the progress words
  icpk::CoherentBuf<LoopState> st_mirror;  // the loop's outputs as the device writes them at its end (LoopState::mirror)
  LoopState* st_mirror_dev = nullptr;    // view: the same memory as the device addresses it
  icpk::LoopInitArgs pending_init{};         // device_loop_begin(defer): the initial LoopState not launched yet
  bool init_pending = false;
  icpk::DevBuf<int> grid_ticket;       // grid_begin_kernel's arrival counter (zero between launches)
  int sub_factor = 0;                  // icpk_set_subsample: keep one valid pixel in sub_factor (<= 1: all), chosen by ...
  unsigned long long sub_seed = 0;     // ... a hash of this seed, the image's stream number and the pixel
  unsigned long long sub_stream = 0;   // images back-projected since icpk_set_subsample (every image draws a fresh pattern, as rand() would)
  struct HostRange {                   // icpk_register_host_buffer: caller memory pinned and mapped for the device
    const char* host;
    size_t bytes;
    const char* dev;
  };
  std::vector<HostRange> registered;
  icpk::PinnedBuf<uint16_t> stage_depth;  // icpk_backproject_pair's images on their way to the device
  icpk::DevBuf<int> pix_tidx;  // icpk_backproject_pair: the target point of every pixel (-1: none) ...
  icpk::DevBuf<int> pix_src;   // ... and the pixel of every source point: image-space seeds of the alignment that follows
  bool have_pix_seed = false;          // they describe the clouds the context holds now
  int pix_rows = 0, pix_cols = 0;
  bool src_pristine = false;     // the working source equals the committed one (see copy_src0_to_src)
  // the working source logically equals the committed one but its planes have not been written (copy_src0_to_src
  // defers the copy): ensure_unpacked brings them up to date for whoever reads them; a device loop of grid sweeps never
  // does (its set-up takes the queries from src0, see query_cloud, and its unpack rewrites every entry)
  bool src_deferred = false;
  const int* stop = nullptr;     // &st_dev->done while a device loop is being enqueued, else null
  LoopState* st_active = nullptr;  // st_dev while a device loop is being enqueued, else null
  icpk::PinnedBuf<float> stage_t, stage_s;  // staging of host clouds (frame-batch slots): target, source
  icpk::DevBuf<uint16_t> depth_dev;
  icpk::DevBuf<uint16_t> depth_flt;  // filtered depth image (icpk_filter_depth_image / icpk_backproject_filtered)
  // K22: the two tables of the bilateral rule on the device (ws, then wr), made again only when the parameters change
  icpk::DevBuf<uint16_t> bil_tables;
  std::vector<uint16_t> bil_tables_host;  // what the upload reads: it lives as long as a copy may be in flight
  icpk_bilateral_params bil_params = {0, 0.f, 0.f, 0};  // radius 0: no tables yet
  int bil_K = 0;
  icpk::DevBuf<int32_t> ks_buf;  // key-point association lists: assoc_q | assoc_t | assoc_d | rej_q, a quarter of it each
  // icpk_backproject_pair keeps the current frame's image on the device (slot frame_slot of depth_dev / depth_flt, two
  // slots of half their capacity): it is the next call's `previous` (SLAM.cpp:305) and need not cross PCIe again
  int frame_slot = -1;               // -1: no resident frame
  int frame_rows = 0, frame_cols = 0;
  int frame_filter[6] = {0, 0, 0, 0, 0, 0};  // filter settings the resident filtered copy was made with (on, max, min, morph, ax, ay)
  icpk::DevBuf<int> bp_counts;
  icpk::PinnedBuf<int> bp_n_host;
  std::vector<hipEvent_t> events;
  std::vector<float> trace_R, trace_t, trace_mse;  // per-iteration record of the last align
  std::vector<int32_t> trace_pairs;
  // robust alignment (icpk_set_robust, K10): the setting, the selection's state and scratch, and the record of the last
  // alignment (icpk_get_robust_trace; the device loop writes it straight into the mapped robust_trace_pin)
  bool robust_on = false;
  icpk_robust robust{};
  icpk::DevBuf<icpk::RobustSel> rsel;
  icpk::PinnedBuf<icpk::RobustSel> rsel_host;
  icpk::DevBuf<int> rhist;        // 2 x SEL_BINS, zero between selections
  icpk::DevBuf<unsigned> rdsel;   // the accepted distance patterns of the sweep being selected
  icpk::CoherentBuf<icpk::RobustTraceEntry> robust_trace_pin;  // LOOP_MAX_ITER entries
  icpk::RobustTraceEntry* robust_trace_dev = nullptr;          // view: the same memory as the device addresses it
  std::vector<icpk::RobustTraceEntry> robust_trace;
  // K1d's index (grid scan ICPK_NN_GRID, K12 .. K17): `grid` is the target's, valid while have_grid.  `aux_grid` is the
  // index of any OTHER cloud (K13: the working source; K14 / K16: the uploaded source): index_aux builds it, the call
  // that built it reads it, and the next call that builds one overwrites it -- nothing caches it or reads it later
  icpk::GridIndex grid, aux_grid;
  int grid_max_cells = icpk::GRID_MAX_CELLS;  // capacity of the cell tables / qcount / qstart (a frame-batch slot: GRID_MAX_CELLS_SLOT)
  icpk::DevBuf<float4> qm4;     // queries in scan order (x, y, z, original index)
  icpk::DevBuf<float4> sp_in;   // seeds as points, scan order: read by the next grid sweep
  icpk::DevBuf<float4> sp_out;  // ... written by it
  icpk::DevBuf<float4> rec;     // device loop behind grid sweeps: caller-order records {(query, distance), (match, index)}, 2 float4 per query -- what K2 reads
  bool rec_pending = false;  // the last device loop left planes / keys to be unpacked from qm4 / rec on demand (ensure_unpacked)
  // frame-batch mode: child contexts (one per pair in flight; own stream for set-up work) --
  // owned by the parent, never handed out
  std::vector<icpk_ctx*> slots;
  hipEvent_t ready_ev = nullptr;       // slot: set-up of the current pair is enqueued up to here
  hipEvent_t group_ev[2] = {nullptr, nullptr};  // parent: the lock-step loop of a slot set has finished
  hipStream_t setup_stream[2] = {nullptr, nullptr};  // parent: the batched set-up launches of a slot set (created on first use)
  hipEvent_t setup_ev[2] = {nullptr, nullptr};       // ... and their completion
  hipEvent_t batch_t0[2] = {nullptr, nullptr}, batch_t1[2] = {nullptr, nullptr};  // parent: params.profile = 1 in the
  bool batch_timed[2] = {false, false};                                           //   frame-batch mode: one sweep per group
  icpk::DevBuf<LoopState> slot_states;          // parent: the loop states of all slots in one allocation (slot k at [k]),
  icpk::PinnedBuf<LoopState> slot_states_host;  //   so that a group's states come back with ONE copy; pinned mirror
  std::vector<nn_key_t*> best_of_sweep;  // device loop: which buffer each enqueued sweep wrote
  // icpk_align_frames_batch (icpk_frames_batch.cpp), parent only: the streams' resident frames (ICPK_MAX_FRAME_STREAMS
  // entries once used), the pinned staging of a group's new images, per slot set the block counts and the totals the
  // scans publish (device and mapped), and the traces of the last call's jobs
  std::vector<icpk::FrameStream> frame_streams;
  icpk::PinnedBuf<uint16_t> fb_stage;
  icpk::DevBuf<int> fb_counts[2];
  icpk::DevBuf<int> fb_n_dev;
  icpk::CoherentBuf<int> fb_n;  // 2 sets x 2 BATCH_MAX words
  int* fb_n_mapped = nullptr;   // view: fb_n as the device addresses it
  std::vector<icpk::FrameTrace> frames_trace;
  // RCCL communicator of the frame-batch / query-sharded modes (icpk_comm.cpp); null until
  // icpk_comm_init_rccl
  struct icpk_comm_state* comm = nullptr;
  // voxel certainty map (icpk_map.cpp); null until the first icpk_map_* call
  struct icpk_map_state* map = nullptr;
  unsigned map_version = 0;       // bumped by every change of the map (update, set_points, reset, release)
  bool tgt_lookup = false;        // the target is icpk_map_lookup_to_target's [key points | points | zero point] ...
  unsigned tgt_lookup_version = 0;  // ... of this map version
  // FAST key points (icpk_fast.cpp); null until the first icpk_detect_fast / icpk_bgr_to_gray call
  struct icpk_fast_state* fast = nullptr;
  icpk::DevBuf<int> qcount;     // query counting sort by cell: counts and starts, grid_max_cells + 1 each
  icpk::DevBuf<int> qstart;
  bool qcount_dirty = false; // a counting sort was cut short: clear the whole count table before the next one
  icpk::DevBuf<int> scan_bsum;  // block sums of the cell-count scans (GRID_SCAN_BLOCKS ints)
  // a fresh pair sorts targets and queries side by side (build_grid_and_order): second count table, block sums and slots
  icpk::DevBuf<int> qcount2;
  bool qcount2_dirty = false;
  icpk::DevBuf<int> scan_bsum2;
  icpk::DevBuf<int> sort_vals2;
  // voxel-grid downsampling (icpk_voxel_downsample, K11; icpk_voxel.cpp): the table, the per-point scratch, the
  // downsampled planes on their way into the cloud, and the grouping of the last call (icpk_get_voxel_groups)
  icpk::DevBuf<icpk::VoxelSlot> vox_table;
  icpk::DevBuf<int> vox_slot;    // [n_in]
  icpk::DevBuf<int> vox_bsum;    // [ceil(n_in / 1024)]
  icpk::DevBuf<int> vox_counts;  // n_out, n_dropped ...
  icpk::PinnedBuf<int> vox_counts_host;  // ... and where the host reads them
  icpk::DevBuf<float> vox_out;   // 3 planes of n_in floats (6 with normals)
  icpk::DevBuf<int> vox_first, vox_count;  // [n_out]
  icpk::DevBuf<int> vox_oop;               // [n_in]
  bool have_vox = false;         // a downsample has run: the three above describe it
  int vox_n_in = 0, vox_n_out = 0;
  // target normals from the target's geometry (icpk_estimate_target_normals, K12; icpk_normals.cpp): what
  // icpk_get_normal_stats returns, kept on the device until asked for
  icpk::DevBuf<long long> nrm_moments;   // [n][NRM_MOMENTS]
  icpk::DevBuf<int> nrm_count;           // [n]
  icpk::DevBuf<float> nrm_curv;          // [n]
  icpk::DevBuf<int> nrm_valid;           // points with a normal ...
  icpk::PinnedBuf<int> nrm_valid_host;   // ... and where the host reads it
  bool have_nstats = false;      // the four above describe the normals of the target the context holds now
  bool nstats_moments = false;   // ... and the caller asked for the moments to be kept
  int nstats_n = 0;
  // outlier removal (icpk_remove_outliers, K13; icpk_filter.cpp): the statistics of the last call
  // (icpk_get_outlier_stats), the scratch of the threshold and the compaction, the filtered planes on their way into
  // the cloud (the index it walks is the target's, or aux_grid for the working source)
  icpk::DevBuf<double> flt_value;    // [n_in]
  icpk::DevBuf<float> flt_kth;       // [n_in]
  icpk::DevBuf<int> flt_oidx;        // [n_in]
  icpk::DevBuf<double> flt_summary;  // 4
  icpk::PinnedBuf<double> flt_summary_host;
  icpk::DevBuf<double> flt_partial;  // 2 x RED_MAX_BLOCKS
  icpk::DevBuf<int> flt_pcount;      // RED_MAX_BLOCKS
  icpk::DevBuf<int> flt_bsum;        // [ceil(n_in / 1024)]
  icpk::DevBuf<int> flt_counts;      // n_out, n_dropped ...
  icpk::PinnedBuf<int> flt_counts_host;  // ... and where the host reads them
  icpk::DevBuf<float> flt_out;       // 3 planes of n_in floats (6 with normals)
  bool have_flt = false;             // a filter has run: the record describes it
  int flt_n_in = 0, flt_n_out = 0, flt_n_finite = 0, flt_kind = 0, flt_min_neighbors = 0;
  // plane-to-plane flavour (ICPK_SOLVE_PLANE_TO_PLANE, K14; icpk_gicp.cpp): the normals of the UPLOADED source in the
  // caller's order (dropped with it: ensure_cloud, icpk_commit_source), the setting, and -- for
  // icpk_estimate_source_normals only -- K12's scratch in buffers of their own (the index it walks is aux_grid)
  icpk::Cloud snrm;
  bool have_src_normals = false;
  float gicp_epsilon = 1e-3f;
  icpk::DevBuf<long long> sn_moments;  // [n][NRM_MOMENTS]
  icpk::DevBuf<int> sn_count;          // [n]
  icpk::DevBuf<float> sn_curv;         // [n]
  icpk::DevBuf<int> sn_valid;          // 1
  // colored ICP (K17; icpk_color.cpp): one intensity per point of the target and of the UPLOADED source (caller's
  // order; dropped with their cloud: target_changed, ensure_cloud), the target's colour gradients (rotated with the
  // target's normals, dropped with the target or its colours), the ten sums per point behind them and the setting
  icpk::DevBuf<float> tcol, scol;        // [n]
  icpk::DevBuf<float> tcol_sorted;       // [n] the target's intensities in cell order (scratch of the estimate)
  icpk::Cloud cgrad;
  icpk::DevBuf<long long> cg_sums;       // [n][COLOR_SUMS]
  bool have_tgt_colors = false, have_src_colors = false, have_color_gradients = false;
  bool have_cg_sums = false;             // cg_sums describes the target as it stands, and the caller asked to keep it
  bool colored_on = false;
  float lambda_geometric = 0.968f;
  // pose scoring (icpk_score_poses, K15; icpk_score.cpp): the poses on their way to the device, the keys of every
  // (pose, point) -- of one chunk of poses, or of the whole call when the associations are kept --, the canonical
  // tree's scratch and the results
  icpk::PinnedBuf<float> score_T_host;   // 16 x n_poses
  icpk::DevBuf<float> score_T;
  icpk::DevBuf<nn_key_t> score_keys;     // [chunk][ns] ...
  icpk::DevBuf<nn_key_t> score_kept;     // ... or, with ICPK_SCORE_KEEP_ASSOC, [n_poses][ns] in a buffer of their own
  icpk::DevBuf<double> score_partial;    // [chunk][NSCORE][RED_MAX_BLOCKS]
  icpk::DevBuf<int> score_pcount;        // [chunk][RED_MAX_BLOCKS]
  icpk::DevBuf<double> score_out;        // [n_poses][NSCORE + 1]
  icpk::PinnedBuf<double> score_out_host;
  bool have_score_assoc = false;   // score_kept holds every pose of the last ICPK_SCORE_KEEP_ASSOC call on the current clouds
  int score_n_poses = 0, score_ns = 0;
  // FPFH descriptors and their matches (icpk_compute_fpfh / icpk_match_features / icpk_register_global, K16;
  // icpk_fpfh.cpp, icpk_global.cpp): per cloud ([0] the uploaded source, [1] the target) the normals in cell order, the
  // 16-bit SPFH, the kept counts and the descriptors; the best keys of both directions and the kept pairs
  struct FpfhSide {
    icpk::DevBuf<float4> n4;          // [n] cell order
    icpk::DevBuf<unsigned short> g;   // [n][FPFH_G_STRIDE] cell order
    icpk::DevBuf<int> counts, m;      // [n][FPFH_BINS], [n] (ICPK_FPFH_KEEP_SPFH)
    icpk::DevBuf<float> desc;         // [n][FPFH_BINS] caller's order
    icpk::DevBuf<uint8_t> valid;      // [n]
    bool have = false;                // they describe the cloud and the normals the context holds now
    bool kept_spfh = false;
    int n = 0;
  } fpfh[2];
  icpk::DevBuf<nn_key_t> match_best[2];  // [ns], [nt]
  icpk::DevBuf<int> match_src, match_tgt;  // [ns]
  icpk::DevBuf<float> match_D;             // [ns]
  icpk::DevBuf<int> match_n;               // the number of kept pairs ...
  icpk::PinnedBuf<int> match_n_host;       // ... and where the host reads it
  bool have_matches = false;       // the pairs belong to the descriptors both sides hold now
  // pose-graph optimisation (icpk_pose_graph_optimize / _evaluate, K18; icpk_posegraph.cpp): the edges and the
  // adjacency list on the device, per edge two linearisations' blocks, per node the two sets of poses, two
  // linearisations' blocks and the solver's vectors, the reductions' slots, the words the host reads once per LM
  // iteration, and the record of the last optimize (icpk_get_pose_graph_trace).  Nothing else of the context is used
  icpk::DevBuf<icpk::PgEdge> pg_edges;   // [n_edges]
  icpk::DevBuf<int> pg_adj;              // [n_nodes + 1] starts, then [2 n_edges] entries
  icpk::DevBuf<double> pg_edge_f64;      // 2 x n_edges x 44: A, b, chi2, l of either linearisation
  icpk::DevBuf<double> pg_node_f64;      // n_nodes x (2 x 16 + 2 x 42 + 36 + 5 x 6)
  icpk::DevBuf<double> pg_partial;       // PG_NPARTIAL x RED_MAX_BLOCKS
  icpk::DevBuf<icpk::PgScalars> pg_scal;
  icpk::PinnedBuf<icpk::PgScalars> pg_scal_host;
  std::vector<double> pg_trace_cost, pg_trace_lambda;
  std::vector<int32_t> pg_trace_pcg, pg_trace_accepted;
  // TSDF volume (icpk_tsdf.cpp, K19); null until icpk_tsdf_create
  struct icpk_tsdf_state* tsdf = nullptr;
  int loop_nact = icpk::NSUM;      // device loop: sums the running alignment's step consumes (NSUM_REF or NSUM)
  int profile_phase = 0;     // alignments profiled so far (offsets the sampled launches, see profile_stride)
  int qperm_kind = 0;        // what qperm holds: 1 Morton order (pruned scan), 2 cell order (grid scan)
  bool grid_chain = false;   // device loop only: the previous sweep was a grid sweep (qm4 / sp_in current)
  bool have_grid = false;  // grid matches tgt
  std::string err;
  icpk_log_fn log_fn = nullptr;
  void* log_user = nullptr;
  std::chrono::steady_clock::time_point log_last;
  // K24: the depth pyramid of the last icpk_depth_pyramid_build, every level in this one buffer (level l at pyr_off[l]),
  // resident until the next build.  (Kept behind every older member: the code that does not use the pyramid is compiled
  // against the offsets it had before.)
  icpk::DevBuf<uint16_t> pyr;
  int pyr_levels = 0;  // 0: no pyramid yet
  int pyr_rows[ICPK_PYRAMID_MAX_LEVELS] = {0}, pyr_cols[ICPK_PYRAMID_MAX_LEVELS] = {0};
  size_t pyr_off[ICPK_PYRAMID_MAX_LEVELS] = {0};
  // K25 (icpk_projective.cpp), behind the pyramid for the same reason: the canonical tree's scratch of the projective
  // reduction, its final sums, the loop's state + trace on the device and where the host reads them, the per-pixel
  // outputs of icpk_projective_associate, and the record of the last icpk_align_projective
  icpk::DevBuf<double> proj_partial;  // NP2L x RED_MAX_BLOCKS
  icpk::DevBuf<int> proj_pcount;      // RED_MAX_BLOCKS
  icpk::DevBuf<double> proj_out;      // NP2L sums, then the count as an int64
  icpk::PinnedBuf<double> proj_out_host;
  icpk::DevBuf<icpk::ProjBlock> proj_block;
  icpk::PinnedBuf<icpk::ProjBlock> proj_block_host;
  icpk::DevBuf<int32_t> proj_pixel;  // [rows_s cols_s]
  icpk::DevBuf<float> proj_dist;     // [rows_s cols_s]
  std::vector<icpk_projective_iter> proj_trace;
  // K26: the intensity pyramid beside the depth pyramid (level l at pyr_off[l], floats), set by
  // icpk_depth_pyramid_set_intensity and dropped by the next build; the K the resident depth pyramid was built with
  icpk::DevBuf<float> pyr_int;
  bool pyr_have_int = false;
  int pyr_K = 0;
  // K27 (icpk_fern.cpp), behind everything older for the same reason: the keyframe database of icpk_fern_create -- the
  // table the codes are drawn with, the codes transposed (word w of keyframe k at w * capacity + k), the poses on the
  // host beside them --, the current code (F / 8 words, then V), the search's lists and answer, and where the host
  // reads code, V and answer.  A pyramid build clears fern_code_current and touches nothing else of these
  bool have_fern = false;
  icpk_fern_params fern_params{};
  int fern_rows = 0, fern_cols = 0;
  int fern_n = 0;
  icpk::DevBuf<int32_t> fern_table;    // F x 6
  icpk::DevBuf<uint32_t> fern_db;      // F / 8 x capacity
  icpk::DevBuf<uint32_t> fern_code;    // F / 8 code words | V | the answer's 8 keys
  icpk::DevBuf<uint32_t> fern_lists;   // ceil(capacity / 256) x 8
  icpk::PinnedBuf<uint32_t> fern_host; // fern_code's mirror
  std::vector<double> fern_poses;      // 16 per keyframe
  bool fern_code_current = false;      // the current code is of the resident pyramid
  int fern_code_valid = 0;             // ... and its V
  // K28 (icpk_frame_view.cpp), behind everything older for the same reason: the frame view -- a snapshot of the pyramid
  // as eight planes per level, null until the first icpk_frame_view_build, outside the TSDF state and untouched by it
  // and by the pyramid builds -- and which view the projective calls read (icpk_projective_set_view)
  struct icpk_frame_view_state* fview = nullptr;
  int proj_view_which = ICPK_VIEW_RAYCAST;
  int proj_view_level = 0;
  // K29 (icpk_sdf_track.cpp), behind everything older for the same reason: the scratch of the SDF tracking calls -- the
  // tree's partials, the final sums, the loop's state + trace (K25's block type) and where the host reads them, the
  // per-pixel outputs of icpk_sdf_associate -- and the record of the last icpk_align_sdf.  K25's own stay as they are
  icpk::DevBuf<double> sdf_partial;  // NP2L x RED_MAX_BLOCKS
  icpk::DevBuf<int> sdf_pcount;      // RED_MAX_BLOCKS
  icpk::DevBuf<double> sdf_out;      // NP2L sums, then the count as an int64
  icpk::PinnedBuf<double> sdf_out_host;
  icpk::DevBuf<icpk::ProjBlock> sdf_block;
  icpk::PinnedBuf<icpk::ProjBlock> sdf_block_host;
  icpk::DevBuf<int32_t> sdf_cell;  // [rows_s cols_s]
  icpk::DevBuf<float> sdf_value;   // [rows_s cols_s]
  std::vector<icpk_projective_iter> sdf_trace;
  // K31 (icpk_esdf.cpp), behind everything older for the same reason: the Euclidean distance map of the TSDF volume -- a
  // snapshot in a state of its own, null until the first icpk_esdf_compute.  icpk_tsdf.cpp drops it (icpk_esdf_drop)
  // where the volume is created, reset, set, shifted or released; nothing else of the context reads or writes it
  struct icpk_esdf_state* esdf = nullptr;
  // K32 (icpk_brief.cpp), behind everything older for the same reason: the two descriptor slots, the image of
  // icpk_describe_points and the match lists, in a state of their own, null until the first describe or set call.
  // brief_map[w]: slot w's key point -> cloud index map describes cloud w as it stands (icpk_described_to_cloud);
  // fpfh_dropped clears it with everything else that speaks of a cloud that is being replaced
  struct icpk_brief_state* brief = nullptr;
  bool brief_map[2] = {false, false};
  // K33 (icpk_cluster.cpp), behind everything older for the same reason: the record of the last icpk_cluster_dbscan
  // (icpk_get_clusters), kept on the device until asked for, the union-find forest and the compaction's scratch, and the
  // selected planes on their way into the cloud (the index it walks is the target's, or aux_grid for the working source)
  icpk::DevBuf<int> cl_labels;       // [n_in]
  icpk::DevBuf<uint8_t> cl_core;     // [n_in]
  icpk::DevBuf<int> cl_count;        // [n_in]
  icpk::DevBuf<int> cl_nearest;      // [n_in]
  icpk::DevBuf<int> cl_oidx;         // [n_in]
  icpk::DevBuf<int> cl_sizes;        // [n_clusters <= n_in]
  icpk::DevBuf<int> cl_first;        // [n_clusters <= n_in]
  icpk::DevBuf<int> cl_parent;       // [n_in] scratch: the forest over the core points
  icpk::DevBuf<int> cl_cid;          // [n_in] scratch: a representative's cluster id
  icpk::DevBuf<int> cl_bsum;         // [ceil(n_in / 1024)]
  icpk::DevBuf<int> cl_counts;       // CL_COUNTS words: clusters, noise, kept, dropped, the error word, the largest ...
  icpk::PinnedBuf<int> cl_counts_host;  // ... and where the host reads them
  icpk::DevBuf<float> cl_out;        // 3 planes of n_in floats (6 with normals)
  bool have_cl = false;              // a clustering has run: the record describes it
  int cl_n_in = 0, cl_n_clusters = 0;
  // K34 (icpk_plane.cpp), behind everything older for the same reason: the record of the last icpk_segment_planes
  // (icpk_get_planes), kept on the device until asked for, the rounds' scratch, and the selected planes on their way into
  // the cloud.  No index is built or read
  icpk::DevBuf<int> pl_labels;       // [n_in]
  icpk::DevBuf<int> pl_oidx;         // [n_in]
  icpk::DevBuf<float4> pl_E;         // [n_in] scratch: a round's list of open points
  icpk::DevBuf<int> pl_bsum;         // [ceil(n_in / 1024)]
  icpk::DevBuf<int> pl_counts;       // (PL_MAX_PLANES + 1) x PL_COUNTS words: one block per round, one for the selection ...
  icpk::PinnedBuf<int> pl_counts_host;  // ... and where the host reads a round's
  icpk::DevBuf<double> pl_hyp;       // [8 n_hypotheses]: a PlaneHyp is 64 bytes
  icpk::DevBuf<int> pl_hidx;         // [3 n_hypotheses]
  icpk::DevBuf<int> pl_hcount;       // [n_hypotheses]
  icpk::DevBuf<double> pl_partial;   // [9][RED_MAX_BLOCKS]
  icpk::DevBuf<int> pl_pcount;       // [RED_MAX_BLOCKS]
  icpk::DevBuf<double> pl_model;     // [PL_MAX_PLANES][8]
  icpk::DevBuf<int> pl_info;         // [PL_MAX_PLANES][6]
  icpk::DevBuf<double> pl_sums;      // [PL_MAX_PLANES][9]
  icpk::DevBuf<float> pl_out;        // 3 planes of n_in floats (6 with normals)
  bool have_pl = false;              // a segmentation has run: the record describes it
  int pl_n_in = 0, pl_n_planes = 0;
};

#define ICPK_HIP(ctx, call)                                                                      \
  do {                                                                                           \
    hipError_t e__ = (call);                                                                     \
    if (e__ != hipSuccess) {                                                                     \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__);                           \
      return ICPK_E_HIP;                                                                         \
    }                                                                                            \
  } while (0)

void icpk_comm_release(icpk_ctx* ctx);  // called by icpk_destroy
void icpk_map_free(icpk_ctx* ctx);      // called by icpk_destroy (icpk_map.cpp)
void icpk_fast_free(icpk_ctx* ctx);     // called by icpk_destroy (icpk_fast.cpp)
void icpk_tsdf_free(icpk_ctx* ctx);     // called by icpk_destroy (icpk_tsdf.cpp)
void icpk_frame_view_free(icpk_ctx* ctx);  // called by icpk_destroy (icpk_frame_view.cpp)
void icpk_esdf_free(icpk_ctx* ctx);     // called by icpk_destroy (icpk_esdf.cpp)
void icpk_esdf_drop(icpk_ctx* ctx);     // the distance map no longer describes the volume: its getters answer ICPK_E_NOT_SET
void icpk_brief_free(icpk_ctx* ctx);    // called by icpk_destroy (icpk_brief.cpp)
int icpk_comm_allreduce_device(icpk_ctx* ctx, double* dev, int n);  // in-stream sum over the ranks (icpk_comm.cpp)
// ICPK_NN_MAP: one K9 sweep of the working source against the map into ctx->best (icpk_map.cpp); the target must be
// the map's current lookup target
int icpk_map_nn_sweep(icpk_ctx* ctx);
bool icpk_map_lookup_current(const icpk_ctx* ctx);

namespace icpk {

inline int fail(icpk_ctx* ctx, int code, const char* msg) {
  if (ctx) ctx->err = msg;
  return code;
}

// the cloud `which` (0 the uploaded source, 1 the target) or its normals have changed: K16's descriptors and matches
// speak of what was there before, and so does K32's map from slot `which`'s key points into the cloud
inline void fpfh_dropped(icpk_ctx* ctx, int which) {
  ctx->fpfh[which].have = false;
  ctx->have_matches = false;
  ctx->brief_map[which] = false;
}

inline int hip_failure(icpk_ctx* ctx, const char* what, hipError_t e) {
  if (ctx) ctx->err = std::string(what) + ": " + hipGetErrorString(e);
  return ICPK_E_HIP;
}

// The host wait on words the device writes into pinned, mapped memory: spins until done() (the wait is short), yields
// now and then, and looks at the stream every 20 ms -- not more often: a stream query may itself put a marker into the
// queue -- so that a faulted kernel ends the wait with an error instead of hanging the caller.  A stream that has
// drained while done() still says no: `stalled`.
// stream: the one whose work the words wait for (nullptr: ctx->stream)
template <class Done>
int spin_until(icpk_ctx* ctx, Done done, const char* stalled, hipStream_t stream = nullptr) {
  auto t_query = std::chrono::steady_clock::now() + std::chrono::milliseconds(20);
  for (unsigned spin = 1; !done(); ++spin) {
    __builtin_ia32_pause();
    if ((spin & 0x3ff) != 0) continue;
    std::this_thread::yield();
    const auto now = std::chrono::steady_clock::now();
    if (now < t_query) continue;
    t_query = now + std::chrono::milliseconds(20);
    const hipError_t q = hipStreamQuery(stream ? stream : ctx->stream);
    if (q == hipSuccess) return done() ? ICPK_OK : fail(ctx, ICPK_E_HIP, stalled);  // (drained: the words are final)
    if (q != hipErrorNotReady) return fail(ctx, ICPK_E_HIP, hipGetErrorString(q));
  }
  return ICPK_OK;
}

// ---- icpk_api.cpp: context and clouds ----
// stream + the fixed-size buffers every context owns; `parent` != nullptr: a frame-batch slot (inherits the tuning)
icpk_ctx* make_context(int device_id, const icpk_ctx* parent);
int check_ready(icpk_ctx* ctx);  // both clouds set, target not empty
// k: hipMemcpyHostToDevice or hipMemcpyDeviceToDevice; sync = false: the caller keeps the host buffers alive and
// synchronises later (frame-batch slots)
int set_target_impl(icpk_ctx* ctx, const float* x, const float* y, const float* z, int32_t n, hipMemcpyKind k,
                    bool sync = true);
int set_source_impl(icpk_ctx* ctx, const float* x, const float* y, const float* z, int32_t n, hipMemcpyKind k,
                    bool sync = true);
int copy_src0_to_src(icpk_ctx* ctx);  // the working source := the committed one (its planes on demand: src_deferred)
// the planes of the committed source into the working one, now (tail_only: just the padding behind the n points)
int copy_source_planes(icpk_ctx* ctx, bool tail_only);
// the target planes hold tgt.n points that replace the previous target: its +inf padding up to the next NN_TILE multiple
int pad_target(icpk_ctx* ctx);
// the target has changed (replaced, or moved with keep_normals = true): drop everything derived from it
void target_changed(icpk_ctx* ctx, bool keep_normals);
void reset_outputs(float T_out[16], icpk_stats* stats);  // identity, zeroed statistics (what a failed alignment returns)
void clear_trace(icpk_ctx* ctx);                        // icpk_get_trace's record of the last alignment

// ---- icpk_sweep.cpp: device buffers, NN sweeps, reductions ----
int ensure_cloud(icpk_ctx* ctx, Cloud& c, int n);  // room for n points (the contents are undefined after a resize)
int ensure_assoc(icpk_ctx* ctx, int nq);
// K1d's index of n points into g (reserved by the caller), everything enqueued: bounds, geometry, cell slots, scan,
// scatter.  The counting sort's cell and slot of every point go through the context's sort scratch, which nothing reads
// after the build that wrote it; the count table is left as it was found
int index_cloud(icpk_ctx* ctx, const float* x, const float* y, const float* z, int n, GridIndex& g);
// the target's index in ctx->grid: built unless have_grid, and then valid until the target changes
int index_target(icpk_ctx* ctx, GridView* out);
// the index of any other cloud the context holds, in ctx->aux_grid: valid until the next index_aux call, so *out is
// used up inside the call that asked for it.  Neither have_grid nor the target's index is touched
int index_aux(icpk_ctx* ctx, const Cloud& c, GridView* out);
// the working source planes hold the cloud icpk_get_source would return (a device loop may leave them to be unpacked)
int ensure_unpacked(icpk_ctx* ctx);
// where the grid set-up reads the query coordinates: the committed source while the working copy is deferred
inline const icpk::Cloud& query_cloud(const icpk_ctx* ctx) { return ctx->src_deferred ? ctx->src0 : ctx->src; }
int flush_loop_init(icpk_ctx* ctx);
NnArgs base_nn_args(const icpk_ctx* ctx);
int prepare_sorted_sweep(icpk_ctx* ctx, int nn_mode, NnArgs& a, NnBoxes& bx, int& recheck);
GridSweepArgs grid_sweep_args(icpk_ctx* ctx, const NnArgs& a, const NnBoxes& bx);
void after_grid_sweep(icpk_ctx* ctx);
int enqueue_nn(icpk_ctx* ctx, int nn_mode, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);
const float4* loop_rec(const icpk_ctx* ctx);
int enqueue_reduce(icpk_ctx* ctx, float max_dist);
int enqueue_reduce_p2l(icpk_ctx* ctx, float max_dist);
// plane-to-plane flavour of enqueue_reduce (K14).  R_acc: the rotation accumulated so far (9 floats); inside a device
// loop the kernel reads it from the loop state and this may be null
int enqueue_reduce_gicp(icpk_ctx* ctx, float max_dist, const float* R_acc);
// the joint step of colored ICP in place of enqueue_reduce_p2l (K17), with the context's lambda_geometric
int enqueue_reduce_colored(icpk_ctx* ctx, float max_dist);
// icpk_set_colored is on and this alignment is the flavour it applies to
inline bool colored_step(const icpk_ctx* ctx, const icpk_params* p) {
  return ctx->colored_on && p->solve == ICPK_SOLVE_POINT_TO_PLANE;
}
// robust sweep (K10): room for the selection of nq queries, its histogram cleared (once per alignment / hook call) ...
int ensure_robust(icpk_ctx* ctx, int nq);
// ... and the selection + the weighted K2 / K5 over the current associations (NSUM_W / NP2L_W sums; outside a device
// loop the sums, the count and the selection state are read back into red_host / rsel_host, not waited for)
int enqueue_reduce_robust(icpk_ctx* ctx, float max_dist, bool p2l);

// ---- icpk_align.cpp: the device-side loop, shared by the single-pair and the frame-batch path ----
int loop_nsum(const icpk_params* p);
int device_loop_begin(icpk_ctx* ctx, const icpk_params* p, bool throttled = false, bool mirror = false,
                      bool defer = false);
void device_loop_disarm(icpk_ctx* ctx);
int device_loop_finish(icpk_ctx* ctx, const icpk_params* p, float T_out[16], icpk_stats* stats,
                       const LoopState* h = nullptr);

// ---- icpk_fast.cpp: a key-point list into a cloud (K8's icpk_detected_to_cloud, K32's icpk_described_to_cloud) ----
// n key points kp (device, x and y floats) back-projected from the host depth image, posed and made cloud `which`, as
// icpk_detected_to_cloud documents; map (device, n ints, or null): every key point's index in the cloud, -1 if dropped
int keypoints_to_cloud(icpk_ctx* ctx, const float* kp, int n, const uint16_t* depth, int32_t d_rows, int32_t d_cols, float fx,
                       float cx, const float R[9], const float t[3], int32_t which, int* map, int32_t* n_out);
// the image and the list the last icpk_detect_fast left on the device (n < 0: none); the pointers are views
struct FastResident {
  const uint8_t* img;
  int rows, cols, channels;
  const float* kp;
  int n;
};
FastResident fast_resident(const icpk_ctx* ctx);

// ---- icpk_tsdf.cpp: the last ray cast as K25 reads it ----
// the eight planes where they lie, their shape, and the camera and pose icpk_tsdf_raycast was given
struct TsdfRayView {
  const float* maps;
  int rows, cols;
  float fx, cx;
  double pose[16];
};
// ICPK_E_NOT_SET (with the reason in ctx->err) without a volume or without a ray cast
int tsdf_raycast_view(icpk_ctx* ctx, TsdfRayView* out);
// K26, after tsdf_raycast_view has succeeded: whether the volume keeps intensities, and the three gradient planes of
// icpk_tsdf_raycast_color_gradients for the current ray cast (nullptr without them)
void tsdf_raycast_color_view(icpk_ctx* ctx, bool* color, const float** grad);
// K29: the volume itself as the SDF tracking calls read it -- the two planes where they lie and the parameters with the
// CURRENT origin (K23).  ICPK_E_NOT_SET (with the reason in ctx->err) without a volume
struct TsdfVolumeView {
  const float* tsdf;
  const uint16_t* weight;
  icpk_tsdf_params p;
};
int tsdf_volume_view(icpk_ctx* ctx, TsdfVolumeView* out);
// K30: what icpk_tsdf_apply (icpk_tsdf_apply.cpp) keeps with the volume -- the device stack of a call's frames, reused
// while the shape fits, and the per-chunk, per-op counts with their totals -- and the volume as that call writes it
struct TsdfApplyBufs {
  DevBuf<uint16_t> depth;    // n_frames x rows x cols
  DevBuf<float> intensity;   // the same, on a colour volume
  DevBuf<int> slots;         // TSDF_MAX_BLOCKS x TSDF_MAX_OPS
  DevBuf<long long> totals;  // TSDF_MAX_OPS
  PinnedBuf<long long> totals_host;
};
struct TsdfApplyView {
  float* tsdf;
  uint16_t* weight;
  float* intensity;  // null without ICPK_TSDF_COLOR
  long long n;
  icpk_tsdf_params p;  // with the CURRENT origin
  TsdfApplyBufs* bufs;
};
int tsdf_apply_view(icpk_ctx* ctx, TsdfApplyView* out);
// the refusals of icpk_tsdf_create and of icpk_tsdf_integrate's camera (nullptr: fine; else what is wrong), its range
// test of the intensities, and the frame the per-voxel rule reads
const char* tsdf_check_volume(const icpk_tsdf_params& p);
const char* tsdf_check_camera(int32_t rows, int32_t cols, float fx, float cx);
bool tsdf_intensities_ok(const float* v, size_t n);
TsdfFrame tsdf_make_frame(const icpk_tsdf_params& p, const float R[9], const float t[3], int rows, int cols, float fx, float cx);

// ---- icpk_frame_view.cpp: the view the projective calls read (K28) ----
// With ICPK_VIEW_RAYCAST exactly tsdf_raycast_view / tsdf_raycast_color_view.  With ICPK_VIEW_FRAME the selected level
// of the frame view in the same terms -- its eight planes, shape, fx / 2^l, cx / 2^l and pose; ICPK_E_NOT_SET without a
// snapshot or for a level it lacks --, whether the snapshot carries intensities, and that level's gradient planes
int projective_view(icpk_ctx* ctx, TsdfRayView* out);
void projective_color_view(icpk_ctx* ctx, bool* color, const float** grad);

// ---- icpk_batch.cpp: the lock-step machinery icpk_frames_batch.cpp shares ----
bool batch_eligible(const icpk_ctx* ctx, const icpk_params* p);  // params the lock-step path runs
int ensure_slots(icpk_ctx* ctx, int n);                           // n frame-batch slots (child contexts)
// throttled: the slot's loop publishes its progress (device_loop_begin), for enqueue_group_loop's throttled mode
int slot_setup_phase2(icpk_ctx* sl, const icpk_params* p, GridSweepArgs& first, bool throttled);
// throttled: the group's iterations are enqueued a few ahead of the slowest pair and stop once all have exited
int enqueue_group_loop(icpk_ctx* ctx, const icpk_params* p, const std::vector<icpk_ctx*>& act,
                       const std::vector<GridSweepArgs>& first, int set, const std::vector<bool>& own_event,
                       bool throttled);

}  // namespace icpk
