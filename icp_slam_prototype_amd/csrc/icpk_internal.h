// icpk_internal.h -- shared between the host side (icpk_api.cpp) and the HIP
// kernels.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "esdf_rule.h"
#include "tsdf_rule.h"

namespace icpk {

// ---- K1 geometry ----------------------------------------------------------
// One query per lane, 256 lanes (4 wave64) per workgroup; the target cloud is
// streamed through LDS in tiles of NN_TILE points (3 planes x 4 KiB).  Target
// planes are padded to a multiple of NN_TILE with +inf (never selected).
constexpr int NN_THREADS = 256;
constexpr int NN_TILE = 1024;
static_assert(NN_TILE == 4 * NN_THREADS, "one float4 per lane per plane per tile");

// (distance bits << 32) | index: for non-negative floats the bit pattern is
// monotone, so an unsigned 64-bit min is the lexicographic (distance, index)
// min -- independent of the order target chunks are merged in.
typedef unsigned long long nn_key_t;
constexpr nn_key_t NN_KEY_INIT = ~0ull;

struct NnArgs {
  const float* qx;
  const float* qy;
  const float* qz;
  int nq;
  const float* tx;
  const float* ty;
  const float* tz;
  int nt_pad;           // multiple of NN_TILE
  int tiles_per_chunk;  // target tiles handled by one workgroup
  nn_key_t* best;       // [nq], pre-set to NN_KEY_INIT
  const int* stop;      // device-loop stop flags (LoopState), or nullptr
};

struct Rt {
  float R[9];
  float t[3];
};
// one row of K3's p' = fl32(fl32(R p) + t) (kernels_transform.hip; K15 moves its points with the same operations):
// products of two floats are exact in double; two double roundings, then one to float
__device__ __forceinline__ float rot_row(float r0, float r1, float r2, float x, float y, float z) {
  return (float)__builtin_fma((double)r2, (double)z, __builtin_fma((double)r1, (double)y, (double)r0 * (double)x));
}
struct LoopState;  // device-side loop state, defined below
struct RobustSel;         // robust selection state (kernels_robust.hip), defined below
struct RobustTraceEntry;  // ... and its per-iteration record

constexpr int NSUM = 19;
constexpr int NSUM_REF = 13;  // sums [0..12]: all the reference flavour's loop step reads
constexpr int NP2L = 28;      // point-to-plane: 21 + 6 + 1
constexpr int NSUM_W = 21;   // robust Kabsch (ICPK_NSUM_W): NSUM weighted, [19] W, [20] kept
constexpr int NP2L_W = 30;   // robust point-to-plane (ICPK_NP2L_W): NP2L weighted, [28] W, [29] kept
constexpr int NSUM_MAX = 30;
constexpr int RED_THREADS = 256;
constexpr int RED_MAX_BLOCKS = 256;

inline int red_blocks(int n) {
  int b = (n + RED_THREADS - 1) / RED_THREADS;
  if (b < 1) b = 1;
  if (b > RED_MAX_BLOCKS) b = RED_MAX_BLOCKS;
  return b;
}

// kernels_nn.hip
void launch_fill_u64(nn_key_t* p, int n, nn_key_t v, const int* stop, hipStream_t s);
void launch_nn_exact(const NnArgs& a, hipStream_t s);
// bounding boxes for the pruned scan: 6 planes (lo x,y,z, hi x,y,z) per 1024-target
// tile (tbox) and per 128-target sub-tile (sbox)
constexpr int NN_SUB = 128;
constexpr int NN_SUBS = NN_TILE / NN_SUB;  // 8 sub-tiles per tile
struct NnBoxes {
  float* tbox;
  int tbox_stride;  // floats per plane
  float* sbox;
  int sbox_stride;
  // pruned scan only: NnArgs::tx/ty/tz are the Morton-ordered planes the boxes were
  // built on; ox/oy/oz the target in the caller's order (seed look-up); tperm maps a
  // scanned position to the original index; qperm lists the queries in Morton order
  const float* ox;
  const float* oy;
  const float* oz;
  const int* tperm;
  const int* qperm;
};

// kernels_sort.hip
void launch_bounds(const float* tbox, int tbox_stride, int ntiles, float* bounds, hipStream_t s);
struct GridInfo;
void launch_morton_order(const float* x, const float* y, const float* z, int n, const float* bounds, int bits,
                         unsigned* keys, int* slot, int* count, int* start, int* bsum, GridInfo* table,
                         unsigned* keys_out, int* perm_out, hipStream_t s);
void launch_gather_planes(const float* x, const float* y, const float* z, const int* perm, int n, int n_pad, float pad,
                          float* ox, float* oy, float* oz, int* perm_pad, hipStream_t s);
void launch_nn_filtered(const NnArgs& a, const nn_key_t* seed, int seed_scale, int q_per_lane, hipStream_t s);
// kernels_nn_pruned.hip
// st != nullptr (device-side loop): K3 is fused into the sweep (see the kernel)
void launch_nn_pruned(const NnArgs& a, const nn_key_t* seed_m, nn_key_t* best_m, const NnBoxes& b, int slices,
                      int recheck, const LoopState* st, hipStream_t s);
void launch_seed_morton(const unsigned* qkeys, const int* qperm, int nq, const float* qx, const float* qy,
                        const float* qz, const unsigned* tkeys, const float* sx, const float* sy, const float* sz,
                        const int* tperm, int nt, nn_key_t* seed_m, hipStream_t s);
void launch_seed_gather(const nn_key_t* best, const int* qperm, int nq, nn_key_t* seed_m, hipStream_t s);
void launch_tile_boxes(const float* x, const float* y, const float* z, int n, int ntiles, const NnBoxes& b,
                       hipStream_t s);
void launch_decimate(const float* x, const float* y, const float* z, int n, int stride, float* ox, float* oy, float* oz,
                     int n_out_pad, hipStream_t s);
// kernels_grid.hip: uniform grid over the target (ICPK_NN_GRID)
#ifndef ICPK_GRID_MAX_CELLS_LOG2
#define ICPK_GRID_MAX_CELLS_LOG2 23  // 3 tables of 32 MB per context; 22 clipped the cell edge of the dense clouds
#endif
constexpr int GRID_MAX_CELLS = 1 << ICPK_GRID_MAX_CELLS_LOG2;
// the slots of the frame-batch mode (up to 32 child contexts) own smaller tables: Kinect-size pairs need ~0.9 M cells,
// and 3 x 8 MB per slot instead of 3 x 32 MB keeps a 64-pair batch at 0.8 GB instead of 3.2 GB (a denser pair in a slot
// merely gets a coarser grid: efficiency only -- tests/test_gpu_lockstep_edges.py holds a slot whose target asks for
// more than 4 x 2^21 cells to the exact kernel)
constexpr int GRID_MAX_CELLS_SLOT = 1 << 21;
constexpr int GRID_BOUNDS_PARTS = 256;  // partial boxes of the bounds pass (6 floats each)
struct GridInfo {
  float lo[3];  // finite lower corner of the target
  float inv_h;  // 1 / cell edge (y and z)
  float h;
  float inv_hx;  // 1 / cell edge along x = xdiv / h
  int xdiv;
  int nx, ny, nz;
  int ncells;
  int nxq;       // cells along x of the coarser grid that orders the queries (nx / xdiv)
  int ncells_q;
};
// K1d's index of a cloud as a kernel that walks it takes it (K12, K13, K14, K15, K16, K17; GridIndex::view, icpk_ctx.h)
struct GridView {
  const float4* t4;       // the cloud sorted by cell (x, y, z, original index)
  const int* cell_start;  // ncells + 1 entries
  const GridInfo* gi;
};
constexpr int GRID_SCAN_BLOCKS = (GRID_MAX_CELLS + 1 + 2047) / 2048 + 1;  // scratch ints of launch_grid_scan
// (the index's set-up steps -- bounds, info, cell slots, scan, scatters -- take their argument structs: see the deferred
// set-up launches below)
// one pair's arguments of a grid sweep (K1d); see nn_grid_body
struct GridSweepArgs {
  float *qx, *qy, *qz;  // the caller's source planes (kept in step when K3 is fused)
  int nq;
  int pad0;
  float4* qm4;            // queries in scan order (x, y, z, original index)
  const float4* t4;       // targets sorted by cell (x, y, z, original index)
  const int* cell_start;
  const GridInfo* gi;
  const float *ox, *oy, *oz;  // target in the caller's order (literal seed, element 0)
  const float4* sp_in;    // seeds as points, scan order
  float4* sp_out;         // matches as points = the next sweep's seeds
  nn_key_t* best;         // results, caller's order
  nn_key_t* best_m;       // results, scan order
  const LoopState* st;    // device-side loop state (K3 fused) or nullptr
  float4* rec;            // device loop: caller-order records {(query, distance), (match, index)} INSTEAD of the planes / best / best_m stores; else nullptr
};
// frame-batch mode: up to BATCH_MAX independent pairs advance in lock step, one launch per
// stage for the whole group (blockIdx.y / blockIdx.x = pair); arguments travel by value.
constexpr int BATCH_MAX = 16;
struct GridSweepBatch {
  GridSweepArgs p[BATCH_MAX];
};
void launch_nn_grid(const GridSweepArgs& a, int slices, int expand, hipStream_t s);
void launch_nn_grid_batch(const GridSweepBatch& b, int count, int slices, int expand, hipStream_t s);
void launch_grid_unpack(const float4* qm4, const float4* rec, int nq, float* qx, float* qy, float* qz, nn_key_t* best,
                        hipStream_t s);
void launch_grid_query_points(const float* qx, const float* qy, const float* qz, const int* qperm, int nq,
                              const nn_key_t* seed_m, const float* ox, const float* oy, const float* oz, float4* qm4,
                              float4* sp, hipStream_t s);
constexpr int NN_SEED_STRIDE = 16;  // decimation of the target for the seeding pre-pass
void launch_pair_distance(const float* a, const float* b, float* out, int n, int point3, hipStream_t s);

// ---- device-side ICP loop (kernels_loop.hip) ------------------------------------
// One LoopState per context lives in device memory; while an alignment runs, every
// kernel of every iteration is enqueued up front and consults it: once `done` (or
// `stop_after_transform`) is set the remaining launches are no-ops, so no host
// round trip is needed to decide the loop exit of icp.cpp:155.
constexpr int LOOP_MAX_ITER = 256;
struct LoopState {
  int done;                  // loop exited (threshold met / max iterations / degenerate)
  int stop_after_transform;  // < min_pairs fallback (icp.cpp:163-182): apply rt, then stop
  int iterations;            // completed loop bodies
  int status;
  int sweeps;                // NN sweeps executed (tells the host which buffer holds the result)
  int steps;                 // loop steps executed (mirrored to *progress)
  long long pairs;           // associations of the latest sweep
  float mse;                 // icp.cpp:622-638 of the latest sweep
  int epoch;                 // tag of this alignment in the progress words (see below)
  // host-visible (pinned, mapped) progress words or nullptr: [0] = loop steps executed, [1] = loop has
  // exited, written only while `throttled`.  With a loop that may exit early (threshold mode) the host enqueues only a couple of
  // iterations ahead of them instead of all max_iterations: every launch after the exit is a no-op that
  // still costs its dispatch (~3 us each: 100 us for the reference's 16 / 1e-4 setting leaving after 5).
  // Both words carry `epoch` ([0] = epoch << 10 | steps, [1] = epoch << 2 | done << 1 | exited), so that words still
  // being written by an alignment that was abandoned on an error are never taken for this one's.
  int* progress;
  // host-visible (pinned, mapped) copy of the OUTPUT fields of this struct or nullptr: the step that ends the loop
  // writes them there and then sets progress[2] = epoch << 1 | 1 with a system-scope release, so the host has the
  // result the moment the loop ends -- no copy kernel, no stream wait (the trace of the completed iterations goes
  // there with them, copied from this state: an iteration stores nothing in host memory)
  LoopState* mirror;
  Rt rt;                     // transform to apply in this iteration
  double Rd[9];              // rt.R widened (exact) by the step: the sweeps' fused K3 takes the rotation as float64 scalars
  float Trot[9];             // icp.cpp:227-233
  float offset[3];           // icp.cpp:240
  double Tk[12];             // accumulated [R|t] (Kabsch / point-to-plane)
  // parameters
  int max_iterations, min_pairs, solve, fixed_iterations;
  float threshold;
  int throttled;             // the host enqueues this loop a few iterations ahead and watches progress[0], [1]
  float last_rotation[9], last_translation[3];
  // per-iteration record (icpk_get_trace)
  float trace_R[LOOP_MAX_ITER * 9];
  float trace_t[LOOP_MAX_ITER * 3];
  float trace_mse[LOOP_MAX_ITER];
  int trace_pairs[LOOP_MAX_ITER];
};
// the first two ints of LoopState, as seen by kernels that only need to know whether to run
__device__ __forceinline__ bool loop_stopped(const int* stop) { return stop && (stop[0] | stop[1]); }

// sums the per-block partials with the canonical tree and, unless stats_only, performs
// one loop body's host work on the device: exit test, solve, pose accumulation, trace
struct StepArgs {
  const double* partial;
  const int* pcount;
  int nblocks;
  int pad0;
  LoopState* st;
};
struct StepBatch {
  StepArgs p[BATCH_MAX];
};
// nsum NSUM_W / NP2L_W: the robust step (kept count for min_pairs, W for the solve, one RobustTraceEntry per
// completed iteration into rtrace, the cut and scale read from sel)
void launch_loop_step(const double* partial, const int* pcount, int nblocks, int nsum, LoopState* st, int stats_only,
                      hipStream_t s, const RobustSel* sel = nullptr, RobustTraceEntry* rtrace = nullptr);
void launch_loop_step_batch(const StepBatch& b, int count, int nsum, int stats_only, hipStream_t s);
void launch_transform_state(float* x, float* y, float* z, int n, const LoopState* st, hipStream_t s);
void launch_reduce_final(const double* partial, const int* pcount, int nblocks, int nsum, double* out, hipStream_t s);
// query-sharded loop: NSUM sums + the count as a double into out[0 .. NSUM]; launch_loop_step with nblocks = -1 then
// takes the (all-reduced) sums from there
void launch_reduce_final_shard(const double* partial, const int* pcount, int nblocks, double* out, const LoopState* st,
                               hipStream_t s);

// kernels_reduce.hip
// What every reduction over one sweep's pairs takes (K2, K5, K14, K17; the device side is pair_reduce.h).
struct PairArgs {
  const nn_key_t* best;        // the sweep's (distance bits, index) keys, caller's order
  const float *ax, *ay, *az;   // the moved source
  const float *tx, *ty, *tz;   // the target
  const float4* o4;            // the target as caller-order (x, y, z, 0) points or nullptr (then tx / ty / tz are gathered)
  const float4* rec;           // != nullptr (device loop behind a grid sweep): everything comes from the sweep's caller-order records instead
  int nq;
  float max_dist;
  int32_t* idx_out;            // the keys unpacked, or nullptr (both)
  float* dist_out;
  double* partial;             // [NSUM_MAX][RED_MAX_BLOCKS] doubles (sum-major: stage 2 reads it coalesced)
  int* pcount;                 // [RED_MAX_BLOCKS] ints
  double* out;                 // nsum doubles followed by one int64 count ((NSUM_MAX + 1) x 8 bytes); nullptr: only the
                               // per-block partials are produced (the device loop sums them in launch_loop_step)
  LoopState* st;               // the device loop's state or nullptr
};
// nact: NSUM, or NSUM_REF inside a device loop of the reference flavour; sel: the weighted K2 (NSUM_W sums)
void launch_assoc_reduce(const PairArgs& a, int nact, hipStream_t s, const RobustSel* sel = nullptr);
// one pair's arguments of K2 inside a device loop (no idx/dist unpacking, no final stage)
struct ReduceArgs {
  const nn_key_t* best;
  const float *ax, *ay, *az;
  const float *tx, *ty, *tz;
  const float4* o4;  // or nullptr
  const float4* rec;  // the sweep's caller-order records
  double* partial;
  int* pcount;
  LoopState* st;
  int nq;
  int nblocks;  // red_blocks(nq): the canonical geometry of THIS pair
};
struct ReduceBatch {
  ReduceArgs p[BATCH_MAX];
};
void launch_assoc_reduce_batch(const ReduceBatch& b, int count, float max_dist, int nact, hipStream_t s);

// K5: nx / ny / nz the target's normals; sel: the weighted K5 (NP2L_W sums)
void launch_p2l_reduce(const PairArgs& a, const float* nx, const float* ny, const float* nz, hipStream_t s,
                       const RobustSel* sel = nullptr);

// kernels_gicp.hip -- K14, the plane-to-plane (generalized ICP) step (ICPK_SOLVE_PLANE_TO_PLANE; the rule is spelled
// out in include/icpk.h).  NP2L sums in the layout solve_p2l reads.
struct GicpArgs {
  const float *snx, *sny, *snz;  // source normals, caller's order (same indexing as the working source)
  const float *tnx, *tny, *tnz;  // target normals
  float R[9];                    // R_acc when st == nullptr (a device loop reads LoopState::Tk instead)
  float epsilon;
};
void launch_gicp_reduce(const PairArgs& a, const GicpArgs& g, hipStream_t s);

// kernels_color.hip -- K17, colored ICP (icpk_estimate_target_color_gradients, icpk_set_colored; the rule is spelled
// out in include/icpk.h)
constexpr int COLOR_SUMS = 10;  // per point: m, S_00 S_01 S_02 S_11 S_12 S_22, T_0 T_1 T_2 (int64 each)
struct ColorGradArgs {
  GridView index;             // K1d's index of the target
  const float *nx, *ny, *nz;  // target normals, caller's order
  const float* col;           // target intensities, caller's order
  float* col_sorted;          // [n] scratch: the intensities in cell order
  int n;
  float radius;
  int min_neighbors;
  long long* sums;      // [n][COLOR_SUMS], caller's order
  float *gx, *gy, *gz;  // [n]
};
static_assert(sizeof(ColorGradArgs) == 112 && offsetof(ColorGradArgs, index) == 0, "the kernarg layout is pinned");
// the three launches of one estimate (gather, sums, solve); n <= 0: nothing
void launch_color_gradients(const ColorGradArgs& a, hipStream_t s);
struct ColoredArgs {
  const float *tnx, *tny, *tnz;  // target normals
  const float *gx, *gy, *gz;     // target colour gradients
  const float* tcol;             // target intensities
  const float* scol;             // source intensities, caller's order (same indexing as the working source)
  float lambda_geometric;
};
// NP2L sums in the layout solve_p2l reads
void launch_colored_reduce(const PairArgs& a, const ColoredArgs& g, hipStream_t s);

// ---- robust alignment (K10: kernels_robust.hip, the weighted K2 / K5 of kernels_reduce.hip) ----------------------
// The exact cut tau and median m of one sweep's accepted distances by a radix select over their bit patterns
// (non-negative floats sort as unsigned integers; the sign bit is cleared, so -0 counts as +0): three passes of
// 11 / 10 / 10 bits (bits 30..20, 19..10, 9..0), each a histogram kernel (LDS integer atomics per block, then the
// block's non-zero bins added into one global histogram with integer atomics -- exact, so deterministic) and a
// one-block scan that narrows both ranks' buckets and clears the histogram for the next pass.
constexpr int SEL_BINS = 2048;  // bins of the widest pass; the global histogram holds 2 x SEL_BINS ints (tau, m)
struct RobustCfg {  // icpk_robust as the kernels take it
  int kernel, scale_mode;
  float scale, trim;
};
struct RobustSel {
  unsigned prefix[2];  // high bits of tau ([0]) and m ([1]) found so far; after the last pass their full patterns
  long long rank[2];   // 1-based ranks still to be found inside those buckets
  long long n;         // accepted pairs of the sweep
  int same;            // prefix[0] == prefix[1]: one histogram serves both ranks
  int kernel;          // ICPK_ROBUST_* for the weighted reduction
  float cut, median;   // tau and m (0 when n == 0)
  double c;            // the scale of the weights
};
struct RobustTraceEntry {  // icpk_get_robust_trace, one per completed iteration
  int kept;
  float cut;
  double c, wsum;
};
// dsel: [nq] scratch (the sweep's accepted distance patterns, 0xffffffff for the others); hist: 2 x SEL_BINS ints, zero
// between selections; nx != nullptr: point-to-plane acceptance (non-zero target normal as well)
void launch_robust_select(const nn_key_t* best, const float4* rec, int nq, float max_dist, const float* nx,
                          const float* ny, const float* nz, unsigned* dsel, int* hist, RobustSel* sel, const RobustCfg& cfg,
                          const LoopState* st, hipStream_t s);

// w(d) of a kept candidate (accepted: d < max_dist): 0 beyond the cut, else the kernel's weight in float64
struct RobustWeight {
  int kernel;
  float cut;
  double c;
  __device__ __forceinline__ double operator()(float d) const {
    if (!(d <= cut)) return 0.0;
    const double x = d;
    if (kernel == 1) return x <= c ? 1.0 : c / x;  // ICPK_ROBUST_HUBER
    if (kernel == 2) {                             // ICPK_ROBUST_TUKEY
      if (x == 0.0) return 1.0;
      if (!(x < c)) return 0.0;
      const double r = x / c, u = 1.0 - r * r;
      return u * u;
    }
    return 1.0;  // ICPK_ROBUST_NONE
  }
};

// kernels_transform.hip
void launch_transform(float* x, float* y, float* z, int n, const Rt& rt, hipStream_t s);
void launch_fill_f32(float* p, int n, float v, hipStream_t s);

// kernels_backproject.hip
// counts: [ceil(npix/1024)+1] ints scratch.  Returns nothing; *n_out (device)
// receives the number of points.
// nx == nullptr: no normals
void launch_backproject(const uint16_t* depth, int rows, int cols, float fx, float cx, float ox, float oy, float oz,
                        float* x, float* y, float* z, float* nx, float* ny, float* nz, int normals_mode,
                        int* block_counts, int* n_out, unsigned long long sub_key, int sub_factor, hipStream_t s);
// icpk_backproject_pair: image 0 = current frame (source; x2/y2/z2 = its working copy), image 1 = previous
// frame (target).  counts: nblocks + 2 ints per image.
struct BpImage {
  const uint16_t* depth;
  float *x, *y, *z;
  float *x2, *y2, *z2;
  int* counts;
  float pad;
  // image-space seeds of the alignment that follows (see QscatterArgs::spix) or nullptr: the pixel of every point
  // (per point) / the point of every pixel, -1 where the pixel is empty (per pixel)
  int* pixel_of_point;
  int* point_of_pixel;
  // zero-copy upload or nullptr: the image still sits in pinned host memory; the counting pass reads it from there
  // (one PCIe read per pixel, no copy-engine command in front of the kernels) and leaves the device copy in raw_out,
  // which `depth` points to for the scatter pass
  const uint16_t* host_src;
  uint16_t* raw_out;
  unsigned long long sub_key;  // seeded subsample of this image (kernels_backproject.hip: bp_keep); factor <= 1: none
  int sub_factor, pad1;
};
struct BpPair {
  BpImage im[2];
};
void launch_backproject_pair(const BpPair& b, int rows, int cols, float fx, float cx, float ox, float oy, float oz,
                             const Rt& rt, int posed, int* n_out, int* n_host, hipStream_t s);
// icpk_align_frames_batch: the frame pairs of a lock-step group (one per job, at most BATCH_MAX), both images of each
// in ONE launch per pass (blockIdx.y = 2 x pair + image).  Image 0 (source) goes to the slot's src0 and src planes
// and records pixel_of_point in pix_src; image 1 (target) goes to tgt and records point_of_pixel in pix_tidx.  The
// per-image fields are those of BpImage; counts: image 0 at counts, image 1 at counts + per_image.
struct BpFramePair {
  const uint16_t* depth[2];
  const uint16_t* host_src[2];
  uint16_t* raw_out[2];
  float *src0, *src, *tgt;  // plane bases (x; y at + cap; z at + 2 cap)
  int src0_cap, src_cap, tgt_cap, sub_factor;
  int* counts;
  int *pix_src, *pix_tidx;
  unsigned long long sub_key[2];
  Rt rt;  // the pose of both clouds (always applied)
};
struct BpFrameBatch {
  BpFramePair p[BATCH_MAX];
};
// n_out: 2 x count ints (device), n_host: 2 x count mapped words (image 2 k + i's total at [2 k + i])
void launch_backproject_frames(const BpFrameBatch& b, int count, int rows, int cols, float fx, float cx, float ox,
                               float oy, float oz, int* n_out, int* n_host, hipStream_t s);

// kernels_frontend.hip
// order-preserving split of a sweep's result into accepted pairs and rejected queries
// (icp.cpp:488-515); block_counts: ceil(nq/1024) + 1 ints of scratch, *n_accepted (device) = count
void launch_assoc_split(const nn_key_t* best, int nq, float max_dist, int* block_counts, int* n_accepted,
                        int32_t* assoc_q, int32_t* assoc_t, float* assoc_d, int32_t* rej_q, hipStream_t s);
// SLAM.cpp:553-574: range clamp, then (morph != 0) 5x5 dilate + erode with anchor (ax, ay)
void launch_depth_filter(const uint16_t* in, uint16_t* out, int rows, int cols, int min_d, int max_d, int ax, int ay,
                         int morph, hipStream_t s);
// the same filter over `count` images of one size in ONE launch (blockIdx.z = image)
struct DfBatch {
  const uint16_t* in[2 * BATCH_MAX];
  uint16_t* out[2 * BATCH_MAX];
};
void launch_depth_filter_batch(const DfBatch& b, int count, int rows, int cols, int min_d, int max_d, int ax, int ay,
                               int morph, hipStream_t s);
// K22, THE BILATERAL RULE: tables = (2 radius + 1)^2 spatial weights, then K range weights (device; in != out)
void launch_depth_bilateral(const uint16_t* in, uint16_t* out, int rows, int cols, int radius, int K,
                            const uint16_t* tables, hipStream_t s);
// K24, THE PYRAMID RULE: level l (rows x cols) gives level l + 1 into out1 and, unless out2 is null, level l + 2 into
// out2, in one launch (device; three different images)
void launch_depth_pyramid(const uint16_t* in, int rows, int cols, uint16_t* out1, uint16_t* out2, int K, hipStream_t s);
// kernels_pyramid_color.hip -- K26: level l + 1 of the intensity pyramid from level l of both pyramids
void launch_intensity_pyramid(const uint16_t* depth, const float* inten, int rows, int cols, float* out, int K,
                              hipStream_t s);
// kernels_raycast_color.hip -- K26: the colour gradients of a ray-cast view (8 planes of rows x cols floats) into three
// planes of grad, and the ten int64 per pixel into sums unless it is nullptr
void launch_raycast_color_gradients(const float* maps, int rows, int cols, float radius, int min_neighbors, float* grad,
                                    long long* sums, hipStream_t s);
// kernels_fern.hip -- K27, THE FERN RULE.  A code on the device is F / 8 words followed by one word that holds V.
constexpr int FERN_MAX_F = 1024;           // ferns: the encode workgroup's size
constexpr int FERN_TOPK = 8;               // ICPK_FERN_MAX_K: keys a workgroup of the search leaves
constexpr int FERN_SEARCH_THREADS = 256;   // keyframes per workgroup of the search; 65536 / 256 lists fit the merge
// level: the level the table (F x FERN_ENTRY int32, device) was drawn for; code: F / 8 + 1 words
void launch_fern_encode(const uint16_t* level, int cols, const int32_t* table, int F, uint32_t* code, hipStream_t s);
// the min(FERN_TOPK, n) smallest keys diss << 16 | index of the n keyframes against `code`, ascending, then FERN_NO_KEY,
// into out[0 .. FERN_TOPK): two launches.  db: W x capacity words; lists: ceil(n / FERN_SEARCH_THREADS) x FERN_TOPK
// words of scratch.  n <= 0: nothing is launched
void launch_fern_search(const uint32_t* db, int capacity, int n, const uint32_t* code, int W, uint32_t* lists, uint32_t* out,
                        hipStream_t s);
void launch_fern_append(uint32_t* db, int capacity, int column, const uint32_t* code, int W, hipStream_t s);

// ---- deferred set-up launches of the frame-batch mode ------------------------------------------------
// A lock-step group's pairs go through the SAME sequence of small set-up kernels (ingest x 2, loop-state
// init, bounds, grid info, 2 x (cell slots, scan sums, scan), target scatter, query scatter): 13 launches per
// pair on its own stream, which for 8 pairs is 0.26 ms that nothing hides when the group is the only one
// (config 4 at 8 GPUs).  While a SetupRecorder is installed in the calling thread the launchers below
// RECORD their arguments instead of launching; flush_setup_batches() then issues ONE launch per step for
// all pairs (blockIdx.y / blockIdx.x = pair, arguments by value), or, should the pairs' sequences differ,
// replays them one by one.  Same kernels' bodies: same bits.
struct IngestArgs {
  const float *x, *y, *z;
  int n, n_pad;
  float pad;
  int cap1;
  float* d1;
  float* d2;
  int cap2;
  int pad0;
};
struct LoopInitArgs {
  LoopState* st;
  int* progress;
  LoopState* mirror;
  int max_iterations, min_pairs, solve, fixed_iterations;
  float threshold;
  int epoch;
  int throttled;  // LoopState::throttled
  float last_rotation[9], last_translation[3];
};
struct BoundsArgs {
  const float *x, *y, *z;
  float* fb;
  int n, nparts;
};
struct InfoArgs {
  const float* fb;
  GridInfo* g;
  int nparts, n;
  float ppc;
  int xdiv;
  int max_cells;  // capacity of this context's cell tables
  int pad0;
};
struct QslotArgs {
  const float *x, *y, *z;
  const GridInfo* gi;
  int *count, *cell, *slot;
  int n, coarse;
};
struct ScanArgs {
  int *count, *out, *bsum;
  const GridInfo* g;
  int coarse, pad0;
};
struct TscatterArgs {
  const float *x, *y, *z;
  const int *tcell, *tslot, *cell_start;
  float4 *t4, *o4;
  int n, pad0;
};
struct QscatterArgs {
  const int *qcell, *qslot, *qstart;
  int* qperm;
  const float *qx, *qy, *qz, *ox, *oy, *oz;
  float4 *qm4, *sp;
  nn_key_t* seed_m;
  int n, pad0;
  // Seeds from the images the two clouds were back-projected from (icpk_backproject_pair), or nullptr: spix[i] = pixel
  // of query i, tidx[p] = target point of pixel p or -1.  Consecutive frames of a depth camera put the same surface
  // within a pixel or two, so the target point of the query's own pixel (or of the nearest occupied pixel of the
  // 5 x 5 around it) is a seed centimetres from the true match -- instead of the reference's literal element 0, metres
  // away (icp.cpp:572).  A seed only sets where the search starts: the result is the exact nearest neighbour either way.
  const int* spix;
  const int* tidx;
  int rows, cols;
};
enum SetupKind : int { SK_INGEST, SK_LOOP_INIT, SK_BOUNDS, SK_INFO, SK_QSLOT, SK_SCAN, SK_TSCATTER, SK_QSCATTER };
struct SetupCall {
  int kind;
  union {
    IngestArgs ingest;
    LoopInitArgs loop_init;
    BoundsArgs bounds;
    InfoArgs info;
    QslotArgs qslot;
    ScanArgs scan;
    TscatterArgs tscatter;
    QscatterArgs qscatter;
  };
};
// a pair's set-up is 13 steps today (ingest x 2, loop init, bounds, info, 2 x (slots, scan), target scatter, query
// scatter + the upload path's extras); a recorder that overflows marks itself and the pair FAILS (align_batch_impl)
constexpr int SETUP_MAX_CALLS = 24;
struct SetupRecorder {
  SetupCall calls[SETUP_MAX_CALLS];
  int n = 0;
  bool overflow = false;
};
SetupRecorder*& setup_recorder();  // of the calling thread; nullptr: launch at once
// THE record point, shared by every step launcher below: with a recorder installed the step's arguments are kept
// instead of launched (true: the launcher has nothing left to do).  A launcher whose step has nothing to do (n <= 0)
// returns before it gets here: an empty step is never recorded, and that decides whether a group's sequences are equal
template <typename A>
bool record_setup_step(int kind, A SetupCall::*field, const A& a) {
  SetupRecorder* const r = setup_recorder();
  if (!r) return false;
  if (r->n < SETUP_MAX_CALLS) {
    r->calls[r->n].kind = kind;
    r->calls[r->n++].*field = a;
  } else {
    r->overflow = true;
  }
  return true;
}
template <typename A>
struct SetupBatchOf {
  A p[BATCH_MAX];
};
// the two steps whose arguments are normalised: every caller makes them here
inline int grid_bounds_parts(int n) {  // one 1024-thread block per 2048 points, at most GRID_BOUNDS_PARTS
  const int nb = (n + 2047) / 2048;
  return nb < 1 ? 1 : (nb > GRID_BOUNDS_PARTS ? GRID_BOUNDS_PARTS : nb);
}
inline BoundsArgs bounds_args(const float* x, const float* y, const float* z, int n, float* fb) {
  return BoundsArgs{x, y, z, fb, n, grid_bounds_parts(n)};
}
// (fb: the partial boxes a bounds step over the same n points leaves)
inline InfoArgs info_args(const float* fb, int n, float ppc, int xdiv, int max_cells, GridInfo* g) {
  return InfoArgs{fb, g, grid_bounds_parts(n), n, ppc, xdiv < 1 ? 1 : xdiv, max_cells < 64 ? 64 : max_cells, 0};
}
// Every step has ONE shape: its argument struct and a stream (recorded or launched, see above), and a _batch form that
// takes the structs of `count` pairs.  tscatter, qslot and qscatter do nothing for n <= 0, ingest for n_pad <= 0.
void launch_ingest_cloud(const IngestArgs& a, hipStream_t s);  // kernels_transform.hip
void launch_loop_init(const LoopInitArgs& a, hipStream_t s);   // kernels_loop.hip
void launch_grid_bounds(const BoundsArgs& a, hipStream_t s);
void launch_grid_info(const InfoArgs& a, hipStream_t s);
void launch_grid_qslot(const QslotArgs& a, hipStream_t s);
// the same step with the initial LoopState of the alignment being enqueued on the side (workgroup 0); never recorded:
// false, and nothing launched, while a recorder is installed or when the step has nothing to do
bool launch_grid_qslot_init(const QslotArgs& a, const LoopInitArgs& init, hipStream_t s);
void launch_grid_scan(const ScanArgs& a, hipStream_t s);  // count[] is left zero; bsum: GRID_SCAN_BLOCKS ints
void launch_grid_tscatter(const TscatterArgs& a, hipStream_t s);
// qm4 != nullptr: also the scan-order queries and every query's seed point and seed key
void launch_grid_qscatter(const QscatterArgs& a, hipStream_t s);
// bounds + info (+ the initial LoopState, init != nullptr) of a fresh pair in one launch; never recorded
void launch_grid_begin(const BoundsArgs& a, const InfoArgs& info, const LoopInitArgs* init, int* ticket, hipStream_t s);
// one launch per recorded step for `count` pairs, in recording order; returns false if the sequences differ
// (nothing launched then: replay them with replay_setup)
bool flush_setup_batches(const SetupRecorder* recs, int count, hipStream_t s);
void replay_setup(const SetupRecorder& rec, hipStream_t s);
void launch_ingest_batch(const SetupBatchOf<IngestArgs>& b, int count, hipStream_t s);
void launch_loop_init_batch(const SetupBatchOf<LoopInitArgs>& b, int count, hipStream_t s);
void launch_grid_bounds_batch(const SetupBatchOf<BoundsArgs>& b, int count, hipStream_t s);
void launch_grid_info_batch(const SetupBatchOf<InfoArgs>& b, int count, hipStream_t s);
void launch_grid_qslot_batch(const SetupBatchOf<QslotArgs>& b, int count, hipStream_t s);
void launch_grid_scan_batch(const SetupBatchOf<ScanArgs>& b, int count, hipStream_t s);
void launch_grid_tscatter_batch(const SetupBatchOf<TscatterArgs>& b, int count, hipStream_t s);
void launch_grid_qscatter_batch(const SetupBatchOf<QscatterArgs>& b, int count, hipStream_t s);
void launch_grid_tqscatter(const TscatterArgs& t, const QscatterArgs& q, hipStream_t s);

// kernels_fast.hip -- K8: FAST key points (SLAM.cpp:255-256) and their back-projection (pointcloud.cpp:60-98)
int fast_tiles_x(int cols);  // tile columns of a cols-wide image (64-pixel tiles)
// img: rows x cols x channels bytes on the device; pattern 12 or 16; masks / counts: rows x fast_tiles_x(cols) entries;
// score: rows x cols bytes; kp / resp: room for every candidate pixel; *total (device) = the number of key points
void launch_fast_detect(const uint8_t* img, int rows, int cols, int channels, int threshold, int nonmax, int pattern,
                        unsigned long long* masks, int* counts, uint8_t* score, int* total, float* kp, float* resp,
                        hipStream_t s);
void launch_bgr_to_gray(const uint8_t* bgr, int n, uint8_t* out, hipStream_t s);
// n key points (x, y) back-projected from depth and posed, into x / y / z (and x2 / y2 / z2 unless null) padded with
// `pad` up to the next multiple of NN_TILE; the count to *n_dev and the mapped word *n_host (or null)
void launch_fast_cloud(const float* kp, int n, const uint16_t* depth, int rows, int cols, float fx, float cx, const Rt& rt,
                       float* x, float* y, float* z, float* x2, float* y2, float* z2, float pad, int* n_dev, int* n_host,
                       int* map, hipStream_t s);

// kernels_map.hip -- the voxel certainty map (map.hpp, map.cpp)
constexpr int MAP_DIM = 300;                              // map.hpp:9 MAP_HEIGHT
constexpr int MAP_CELLS = MAP_DIM * MAP_DIM * MAP_DIM;    // keys < 2^25
constexpr int MAP_TILE = 1024;                            // items per workgroup of the sort / compaction kernels
constexpr int MAP_RADIX_BITS = 9;
constexpr int MAP_RADIX = 1 << MAP_RADIX_BITS;
constexpr int MAP_PASSES = 3;                             // 27 bits >= 25
static_assert((1 << (MAP_RADIX_BITS * MAP_PASSES)) >= MAP_CELLS, "radix passes must cover every voxel key");
struct MapPoints {  // batch element i = point idx[i] of the planes (idx == nullptr: point i)
  const float* x;
  const float* y;
  const float* z;
  const int* idx;
  int n;
};
struct MapBuffers {  // batch-sized scratch of an update (n entries each unless noted)
  int* key;          // voxel keys in input order
  int* ka;
  int* kb;
  int* va;
  int* vb;
  int* hist;         // MAP_RADIX x tiles
  int* flag;
  int* tcount;       // tiles + 1
  int* total;        // 1: entries appended by the update / rejected positions found
};
void launch_map_update(const MapPoints& p, int rule, int delta, int old_len, int list, float* lx, float* ly, float* lz,
                       uint8_t* cert, int* slot, const MapBuffers& b, hipStream_t s);
// out[i] = certainty, out[n + i] = slot of point i's voxel
void launch_map_query(const float* x, const float* y, const float* z, int n, const uint8_t* cert, const int* slot,
                      int* out, hipStream_t s);
// the rejected positions of nsw association sweeps of ns source points (motion[s]: the transform after sweep s) against
// nt map key points, compacted into ox / oy / oz in (sweep, query) order; *b.total = their number.  px / py / pz:
// ns x nsw scratch; b sized for ns x nsw entries.
void launch_map_rejected(const float* x, const float* y, const float* z, int ns, const Rt* motion, int nsw, float* px,
                         float* py, float* pz, const float* tx, const float* ty, const float* tz, int nt,
                         float max_dist, float* ox, float* oy, float* oz, const MapBuffers& b, hipStream_t s);

// kernels_map_nn.hip -- K9, the mapped nearest-neighbour lookup (icp.cpp:371-486)
constexpr int MAP_BRICKS = MAP_DIM / 4;  // occupancy mask: one bit per 4^3 brick
constexpr int MAP_MASK_WORDS = (MAP_BRICKS * MAP_BRICKS * MAP_BRICKS + 31) / 32;
struct MapNnArgs {
  const float* qx;
  const float* qy;
  const float* qz;
  int nq;
  const int* slot;
  const unsigned* mask;  // MAP_MASK_WORDS, current for `slot`
  int cells_exact;       // every filled slot names a point inside its voxel's cell (see icpk_map.cpp)
  const float *l0x, *l0y, *l0z;  // key-point list (n0 entries)
  int n0;
  const float *l1x, *l1y, *l1z;  // point list (n1 entries)
  int n1;
  nn_key_t* best;  // per query: (bits(d) << 32) | target index in [key points | points | zero point]
  const int* stop;  // device-loop stop flags, or nullptr
};
void launch_map_mask(const int* slot, unsigned* mask, hipStream_t s);
void launch_map_nn(const MapNnArgs& a, hipStream_t s);
// the positions of nsw sweeps of ns source points (as launch_map_rejected rebuilds them): sweep s at px + s * ns
void launch_map_poses(const float* x, const float* y, const float* z, int ns, const Rt* motion, int nsw, float* px,
                      float* py, float* pz, hipStream_t s);
// icpk_align_to_map_dense: the positions of the last sweep whose key says d < max_dist, compacted in query order into
// ox / oy / oz; *b.total = their number (b sized for n entries)
void launch_map_accepted(const float* px, const float* py, const float* pz, int n, const nn_key_t* best,
                         float max_dist, float* ox, float* oy, float* oz, const MapBuffers& b, hipStream_t s);

// kernels_voxel.hip -- K11, voxel-grid downsampling (icpk_voxel_downsample)
struct VoxelSlot {         // one entry of the open-addressing table: 64 bytes, one line
  unsigned long long key;  // the packed voxel + 1; 0: empty
  unsigned inv_first;      // 0x7fffffff - the lowest member index so far (atomicMax); 0: no member yet
  int count;               // members
  long long sum[6];        // centroid mode: the fixed-point sums of the members' x, y, z and of their normals
};
struct VoxelArgs {
  const float *x, *y, *z;     // the cloud, n points
  const float *nx, *ny, *nz;  // its normals, or nullptr
  int n;
  int centroid;               // 0: ICPK_VOXEL_FIRST, 1: ICPK_VOXEL_CENTROID
  double leaf;
  VoxelSlot* table;           // mask + 1 slots (a power of two >= 2 n), all zero
  unsigned mask;
  int* slot_of;               // [n] scratch: the slot of every point, -1 if dropped
  int* bsum;                  // [ceil(n / 1024)] scratch
  int* counts;                // [2]: n_out (written), n_dropped (added to: zero before the launch)
  float *ox, *oy, *oz;        // [n_out <= n] each
  float *onx, *ony, *onz;     // (with normals)
  int *first_index, *count;   // [n_out <= n]
  int* out_of_point;          // [n]
};
// the five launches of one downsample; n <= 0: nothing
void launch_voxel_downsample(const VoxelArgs& a, hipStream_t s);

// kernels_normals.hip -- K12, target normals from the target's own geometry (icpk_estimate_target_normals)
constexpr int NRM_MOMENTS = 10;  // per point: m, S_x S_y S_z, S_xx S_xy S_xz S_yy S_yz S_zz (int64 each)
struct NormalsArgs {
  GridView index;             // K1d's index of the cloud
  const float *x, *y, *z;     // the target in the caller's order, n points
  int n;
  float radius;
  int min_neighbors;
  int has_viewpoint;
  float viewpoint[3];
  long long* moments;         // [n][NRM_MOMENTS], caller's order
  float *nx, *ny, *nz;        // [n]
  int* count;                 // [n]
  float* curvature;           // [n]
  int* n_valid;               // added to: zero before the launch
};
static_assert(sizeof(NormalsArgs) == 136 && offsetof(NormalsArgs, index) == 0, "the kernarg layout is pinned");
// the two launches of one estimate (moments, then the eigen-solve); n <= 0: nothing
void launch_estimate_normals(const NormalsArgs& a, hipStream_t s);

// kernels_filter.hip -- K13, outlier removal (icpk_remove_outliers)
constexpr int FILTER_MAX_K = 64;  // ICPK_FILTER_MAX_K
// the k nearest neighbours of every query in an indexed cloud.  Queries and indexed cloud are separate arguments: the
// filter passes the index's own cell-sorted copy as the queries (every point against its own cloud)
struct KnnArgs {
  const float4* q4;        // queries (x, y, z, w): the indexed point of index bits(w) is not a neighbour (-1: none is)
  int nq;
  int k;                   // 1 .. FILTER_MAX_K
  float r0_scale;          // first search radius = h sqrt((k + 1) r0_scale), h the cell edge (efficiency only)
  int pad0;
  GridView index;          // K1d's index of the indexed cloud
  double* mean;            // [.] at bits(w) of the query: the mean of its k' smallest distances (0: none, or not finite)
  float* kth;              // [.] the k'-th
};
static_assert(sizeof(KnnArgs) == 64 && offsetof(KnnArgs, index) == 24, "the kernarg layout is pinned");
void launch_knn_mean(const KnnArgs& a, hipStream_t s);
struct FilterArgs {
  const float *x, *y, *z;     // the cloud, n points
  const float *nx, *ny, *nz;  // its normals, or nullptr
  int n;
  int kind;                   // ICPK_FILTER_*
  int min_neighbors;
  float std_ratio;
  double* value;              // [n]: mean_i / (double)m_i
  double* partial;            // [2][RED_MAX_BLOCKS] scratch of the canonical tree
  int* pcount;                // [RED_MAX_BLOCKS]
  double* summary;            // [4]: N, mu, sigma, T (STATISTICAL)
  int* bsum;                  // [ceil(n / 1024)] scratch
  int* counts;                // [2]: n_out (written), n_dropped (added to: zero before the launch)
  float *ox, *oy, *oz;        // [n_out <= n] each
  float *onx, *ony, *onz;     // (with normals)
  int* out_index;             // [n]
};
// RADIUS: value[i] = (double)m_i over K1d's index of the same cloud (K12's neighbourhood)
void launch_radius_count(const GridView& index, int n, float radius, double* value, hipStream_t s);
// threshold (STATISTICAL: the canonical sums, then mu, sigma, T on one lane) and the order-preserving compaction
void launch_filter_compact(const FilterArgs& a, hipStream_t s);

// kernels_score.hip -- K15, scoring of candidate poses (icpk_score_poses)
constexpr int NSCORE = 11;             // ICPK_NSCORE
constexpr int SCORE_CHUNK_POSES = 256;      // poses per launch at most (the partials' scratch: 11 x 256 doubles per pose) ...
constexpr size_t SCORE_CHUNK_KEYS = 1 << 24;  // ... and (pose, point) keys per launch (128 MiB of scratch)
struct ScoreArgs {
  const float *sx, *sy, *sz;  // the source points, caller's order
  int ns;
  float max_dist;
  const float* T;             // 16 floats per pose of this launch (row-major 4 x 4), or nullptr: the points as they stand
  GridView index;             // K1d's index of the target
  const float4* o4;           // the target in the caller's order
  nn_key_t* keys;             // [poses][ns]: an inlier's (distance bits << 32) | index, NN_KEY_INIT for the others
  double* partial;            // [poses][NSCORE][RED_MAX_BLOCKS] scratch of the canonical tree
  int* pcount;                // [poses][RED_MAX_BLOCKS]
  double* out;                // [poses][NSCORE + 1]: the sums, then the inlier count as an int64
};
static_assert(sizeof(ScoreArgs) == 104 && offsetof(ScoreArgs, index) == 40, "the kernarg layout is pinned");
// the three launches of one chunk of poses (search, per-block sums, final sums); n_poses <= 0: nothing
void launch_score_poses(const ScoreArgs& a, int n_poses, hipStream_t s);

// kernels_fpfh.hip -- K16, FPFH descriptors of a cloud and their matching (icpk_compute_fpfh, icpk_match_features)
constexpr int FPFH_BINS = 33;       // ICPK_FPFH_BINS: three sub-histograms of 11 bins
constexpr int FPFH_G_STRIDE = 34;   // 16-bit words per point of the normalised SPFH: the 33 bins, then "m > 0"
struct FpfhArgs {
  GridView index;             // K1d's index of the cloud
  const float *nx, *ny, *nz;  // its normals in the caller's order, n each
  int n;
  float radius;
  float4* n4;                 // [n] cell order: the normal, w = 1 for a described point and 0 for any other
  unsigned short* g;          // [n][FPFH_G_STRIDE] cell order
  int* counts;                // [n][FPFH_BINS] caller's order, or nullptr (ICPK_FPFH_KEEP_SPFH)
  int* m;                     // [n] caller's order, or nullptr
  float* desc;                // [n][FPFH_BINS] caller's order
  uint8_t* valid;             // [n]
};
static_assert(sizeof(FpfhArgs) == 104 && offsetof(FpfhArgs, index) == 0, "the kernarg layout is pinned");
// the three launches of one cloud's descriptors (normals into cell order, SPFH, FPFH); n <= 0: nothing
void launch_compute_fpfh(const FpfhArgs& a, hipStream_t s);
struct MatchArgs {
  const float* fa;            // descriptors of the side that searches, [na][FPFH_BINS] ...
  const uint8_t* va;          // ... and which of its points are valid
  int na;
  int nb;
  const float* fb;            // the side that is searched
  const uint8_t* vb;
  nn_key_t* best;             // [na], pre-set to NN_KEY_INIT: (bits(D) << 32) | index of the best valid b
};
void launch_match_features(const MatchArgs& a, hipStream_t s);
// the kept pairs in source order: every valid source with a partner, under `mutual` only where the partner's own best
// is that source.  *n_out (device) = their number; msrc / mtgt / mD: room for ns entries
void launch_match_compact(const nn_key_t* best_s, int ns, const nn_key_t* best_t, int mutual, int* msrc, int* mtgt,
                          float* mD, int* n_out, hipStream_t s);

// kernels_posegraph.hip -- K18, pose-graph optimisation (icpk_pose_graph_optimize / _evaluate); float64 throughout
struct PgEdge {  // icpk_pg_edge as the device reads it (icpk_posegraph.cpp asserts the layout)
  int32_t source, target, uncertain, reserved;
  double T[16];
  double info[36];
};
// one linearisation, left by an edge pass and a node pass over one set of poses.  Explicit blocks: J_t = -J_s, so an
// edge is ONE 6 x 6 block A and one 6-vector b (include/icpk.h): 44 doubles = 352 bytes per edge with chi2 and l
struct PgLin {
  const double* poses;  // [n_nodes][16] the poses it was taken at
  double* A;            // [n_edges][36]
  double* b;            // [n_edges][6]
  double* chi2;         // [n_edges]
  double* l;            // [n_edges]
  double* D;            // [n_nodes][36] sum of the incident edges' A
  double* g;            // [n_nodes][6]  sum of the incident edges' +-b
};
enum { PG_P_COST = 0, PG_P_PRED, PG_P_PQ, PG_P_RZ, PG_P_RR, PG_P_DMAX, PG_P_GMAX, PG_P_HMAX, PG_NPARTIAL };
struct PgScalars {  // the words of one LM iteration; the host reads them after its one wait
  double cost, pred, dmax, gmax, hmax;  // of the trial linearisation / step (pg_finish_kernel)
  double rz[2];                         // PCG: r . z of iteration k in rz[k & 1]
  double gnorm2;                        // |g|^2 over the free nodes
  int done[2];                          // PCG: iteration k does nothing when done[k & 1]
  int pcg_iters;
  int breakdown;                        // p . (H + lambda D) p was not > 0
};
struct PgArgs {
  int n_nodes, n_edges, ref;
  double mu;
  const PgEdge* edges;
  const int* adj_start;  // [n_nodes + 1]
  const int* adj;        // [2 n_edges]: 2 * edge + (1 where the node is the edge's target), ascending per node
  double* x;             // PCG vectors, [n_nodes][6] each
  double* r;
  double* z;
  double* p;
  double* q;
  double* L;             // [n_nodes][36] Cholesky factors of the damped diagonal blocks
  double* partial;       // [PG_NPARTIAL][RED_MAX_BLOCKS]
  PgScalars* scal;
};
// edge pass + node pass over lin.poses; with_finish: pg_finish_kernel behind them (cost, |g|inf, max diag H into scal)
void launch_pg_linearise(const PgArgs& a, const PgLin& lin, bool with_finish, hipStream_t s);
// one LM iteration's launches up to the trial poses: damping + factors + PCG start, max_pcg x 3 PCG launches, the
// trial update lin.poses -> trial.  Nothing waits in between
void launch_pg_solve(const PgArgs& a, const PgLin& lin, double lambda, double pcg_tol, int max_pcg, double* trial,
                     hipStream_t s);

// kernels_tsdf.hip -- K19, the dense TSDF volume (icpk_tsdf_*); the rule itself is tsdf_rule.h
constexpr int TSDF_THREADS = 256;
constexpr int TSDF_MAX_BLOCKS = 8192;  // chunks a volume is cut into: also the length of the extraction's scan
// voxels per chunk: a multiple of TSDF_THREADS, at most TSDF_MAX_BLOCKS chunks (n <= 2^30: at most 2^17)
inline long long tsdf_chunk(long long n) {
  const long long per = (n + TSDF_MAX_BLOCKS - 1) / TSDF_MAX_BLOCKS;
  const long long c = (per + TSDF_THREADS - 1) / TSDF_THREADS * TSDF_THREADS;
  return c < TSDF_THREADS ? TSDF_THREADS : c;
}
inline int tsdf_blocks(long long n) { return (int)((n + tsdf_chunk(n) - 1) / tsdf_chunk(n)); }
struct TsdfIntegrateArgs {
  TsdfFrame fr;
  const uint16_t* depth;           // rows x cols
  const float* intensity_image;    // rows x cols, or null ...
  float* tsdf;
  uint16_t* weight;
  float* intensity;                // ... as the volume's intensity plane is
  long long n, chunk;
  int* slots;                      // [nblocks] voxels written per chunk
};
// one frame into the volume; *n_updated (device) = the voxels written
void launch_tsdf_integrate(const TsdfIntegrateArgs& a, int nblocks, long long* n_updated, hipStream_t s);
struct TsdfExtractArgs {
  TsdfPlanes v;
  long long n, chunk;
  int* counts;         // [nblocks] crossings listed per chunk
  int* dropped;        // [nblocks] crossings without a normal per chunk
  long long* offsets;  // [nblocks + 1] the scan of counts
  long long capacity;  // entries the list has room for
  float *x, *y, *z, *nx, *ny, *nz, *intensity;
  int* voxel_index;
  uint8_t* axis;
  bool leaving;        // K23: only the crossings a shift would lose ...
  TsdfKeep keep;       // ... that keeps this box of voxels (read only when leaving)
};
// count pass + scan: totals[0] = crossings to list, totals[1] = crossings dropped (device)
void launch_tsdf_count(const TsdfExtractArgs& a, int nblocks, long long* totals, hipStream_t s);
void launch_tsdf_scatter(const TsdfExtractArgs& a, int nblocks, hipStream_t s);

// K23, the shift of the volume by whole voxels: out of place, every destination voxel written once (moved or fresh)
constexpr int TSDF_SHIFT_RUN = 4;  // consecutive voxels a thread owns: one 16-byte store to the tsdf plane
struct TsdfShiftArgs {
  const float* tsdf_in;
  const uint16_t* weight_in;
  const float* intensity_in;  // or null, with intensity_out
  float* tsdf_out;
  uint16_t* weight_out;
  float* intensity_out;
  int dims[3];
  int s[3];                   // clamped to -dims .. dims
  long long n, chunk;
};
void launch_tsdf_shift(const TsdfShiftArgs& a, int nblocks, hipStream_t s);
// the sub-box [lo, lo + size) of a plane, packed x fastest into out (size[0] size[1] size[2] entries)
struct TsdfBoxArgs {
  int dims[3], lo[3], size[3];
  long long m;                // entries of the box
};
void launch_tsdf_box(const TsdfBoxArgs& a, const float* plane, float* out, hipStream_t s);
void launch_tsdf_box(const TsdfBoxArgs& a, const uint16_t* plane, uint16_t* out, hipStream_t s);

// K20, the ray cast of the volume (the ray rule of tsdf_rule.h).  A workgroup of TSDF_THREADS covers a tile of
// TSDF_RAY_TILE x TSDF_RAY_TILE pixels, each of its four waves an 8 x 8 quarter; the tiles are dealt out to at most
// TSDF_MAX_BLOCKS workgroups, so that the counts fit K19's slots
constexpr int TSDF_RAY_TILE = 16;
inline int tsdf_ray_tiles(int n) { return (n + TSDF_RAY_TILE - 1) / TSDF_RAY_TILE; }
inline int tsdf_ray_blocks(int rows, int cols) {
  const long long t = (long long)tsdf_ray_tiles(rows) * tsdf_ray_tiles(cols);
  return (int)(t < TSDF_MAX_BLOCKS ? t : TSDF_MAX_BLOCKS);
}
struct TsdfRaycastArgs {
  TsdfPlanes v;
  TsdfRay r;
  float* maps;    // 8 planes of rows x cols: x, y, z, nx, ny, nz, depth, intensity
  int tiles_x;    // tiles per row of tiles
  int ntiles;
  int* hits;      // [nblocks] listed hits per workgroup
  int* dropped;   // [nblocks] crossings without a normal per workgroup
};
// the maps; totals[0] = listed hits, totals[1] = crossings without a normal (device)
void launch_tsdf_raycast(const TsdfRaycastArgs& a, int nblocks, long long* totals, hipStream_t s);
// the valid pixels of the maps (depth > 0) as a list in row-major pixel order: chunks of TSDF_THREADS consecutive pixels
struct TsdfRayCompactArgs {
  const float* maps;
  int npix;            // <= TSDF_MAX_BLOCKS * TSDF_THREADS
  int* counts;         // [nblocks] valid pixels per chunk
  long long* offsets;  // [nblocks + 1] the scan of counts
  long long capacity;  // entries of each of the list's planes
  float* list;         // 7 planes: x, y, z, nx, ny, nz, intensity
};
inline int tsdf_ray_chunks(int npix) { return (npix + TSDF_THREADS - 1) / TSDF_THREADS; }
// count pass + scan: totals[0] = the valid pixels (device)
void launch_tsdf_ray_count(const TsdfRayCompactArgs& a, long long* totals, hipStream_t s);
void launch_tsdf_ray_scatter(const TsdfRayCompactArgs& a, hipStream_t s);

// K21, the triangle mesh of the volume (the mesh rule of tsdf_rule.h), over K19's chunks
struct TsdfMeshArgs {
  TsdfPlanes v;
  long long n, chunk;
  int* vcounts;         // [nblocks] vertices listed per chunk
  int* tcounts;         // [nblocks] triangles per chunk
  int* nonormal;        // [nblocks] listed vertices without a normal per chunk
  long long* voffsets;  // [nblocks + 1] the scan of vcounts: also the range a vertex look-up searches
  long long* toffsets;  // [nblocks + 1] the scan of tcounts
  long long vcapacity, tcapacity;  // entries the vertex list / the triangle list has room for
  float *x, *y, *z, *nx, *ny, *nz, *intensity;
  int* voxel_index;     // the key of every vertex: its owner voxel ...
  uint8_t* edge;        // ... and its edge type 1 .. 7
  int* triangles;       // 3 per triangle
};
// count pass + two scans: totals[0] = vertices, totals[1] = vertices without a normal, totals[2] = triangles (device)
void launch_tsdf_mesh_count(const TsdfMeshArgs& a, int nblocks, long long* totals, hipStream_t s);
// the vertices, then the triangles
void launch_tsdf_mesh_scatter(const TsdfMeshArgs& a, int nblocks, hipStream_t s);

// kernels_tsdf_apply.hip -- K30, several signed frame updates in one pass over the volume (the signed update rule of
// tsdf_rule.h), over K19's chunks
constexpr int TSDF_MAX_OPS = 16;  // ICPK_TSDF_MAX_OPS
struct TsdfApplyOp {
  float R[9], t[3];  // world -> camera, as TsdfFrame's
  int sign;          // +1 or -1
  int frame;         // which image of the stack: < n_frames
};
struct TsdfApplyArgs {
  TsdfFrame fr;                  // the geometry and the camera; its R and t are taken from the op
  const uint16_t* depth;         // the stack: n_frames x rows x cols
  const float* intensity_image;  // the same, or null ...
  float* tsdf;
  uint16_t* weight;
  float* intensity;              // ... as the volume's intensity plane is
  long long n, chunk;
  long long npix;                // rows x cols: one image of the stack
  int n_ops;
  int* slots;                    // [nblocks][TSDF_MAX_OPS] voxels written per chunk and op
  TsdfApplyOp ops[TSDF_MAX_OPS];
};
// the ops in order, voxel by voxel; n_updated[k] (device, n_ops entries) = the voxels op k wrote
void launch_tsdf_apply(const TsdfApplyArgs& a, int nblocks, long long* n_updated, hipStream_t s);

// kernels_projective.hip -- K25, projective frame-to-model alignment (the projective rule is projective_rule.h)
constexpr int PROJ_MAX_ITER = 64;  // ICPK_PROJECTIVE_MAX_ITERATIONS
// The loop's state on the device: the reduce launch reads `done` and the float pose, the step launch behind it writes
// the trace entry of its iteration and either the next pose or done + status.
struct ProjState {
  int done;
  int status;
  int iterations;  // updates made
  int pad0;
  float R[9], t[3];  // E_k rounded to float once: what the reduce launch moves the vertices by
  double E[12];      // E_k, rows of [R | t]
};
struct ProjIter {  // icpk_projective_iter
  double E[12];
  double sums[NP2L];
  long long count;
  int status;
  int pad0;
};
// state and trace in one allocation, so that both come back with one copy
struct ProjBlock {
  ProjState st;
  ProjIter trace[PROJ_MAX_ITER];
};
struct ProjArgs {
  const uint16_t* depth;  // the level
  int rows, cols;
  float fx, cx;           // fx / 2^l, cx / 2^l
  const float* maps;      // the ray cast's planes, npix_v floats each: x, y, z, nx, ny, nz, depth, intensity
  int rows_v, cols_v;
  float fx_v, cx_v;
  float Q[9], s[3];       // the view's pose inverted
  float max_dist, min_normal_cos;
  double* partial;        // [NP2L][RED_MAX_BLOCKS]
  int* pcount;            // [RED_MAX_BLOCKS]
  const ProjState* st;
  // K26, the coloured step (grad == nullptr: the geometric one): the level's intensities, the view's three gradient
  // planes (npix_v floats each) and lambda_geometric; the view's intensity is plane 7 of maps
  const float* inten;
  const float* grad;
  float lambda_geometric;
};
// red_blocks(rows cols) workgroups: the per-block partials of one evaluation at the state's pose (nothing once done)
void launch_proj_reduce(const ProjArgs& a, hipStream_t s);
// one workgroup: the canonical stage 2, then iteration k of the loop rule on one lane
void launch_proj_step(const double* partial, const int* pcount, int nblocks, ProjBlock* blk, int k, int min_pairs,
                      hipStream_t s);
// every pixel's code or view pixel, and its distance, at the state's pose (device arrays of rows cols entries)
void launch_proj_associate(const ProjArgs& a, int32_t* pixel, float* dist, hipStream_t s);

// kernels_frame_view.hip -- K28, the frame view (the frame view rule is frame_view_rule.h)
constexpr int FRAME_VIEW_THREADS = 256;
constexpr int FRAME_VIEW_MAX_LEVELS = 8;  // ICPK_PYRAMID_MAX_LEVELS
struct FrameViewLevel {
  const uint16_t* depth;  // the pyramid's level ...
  const float* inten;     // ... and its intensities (nullptr: the view's intensity plane holds 0)
  float* planes;          // 8 planes of rows cols floats: x, y, z, nx, ny, nz, depth, intensity
  int rows, cols;
  float fx, cx;           // fx / 2^l, cx / 2^l
};
struct FrameViewArgs {
  FrameViewLevel level[FRAME_VIEW_MAX_LEVELS];
  int block0[FRAME_VIEW_MAX_LEVELS + 1];  // level l owns workgroups block0[l] .. block0[l + 1); [levels]: the grid
  int levels;
  float R[9], t[3];  // the pose rounded to float once
  int* slots;        // [2 x grid] listed pixels, pixels without a normal, per workgroup
};
inline int frame_view_blocks(int npix) { return (npix + FRAME_VIEW_THREADS - 1) / FRAME_VIEW_THREADS; }
// every level in one launch, then totals[2 l], totals[2 l + 1] = level l's two counts (device, 2 x levels ints)
void launch_frame_view(const FrameViewArgs& a, int* totals, hipStream_t s);

// kernels_sdf_track.hip -- K29, frames tracked directly against the TSDF (the SDF tracking rule is sdf_track_rule.h).
// The loop's state, trace and step launch are K25's (ProjState, ProjBlock, launch_proj_step), on a block of its own.
struct SdfArgs {
  const uint16_t* depth;  // the level
  int rows, cols;
  float fx, cx;           // fx / 2^l, cx / 2^l
  TsdfPlanes vol;         // the volume's planes, dims, voxel, CURRENT origin and min_weight
  float trunc, max_abs_tsdf, min_normal_cos;
  double* partial;        // [NP2L][RED_MAX_BLOCKS]
  int* pcount;            // [RED_MAX_BLOCKS]
  const ProjState* st;
};
// red_blocks(rows cols) workgroups: the per-block partials of one evaluation at the state's pose (nothing once done)
void launch_sdf_reduce(const SdfArgs& a, hipStream_t s);
// every pixel's cell or code, and its distance D, at the state's pose (device arrays of rows cols entries)
void launch_sdf_associate(const SdfArgs& a, int32_t* cell, float* value, hipStream_t s);

// kernels_esdf.hip -- K31, the Euclidean distance map of the TSDF volume (the distance rule and the query rule are
// esdf_rule.h), over K19's chunks: a thread owns a voxel in every pass
#ifndef ICPK_ESDF_STEP
#define ICPK_ESDF_STEP 4  // (a diagnostic build may set another: DESIGN.md K31 has what 1 .. 16 measured)
#endif
constexpr int ESDF_STEP = ICPK_ESDF_STEP;  // offsets a lane takes between two looks at its bound (esdf_line_min's STEP)
struct EsdfArgs {
  const float* tsdf;       // the volume's planes: read by the classification alone
  const uint16_t* weight;
  uint8_t* cls;            // the class plane
  int32_t* plane[2];       // the signed plane of the passes: x writes [0], y [1], z [0] again, which then holds q
  int dims[3];
  long long n, chunk;
  int min_weight, flags, R;
  int* slots;              // [4][TSDF_MAX_BLOCKS] per chunk: voxels of class 0, 1, 2; voxels with |q| == FAR
};
// classification, the three passes and counts[4] (device) = n_unknown, n_free, n_occupied, n_far
void launch_esdf_compute(const EsdfArgs& a, int nblocks, long long* counts, hipStream_t s);
// sq, cls and m(q) of the sub-box into packed arrays of a.m entries (device; any may be null)
struct EsdfBoxArgs {
  TsdfBoxArgs box;
  const int32_t* sq;
  const uint8_t* cls;
  int R;
  float voxel;
};
void launch_esdf_box(const EsdfBoxArgs& a, int32_t* sq_out, uint8_t* cls_out, float* dist_out, hipStream_t s);
// THE QUERY RULE for n points: xyz three planes of n floats in, out five planes of n words: dist, gx, gy, gz and the
// status widened to an int
void launch_esdf_query(const EsdfMap& m, const float* xyz, int n, float* out, hipStream_t s);

// kernels_brief.hip -- K32, oriented BRIEF descriptors of key points and their Hamming matches (the rule is brief_rule.h)
constexpr int BRIEF_MATCH_CHUNK = 512;  // descriptors of the scanned side per run (grid.y of the match launch)
inline int brief_match_runs(int n_scanned) { return n_scanned < 1 ? 1 : (n_scanned + BRIEF_MATCH_CHUNK - 1) / BRIEF_MATCH_CHUNK; }
// words [n][8], bin [n], valid [n] of the n key points kp (x, y floats) against the device image; table: BRIEF_TABLE
void launch_brief_describe(const uint8_t* img, int rows, int cols, int channels, const float* kp, int n, int upright,
                           const int8_t* table, uint32_t* words, uint8_t* bin, uint8_t* valid, hipStream_t s);
struct BriefSide {
  const uint32_t* words;
  const uint8_t* valid;
  int n;
};
// for every descriptor i of a and every run c of b: key[c a.n + i] = H << 32 | j, h2[c a.n + i] = H2 over the valid
// descriptors of the run (j all ones: none)
void launch_brief_match(const BriefSide& a, const BriefSide& b, unsigned long long* key, unsigned* h2, hipStream_t s);
struct BriefFinishArgs {
  const unsigned long long* key[2];  // [0] sources against targets, [1] targets against sources (mutual only)
  const unsigned* h2[2];
  int runs[2];
  int ns, nt;
  const uint8_t* valid_s;
  int max_hamming, ratio_num, ratio_den, mutual;
  const int* map_s;  // key point -> cloud index of either side, or both null
  const int* map_t;
  int *out_src, *out_tgt, *out_H, *out_H2;  // [ns] the kept pairs, source order
  int *cl_src, *cl_tgt;                     // [ns] K16's list (with the maps)
  float* cl_D;
  int* counts;  // kept pairs, pairs in K16's list
  int* cl_n;    // K16's count word, or null
};
void launch_brief_finish(const BriefFinishArgs& a, hipStream_t s);

// kernels_cluster.hip -- K33, DBSCAN clustering of an indexed cloud (icpk_cluster_dbscan; the shared parts of the rule
// are cluster_rule.h)
constexpr int CL_COUNTS = 8;  // words of ClusterArgs::counts (a multiple of 16 bytes, zeroed before every call)
enum { CL_N_CLUSTERS = 0, CL_N_NOISE = 1, CL_N_OUT = 2, CL_N_DROPPED = 3, CL_ERROR = 4, CL_LARGEST = 5 };
struct ClusterArgs {
  GridView index;             // K1d's index of the cloud
  const float *x, *y, *z;     // the cloud in the caller's order, n points
  const float *nx, *ny, *nz;  // its normals, or nullptr
  int n;
  float eps;
  int min_points, min_size, max_size, largest_only;
  // the record, by original index
  int* labels;                // [n] (the root between the flatten and the label launches)
  uint8_t* core;              // [n]
  int* count;                 // [n] m_i
  int* nearest;               // [n] nearest_core
  int* out_index;             // [n]
  int* sizes;                 // [n_clusters <= n]
  int* first;                 // [n_clusters <= n]
  // scratch
  int* parent;                // [n] the union-find forest over the core points
  int* cid;                   // [n] a representative's cluster id
  int* bsum;                  // [ceil(n / 1024)]
  int* counts;                // [CL_COUNTS]: CL_*, zero before the launches
  float *ox, *oy, *oz;        // [n_out <= n] each
  float *onx, *ony, *onz;     // (with normals)
};
// every launch of one call: count, link, flatten / scan / rank / label, the largest cluster if asked for, and the
// selection's flag / scan / emit.  n <= 0: nothing
void launch_cluster_dbscan(const ClusterArgs& a, hipStream_t s);

// kernels_plane.hip -- K34, RANSAC plane segmentation of a cloud (icpk_segment_planes; the rule is plane_rule.h)
struct PlaneHyp;                 // plane_rule.h: one hypothesis, 64 bytes
constexpr int PL_COUNTS = 8;     // words of one round's count block (PlaneArgs::counts; all blocks zeroed before a call)
constexpr int PL_MAX_PLANES = 16;  // ICPK_PLANE_MAX_PLANES: rounds, and so count blocks but the selection's
enum { PL_M = 0, PL_WINNER = 1, PL_RANSAC = 2, PL_FINAL = 3, PL_ACCEPTED = 4, PL_FIT = 5, PL_N_OUT = 6 };
struct PlaneArgs {
  const float *x, *y, *z;     // the cloud in the caller's order, n points
  const float *nx, *ny, *nz;  // its normals, or nullptr (the selection carries them)
  int n;
  unsigned long long seed;
  float t;                    // distance_threshold
  int H, min_inliers;
  int round;                  // r: the label this round gives, the record's slot
  int m_bound;                // an upper bound on |E| of this round that the host knows: it sizes the launches over E
  int keep_inliers, select_plane;  // the selection
  int* labels;                // [n] -1, or the plane
  int* out_index;             // [n]
  float4* E;                  // [n] scratch: the round's list, (x, y, z, index bits)
  int* bsum;                  // [ceil(n / 1024)]
  int* counts;                // [PL_COUNTS] THIS round's (or the selection's) block: PL_*
  PlaneHyp* hyp;              // [H]
  int* hyp_idx;               // [3 H] the samples' indices in the cloud
  int* hcount;                // [H] c_h
  double* partial;            // [9][RED_MAX_BLOCKS] scratch of the canonical tree
  int* pcount;                // [RED_MAX_BLOCKS]
  double* model;              // [8] per plane
  int* info;                  // [6] per plane: h, the three samples, the RANSAC count, the final count
  double* sums;               // [9] per plane
  float *ox, *oy, *oz;        // [n_out <= n] each
  float *onx, *ony, *onz;     // (with normals)
};
// every launch of round a.round: E, the hypotheses, the count, the pick, the refit, the final inliers and their labels.
// The host reads a.counts afterwards.  n <= 0: nothing
void launch_plane_round(const PlaneArgs& a, hipStream_t s);
// the selection's flag / scan / emit: out_index, the selected cloud, counts[PL_N_OUT].  n <= 0: nothing
void launch_plane_select(const PlaneArgs& a, hipStream_t s);

}  // namespace icpk
