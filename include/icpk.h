/*
 * icpk.h -- C ABI of libicpk.so: the MI355X (gfx950) implementation of the ICP
 * inner loop of BenniG123/icp-slam-prototype.
 *
 * This is the drop-in boundary.  The reference has no
 * FFI: its hot path is C++ called in-process.  Each entry point below names the
 * reference code it replaces ("file:line" relative to the reference checkout).
 * Plain pointers and sizes only; no C++/torch types; nothing throws across the
 * boundary.  All functions return an int status (ICPK_OK == 0, negative =
 * error, positive = completed with a documented fallback) unless noted.
 *
 * There is NO CPU fallback: icpk_create fails with ICPK_E_NO_DEVICE when no HIP
 * device is usable.
 *
 * Data layout: point clouds are xyz structure-of-arrays (three float planes),
 * replacing the reference's 16-byte AoS color_point_t (pointcloud.hpp:13-19);
 * colour is dropped from the pair distance because COLOR_WEIGHT is 0.0f
 * (icp.hpp:6); colored ICP (K17) takes one intensity per point in arrays of its
 * own.  Coordinates are
 * expected to be finite (the reference produces them from uint16 depth): a NaN/inf
 * point never faults or hangs a kernel and never pairs, but which index it reports
 * is unspecified.
 */
#ifndef ICPK_H
#define ICPK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ICPK_VERSION_STRING "icpk 0.3.0 (gfx950)"

/* ---- status codes -------------------------------------------------------- */
#define ICPK_OK 0
#define ICPK_W_DEGENERATE 2       /* point-to-plane normal equations not positive definite:  \
                                    iteration stopped, transform so far returned            */
#define ICPK_W_EMPTY_MAP 3       /* icpk_associate_keypoints with an empty target: outputs left \
                                    untouched, as icp.cpp:490-491 returns before clearing them  */
#define ICPK_W_TOO_FEW_PAIRS 1   /* < min_pairs associations: fell back to the  \
                                    caller's last motion (icp.cpp:163-182)      */
#define ICPK_E_ARG (-1)          /* null pointer / negative size / bad enum     */
#define ICPK_E_EMPTY_TARGET (-2) /* icp.cpp:572 dereferences begin(): UB there  */
#define ICPK_E_HIP (-3)          /* a HIP runtime call failed (see last_error)  */
#define ICPK_E_NOT_SET (-4)      /* source or target not uploaded yet           */
#define ICPK_E_NO_DEVICE (-5)    /* no usable HIP device: no CPU fallback       */
#define ICPK_E_RCCL (-6)         /* librccl missing or an RCCL call failed       */

/* ---- reference constants (defaults of icpk_default_params) --------------- */
#define ICPK_MAX_NN_DISTANCE 0.75f          /* icp.hpp:8  MAX_NN_COLOR_DISTANCE    */
#define ICPK_MAX_NN_KEYPOINT_DISTANCE 0.1f  /* icp.hpp:10 MAX_NN_KEYPOINT_DISTANCE */
#define ICPK_DEFAULT_MAX_ITERATIONS 16      /* SLAM.cpp:277                        */
#define ICPK_DEFAULT_THRESHOLD 0.0001f      /* SLAM.cpp:277                        */
#define ICPK_MIN_PAIRS 3                    /* icp.cpp:163                         */
#define ICPK_FX 468.60f                     /* pointcloud.hpp:7                    */
#define ICPK_CX 318.27f                     /* pointcloud.hpp:9                    */
#define ICPK_DEPTH_SCALE 5000.0f            /* pointcloud.cpp:37                   */

/* solve flavours */
#define ICPK_SOLVE_REFERENCE 0 /* bug-for-bug icp.cpp:199-246 (un-centred moment,    \
                                  R = V U^T, column-2 flip, mean-difference offset)  */
#define ICPK_SOLVE_KABSCH 1    /* centred Kabsch, rigid_transform_3D.py:9-40         */
#define ICPK_SOLVE_POINT_TO_PLANE 2 /* linearised point-to-plane (extension: TODO:9 of the \
                                       reference only plans it); needs target normals     */
#define ICPK_SOLVE_PLANE_TO_PLANE 3 /* plane-to-plane step of Generalized-ICP (extension, K14): \
                                       needs source AND target normals; see the section below */

/* nearest-neighbour kernel selection */
#define ICPK_NN_EXACT 0    /* literal double-precision distance per pair             */
#define ICPK_NN_FILTERED 1 /* seeded fp32 filter + exact re-evaluation; same results */
#define ICPK_NN_PRUNED 2   /* FILTERED + skipping of target tiles whose bounding box is out \
                              of reach; same results                                   */
#define ICPK_NN_GRID 3     /* uniform grid over the target: only the cells that meet the cube \
                              [q - r, q + r] around a query with seed distance r are scanned; \
                              same results; default                                     */
#define ICPK_NN_MAP 4      /* the reference's mapped lookup (icp.cpp:347-486, K9): NOT the nearest target but \
                              what the voxel walk of icpk_map_nearest finds; only against the map's current  \
                              lookup target (icpk_map_lookup_to_target), see there                       */

/* log keys mirrored from SLAM.hpp:4-13 for the optional callback */
#define ICPK_LOG_NEAREST_NEIGHBOR 0
#define ICPK_LOG_RECONSTRUCT_POINT_CLOUDS 5
#define ICPK_LOG_SVD 6
#define ICPK_LOG_ROTATE 7
#define ICPK_LOG_MSE 8

/* Canonical reduction geometry (part of the ABI: it fixes the summation order
 * of icpk_reduce so results are bit-reproducible and checkable): 256-thread
 * blocks, B = clamp(ceil(n/256), 1, 256) blocks, thread g sums elements
 * g, g+256B, ... in order; 64-lane xor butterfly; ((w0+w1)+w2)+w3; the B block
 * sums (padded to 256 slots with +0.0) go through the same 4-wave tree again. */
#define ICPK_RED_THREADS 256
#define ICPK_RED_MAX_BLOCKS 256
#define ICPK_NP2L 28 /* point-to-plane sums: [0..20] upper triangle of J J^T (row-major),  \
                        [21..26] J r, [27] sum dist; J = [p x n ; n], r = (p - q).n      */
#define ICPK_NSUM 19 /* [0..8] M[r][c]=sum b_r a_c, [9..11] sum (float)(a-b), \
                        [12] sum dist, [13..15] sum a, [16..18] sum b          */
/* icpk_reduce_weighted (robust alignment, icpk_set_robust): the same sums with every term multiplied by the pair's
 * weight w, over the accepted pairs, canonical tree -- except the distance sum, which stays unweighted (the loop test
 * reads it) -- followed by W = sum w and the kept count (pairs with w > 0) as a float64:
 *   ICPK_NSUM_W: [0..18] as ICPK_NSUM (weighted; [12] unweighted), [19] W, [20] kept
 *   ICPK_NP2L_W: [0..26] as ICPK_NP2L (weighted), [27] unweighted sum dist, [28] W, [29] kept */
#define ICPK_NSUM_W 21
#define ICPK_NP2L_W 30

typedef struct icpk_ctx icpk_ctx; /* opaque: owns device buffers + one HIP stream */

typedef struct icpk_params {
  int32_t max_iterations;   /* SLAM.cpp:277 (16)                                  */
  float threshold;          /* SLAM.cpp:277 (1e-4): loop while mse > threshold    */
  float max_nn_dist;        /* icp.hpp:8 (0.75) or icp.hpp:10 (0.1)               */
  int32_t min_pairs;        /* icp.cpp:163 (3); < 1: ICPK_E_ARG                   */
  int32_t solve;            /* ICPK_SOLVE_*                                       */
  int32_t fixed_iterations; /* 1: ignore threshold, run max_iterations (bench)    */
  int32_t nn_mode;          /* ICPK_NN_*                                          */
  int32_t profile;          /* 1: HIP events around the NN kernels -> stats.nn_ms_total;
                               2: around every stage (reduce, transform) as well   */
  float last_rotation[9];    /* caller's previous motion, icp.cpp:23,176          */
  float last_translation[3]; /* icp.cpp:25,177                                    */
  int32_t host_loop;        /* 0 (default): every iteration's kernels are enqueued up front
                               and the loop test / solve run on the device (no host round
                               trip per iteration); 1: the host drives each iteration and
                               solves (one 160-byte read-back per iteration).  Same results. */
  int32_t profile_stride;   /* profile == 1 only: bracket every n-th NN launch (0, 1: every one;
                               the offset advances with every alignment, so the sample covers all
                               sweep positions); an event pair costs ~4 us of queue time, which a
                               20 us kernel notices */
} icpk_params;

typedef struct icpk_stats {
  int32_t iterations;  /* completed loop bodies (icp.cpp:257)                     */
  int32_t status;      /* same value icpk_align returned                          */
  int32_t final_pairs; /* associations after the last sweep                       */
  float final_mse;     /* meanSquareError of the last sweep (icp.cpp:264)         */
  int32_t nn_launches; /* NN sweeps launched (= iterations + 1)                   */
  int32_t nn_timed_launches; /* NN launches bracketed by events (see profile_stride)    */
  /* device times measured with HIP events on the context's stream; filled only
   * when params.profile != 0 */
  float nn_ms_total;        /* sum over the nn_timed_launches bracketed NN kernels */
  float reduce_ms_total;    /* association reduce kernels                         */
  float transform_ms_total; /* point transform kernels                            */
  float total_ms;           /* first to last recorded event                       */
} icpk_stats;

/* One frame pair for icpk_align_batch (xyz-SoA: host pointers; icpk_align_batch_device:
 * device pointers on the context's device).  idx_out / dist_out: optional HOST arrays of ns
 * entries that receive the pair's final associations (as icpk_get_associations); NULL = not
 * wanted. */
typedef struct icpk_pair {
  const float *sx, *sy, *sz;
  int32_t ns;
  const float *tx, *ty, *tz;
  int32_t nt;
  int32_t *idx_out;
  float *dist_out;
} icpk_pair;

/* same shape as logDeltaTime(int logKey, int quantity) (SLAM.hpp:30,
 * SLAM.cpp:493-510) plus the elapsed microseconds the reference computes
 * internally */
typedef void (*icpk_log_fn)(int key, int quantity, double usec, void *user);

/* ---- lifetime ------------------------------------------------------------ */
const char *icpk_version(void);
int icpk_create(icpk_ctx **out, int device_id);
void icpk_destroy(icpk_ctx *ctx);
const char *icpk_last_error(const icpk_ctx *ctx);
void icpk_default_params(icpk_params *p);
int icpk_set_log_callback(icpk_ctx *ctx, icpk_log_fn fn, void *user);
/* the HIP stream all work of this context is enqueued on (hipStream_t) */
void *icpk_stream(icpk_ctx *ctx);

/* ---- clouds: replaces the PointCloud containers built at icp.cpp:38-39 ---- */
/* host pointers (copied; caller keeps ownership) */
int icpk_set_target(icpk_ctx *ctx, const float *x, const float *y, const float *z, int32_t n);
int icpk_set_source(icpk_ctx *ctx, const float *x, const float *y, const float *z, int32_t n);
/* device pointers on the context's device (copied device-to-device) */
int icpk_set_target_device(icpk_ctx *ctx, const float *dx, const float *dy, const float *dz, int32_t n);
int icpk_set_source_device(icpk_ctx *ctx, const float *dx, const float *dy, const float *dz, int32_t n);
/* working copy of the source <- the cloud last given to icpk_set_source*     */
int icpk_reset_source(icpk_ctx *ctx);
/* the cloud icpk_align / icpk_reset_source start from <- the working copy (makes
 * transforms applied with icpk_transform_source permanent; device-side copy) */
int icpk_commit_source(icpk_ctx *ctx);
/* current (transformed) source, to host */
int icpk_get_source(icpk_ctx *ctx, float *x, float *y, float *z);
/* target cloud as the device holds it (after icpk_transform_target / icpk_backproject) */
int icpk_get_target(icpk_ctx *ctx, float *x, float *y, float *z);
int32_t icpk_source_size(const icpk_ctx *ctx);
int32_t icpk_target_size(const icpk_ctx *ctx);

/* ---- the three steps of one iteration ------------------------------------ */
/* icp.cpp:541-563 findGlobalNearestNeighborAssociations + :566-593
 * getNearestPoint + :606-620 distance.  For every source point the index of
 * the target element the reference scan would copy (strict '<' on the float
 * distance, lowest index wins ties) and that distance.  Outputs may be NULL
 * (results stay on the device for icpk_reduce).  The `d < max` acceptance of
 * icp.cpp:553 is applied by the consumers, not here. */
int icpk_nn(icpk_ctx *ctx, int32_t nn_mode, int32_t *idx_out, float *dist_out);
/* icp.cpp:186-212 (association split + cross moment), :314-344
 * (calculateOffset sums), :622-638 (meanSquareError sum), in one pass over the
 * associations of the last icpk_nn, canonical order.  sums: ICPK_NSUM doubles. */
int icpk_reduce(icpk_ctx *ctx, float max_dist, double *sums, int64_t *count);
/* pointcloud.cpp:321-346 rotate + :349-359 translate:
 * p <- fl32(fl32(R p) + t), R row-major, applied to the working source. */
int icpk_transform_source(icpk_ctx *ctx, const float R[9], const float t[3]);
/* same transform applied to the target cloud (the reference moves the previous
 * frame into the world frame the same way, icp.cpp:58-59) */
int icpk_transform_target(icpk_ctx *ctx, const float R[9], const float t[3]);
/* associations of the last sweep (device -> host) */
int icpk_get_associations(icpk_ctx *ctx, int32_t *idx_out, float *dist_out);

/* icp.cpp:488-515 findGlobalKeyPointAssociations + :517-539 getNearestKeyPoint -- the LIVE
 * association of the reference (icp.cpp:98,255) -- on the context's clouds: source = the frame's
 * key points, target = the map's key points.  One NN sweep (same kernels as icpk_nn), then the
 * order-preserving split on the device:
 *   assoc_query / assoc_target / assoc_dist  [*n_assoc]  accepted pairs in query order
 *       (`associations`, `errors`; rebuilt by every call, icp.cpp:497-498), accepted iff
 *       dist < max_dist (MAX_NN_KEYPOINT_DISTANCE 0.1f, icp.hpp:10 / icp.cpp:503);
 *   rejected_query [rejected_capacity]  the rejected query indices are APPENDED at *n_rejected,
 *       which is in/out (`nonAssociations` is never cleared between sweeps, icp.cpp:507-509).
 * Arrays need room for the source size.  Empty target: returns ICPK_W_EMPTY_MAP and touches
 * nothing (icp.cpp:490-491).  Inside icpk_align the same acceptance is params.max_nn_dist. */
int icpk_associate_keypoints(icpk_ctx *ctx, int32_t nn_mode, float max_dist, int32_t *assoc_query,
                             int32_t *assoc_target, float *assoc_dist, int32_t *n_assoc,
                             int32_t *rejected_query, int32_t rejected_capacity, int32_t *n_rejected);

/* ---- whole loop: replaces icp.cpp:98-268 --------------------------------- */
/* Starts from the source as uploaded (icpk_reset_source), leaves the aligned
 * source on the device.  T_out: row-major 4x4, same content as the CV_32FC1
 * matrix icp::getTransformation returns (icp.cpp:29,227-233,266-268) with row
 * 3 = (0,0,0,1) instead of uninitialised memory.  stats may be NULL.
 * Returns as soon as T_out / stats / the trace are final (the device writes them into pinned, mapped host memory);
 * the last launches of the call -- the caller-order copy of the aligned source among them -- may still be running,
 * and every later call on this context is ordered behind them (icpk_get_source and icpk_get_associations wait). */
int icpk_align(icpk_ctx *ctx, const icpk_params *p, float T_out[16], icpk_stats *stats);
/* Per-iteration record of the last icpk_align: for iteration i < *n_iter,
 * R_out[9*i..] is the rotation found (icp.cpp:218-223, before inversion),
 * t_out[3*i..] the offset (reference flavour, icp.cpp:240) or translation
 * (Kabsch), pairs_out[i] / mse_out[i] the association count and MSE the loop
 * test at icp.cpp:155 saw.  The caller needs these to keep the reference's pose
 * state (cameraRotation *= R^-1, cameraPosition -= offset, icp.cpp:237,246).
 * Arrays sized for params.max_iterations entries; any may be NULL. */
int icpk_get_trace(icpk_ctx *ctx, int32_t *n_iter, float *R_out, float *t_out, int32_t *pairs_out,
                   float *mse_out);
/* ---- robust alignment (extension: the reference plans it, TODO:5 and TODO:10, icp.cpp:328-330) ----------------
 * A setting of the context, off by default; off, every path runs exactly what it runs without it.  On, every sweep
 * of the loop (the initial one and the one after every completed iteration) weighs its pairs:
 *   accepted  the pairs the flavour's reduction accepts: d < max_nn_dist (point-to-plane: and a non-zero target
 *             normal); n of them.  d is the NN distance in both flavours (not the point-to-plane residual).
 *   cut tau   k = clamp(ceil((double)trim_fraction * n), 1, n); tau = the k-th smallest accepted d (from 1); a pair
 *             is kept if it is accepted and d <= tau (ties at the cut are kept)
 *   median m  the ceil(n/2)-th smallest accepted d, before trimming (n = 0: tau = m = 0)
 *   scale c   (double)scale, or (double)scale * 1.4826 * (double)m; w(d) in float64 as below, 0 for a trimmed pair;
 *             "kept" means w > 0
 *   solve     Kabsch from the weighted centred sums (n -> W = sum w, sum a -> sum w a, sum b -> sum w b,
 *             sum b a^T -> sum w b a^T); point-to-plane with its 27 normal-equation terms multiplied by w
 *   control   unchanged: the loop test (icp.cpp:155), stats.final_pairs / final_mse and icpk_get_trace's pairs / mse
 *             are those of the accepted pairs, unweighted; min_pairs applies to the KEPT count (below it the
 *             fallback to the caller's last motion, ICPK_W_TOO_FEW_PAIRS)
 * The identity setting (NONE, FIXED, any scale, trim_fraction 1) runs the robust kernels and returns T, statistics
 * and trace bit-equal to the plain flavour.
 * Where it applies: icpk_align (Kabsch and point-to-plane, every nn_mode, device and host loop: the same bits;
 * ICPK_E_ARG for the reference flavour); icpk_align_to_map and icpk_align_to_map_dense (they run icpk_align's loop);
 * icpk_align_batch / _device (the pairs run one by one, each equal to icpk_align).  icpk_align_frames_batch and
 * icpk_align_query_sharded: ICPK_E_ARG while it is on. */
#define ICPK_ROBUST_NONE  0   /* w = 1                                          */
#define ICPK_ROBUST_HUBER 1   /* w = d <= c ? 1 : c / d                         */
#define ICPK_ROBUST_TUKEY 2   /* w = d == 0 ? 1 : d < c ? (1 - (d/c)^2)^2 : 0   */
#define ICPK_SCALE_FIXED  0   /* c = scale (metres)                             */
#define ICPK_SCALE_MEDIAN 1   /* c = scale * 1.4826 * m   (m: median above)     */
typedef struct icpk_robust {
  int32_t kernel;       /* ICPK_ROBUST_*                                        */
  int32_t scale_mode;   /* ICPK_SCALE_*                                         */
  float scale;          /* > 0, finite                                          */
  float trim_fraction;  /* (0, 1]: keep the closest share of accepted pairs    */
} icpk_robust;
/* NULL: off (the default).  ICPK_E_ARG for an unknown kernel or scale mode, a non-finite or non-positive scale, or
 * trim_fraction outside (0, 1]; the setting is then left as it was. */
int icpk_set_robust(icpk_ctx *ctx, const icpk_robust *r);
/* Per iteration i < *n_iter of the last robust icpk_align (as icpk_get_trace): the kept count, the cut tau, the scale
 * c and W = sum w of the sweep the iteration solved from.  *n_iter is icpk_get_trace's: the completed iterations -- an
 * iteration that ends in the min_pairs fallback or in ICPK_W_DEGENERATE leaves no entry, in the device and the host
 * loop alike.  *n_iter = 0 after an alignment with robust off.  Arrays
 * sized for params.max_iterations entries; any may be NULL. */
int icpk_get_robust_trace(icpk_ctx *ctx, int32_t *n_iter, int32_t *kept_out, float *cut_out, double *c_out,
                          double *wsum_out);
/* test hook: one robust reduction over the associations of the last icpk_nn (as icpk_reduce / icpk_reduce_p2l) with
 * the context's setting (ICPK_E_NOT_SET while it is off).  solve: ICPK_SOLVE_KABSCH (sums: ICPK_NSUM_W doubles) or
 * ICPK_SOLVE_POINT_TO_PLANE (ICPK_NP2L_W); accepted = n, kept, cut = tau, median = m, c as defined above.  Any
 * output but sums may be NULL. */
int icpk_reduce_weighted(icpk_ctx *ctx, float max_dist, int32_t solve, double *sums, int64_t *accepted, int64_t *kept,
                         float *cut, float *median, double *c);

/* frame-batch mode (the frame-pair formulation of icp.cpp:541-563): n_pairs
 * independent pairs on this context's device; T_out n_pairs x 16, stats n_pairs (or NULL).
 * With the default kernels (ICPK_NN_GRID, device-side loop, reference or Kabsch flavour) up to
 * ICPK_BATCH_GROUP (default and at most 16) pairs advance in lock step -- one launch per stage
 * for the whole group -- while the next group is being uploaded and indexed; every pair's
 * result equals icpk_align on that pair bit for bit.  Other settings run the pairs one after
 * the other.  The context's own clouds are not touched by the lock-step path.  params.profile = 1
 * in this mode: ONE batched NN launch per group (its position rotating) is bracketed by HIP events;
 * the time is booked on the group's first pair (stats.nn_ms_total, nn_timed_launches = 1) and covers
 * ALL pairs of that group.
 * Returns the first negative status, else the max status. */
int icpk_align_batch(icpk_ctx *ctx, int32_t n_pairs, const icpk_pair *pairs,
                     const icpk_params *p, float *T_out, icpk_stats *stats);
/* same with the clouds already resident in HBM (sx..tz are device pointers; copied
 * device-to-device into the slots, so the caller's buffers stay untouched) */
int icpk_align_batch_device(icpk_ctx *ctx, int32_t n_pairs, const icpk_pair *pairs,
                            const icpk_params *p, float *T_out, icpk_stats *stats);

/* ---- multi-GPU: RCCL over xGMI behind the C ABI ------- */
/* One process (or host thread) and one context per GPU.  The path shards over independent
 * frame pairs (frame-pair formulation of icp.cpp:541-563): no per-iteration collective; the
 * collectives are one broadcast of a shared target cloud (key frame) and one all-gather of the
 * results.  librccl.so.1 is opened on first use (dlopen), not linked. */
#define ICPK_COMM_ID_BYTES 128
/* rank 0 makes the id (ncclGetUniqueId) and ships it to the other ranks by the host's own
 * means (socket, file, MPI, torch store) */
int icpk_comm_unique_id(void *id_out /* ICPK_COMM_ID_BYTES */);
int icpk_comm_init_rccl(icpk_ctx *ctx, const void *unique_id, int rank, int world);
int icpk_comm_destroy(icpk_ctx *ctx);
int icpk_comm_rank(const icpk_ctx *ctx);   /* -1 without a communicator */
int icpk_comm_world(const icpk_ctx *ctx);  /*  0 without a communicator */
/* block-wise shard of n_items over world ranks: rank's contiguous [start, start + count) */
void icpk_comm_partition(int32_t n_items, int world, int rank, int32_t *start, int32_t *count);
/* the root's target cloud (icpk_set_target* / icpk_backproject there) becomes the target of
 * every rank: ncclBroadcast of the three planes, 3 * Nt * 4 bytes */
int icpk_comm_broadcast_target(icpk_ctx *ctx, int root);
/* results of a block-partitioned batch of n_total pairs: this rank contributes the n_local
 * rows of its block (T_local n_local x 16, stats_local n_local or NULL) and receives all rows
 * in global pair order: T_all n_total x 16, stats_all n_total x 4 four-byte slots (iterations, status,
 * final_pairs as int32 BIT PATTERNS -- memcpy them out, exact whatever the cloud size -- and final_mse as a
 * float) or NULL.  One ncclAllGather. */
int icpk_comm_gather_results(icpk_ctx *ctx, const float *T_local, const icpk_stats *stats_local,
                             int32_t n_local, int32_t n_total, float *T_all, float *stats_all);
/* query-sharded single pair (SURVEY.md 8e alternative): sums[0..n) and *count summed over the
 * ranks in place; one ncclAllReduce of (n + 1) doubles per iteration */
int icpk_comm_allreduce_sums(icpk_ctx *ctx, double *sums, int32_t n, int64_t *count);
int icpk_comm_barrier(icpk_ctx *ctx);
/* Query-sharded alignment of ONE pair over the communicator's ranks (SURVEY.md 8e alternative; the frame-pair
 * formulation icp.cpp:541-563 with the queries split): same target on every rank (icpk_comm_broadcast_target),
 * source = this rank's slice of the queries; collective call.  The whole loop is enqueued: per iteration the grid
 * sweep and the reduction on the slice, then ONE in-stream ncclAllReduce of 20 doubles (19 sums + pair count) and
 * the replicated loop step on the reduced sums -- no host round trip per iteration.  reference and Kabsch
 * flavours.  Every rank returns the same T and statistics (final_pairs = all ranks' pairs); they agree with
 * icpk_align on the whole pair to ~1e-6 (the ranks' sums are added in the collective's order), bit for bit
 * with one rank. */
int icpk_align_query_sharded(icpk_ctx *ctx, const icpk_params *p, float T_out[16], icpk_stats *stats);

/* ---- front end -------------------------------------- */
/* pointcloud.cpp:27-30: the reference keeps one valid pixel in SUBSAMPLE_FACTOR, chosen by an unseeded rand().
 * factor > 1: every back-projection of this context (icpk_backproject*, both images of icpk_backproject_pair --
 * the source first, then the target, as icp.cpp:38-39 builds them; a resident previous frame draws a fresh
 * pattern too, as the reference's rebuilt cloud does) keeps a valid pixel p iff
 *   z = seed + (k + 1) * 0x9E3779B97F4A7C15 + p * 0xD1B54A32D192ED03          (k = images since this call, mod 2^64)
 *   z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^= z >> 31
 *   (uint32)(z >> 32) % factor == 0
 * -- reproducible, unlike rand(); the stream of the reference's C library is not pinned by anything it ships.
 * factor 0 or 1 (the default): every valid pixel.  Resets k to 0. */
/* Optional, for callers whose frames live in long-lived buffers (a camera driver's ring, a reused cv::Mat): pins
 * [ptr, ptr + bytes) and maps it for the device (hipHostRegister).  icpk_backproject_pair then reads a depth image that
 * lies inside a registered range where it is -- no staging copy, no transfer command; the image has been consumed
 * when the call returns, as always.  The memory must stay allocated until icpk_unregister_host_buffer (or
 * icpk_destroy).  Not needed for correctness; results are the same. */
int icpk_register_host_buffer(icpk_ctx *ctx, const void *ptr, size_t bytes);
int icpk_unregister_host_buffer(icpk_ctx *ctx, const void *ptr);

#define ICPK_SUBSAMPLE_FACTOR 40 /* pointcloud.hpp:11 */
int icpk_set_subsample(icpk_ctx *ctx, int32_t factor, uint64_t seed);

/* pointcloud.cpp:19-58 (the subsample of :27-30 as set by icpk_set_subsample; none by default): row-major back-
 * projection of a rows x cols uint16 depth image (host pointer) into the
 * source (which = 0) or target (which = 1) cloud, adding `offset` to every
 * coordinate afterwards (PointCloud::translate(cameraPosition), icp.cpp:71).
 * Returns the number of points (>= 0) or a negative status. */
int icpk_backproject(icpk_ctx *ctx, const uint16_t *depth, int32_t rows, int32_t cols,
                     float fx, float cx, const float offset[3], int32_t which);

/* SLAM.cpp:553-574 filterDepthImage on the device: every value outside [min_d, max_d] -> 0
 * (:558-566; SLAM.cpp:229 passes 25000 / 1000, SLAM.hpp:15-16), then, if morph != 0, cv::dilate and
 * cv::erode with the 5x5 rectangle of :568-573 in one LDS-tiled pass.  anchor_x / anchor_y: the
 * anchor of dilate / erode inside the element, -1 = its centre (2, 2) -- what OpenCV uses when,
 * as at :572-573, no anchor is passed (the Point(3,3) handed to getStructuringElement only shapes
 * MORPH_CROSS elements).  OpenCV is third-party and absent here: anchor and border rule
 * (out-of-image pixels never win) are PARITY UNPINNED, restated from its documentation.
 * depth_in / depth_out: host arrays of rows x cols (may be the same array). */
int icpk_filter_depth_image(icpk_ctx *ctx, const uint16_t *depth_in, uint16_t *depth_out, int32_t rows,
                            int32_t cols, int32_t max_d, int32_t min_d, int32_t morph, int32_t anchor_x,
                            int32_t anchor_y);
/* filterDepthImage + back-projection without the image leaving the device (SLAM.cpp:229 then
 * icp.cpp:38-39): as icpk_backproject (normals_mode < 0) or icpk_backproject_with_normals
 * (normals_mode >= 0, which must be 1) on the filtered image */
int icpk_backproject_filtered(icpk_ctx *ctx, const uint16_t *depth, int32_t rows, int32_t cols, float fx,
                              float cx, const float offset[3], int32_t which, int32_t normals_mode,
                              int32_t max_d, int32_t min_d, int32_t morph, int32_t anchor_x, int32_t anchor_y);

/* The cloud set-up of icp::getTransformation for one frame pair in ONE call (icp.cpp:38-39 back-project
 * `data` and `previous`, :58-59 / :70-71 rotate both by cameraRotation and translate by cameraPosition):
 * depth_source = the current frame, depth_target = the previous one; offset as in icpk_backproject;
 * R, t (both or neither) = the pose applied to every point afterwards, p <- fl32(fl32(R p) + t); filter != 0
 * runs icpk_filter_depth_image's filter (max_d ... anchor_y) on both frames first.  Equivalent, bit for bit,
 * to icpk_backproject[_filtered] x 2 + icpk_transform_target + icpk_transform_source + icpk_commit_source
 * (the posed source is the starting point of the alignment), with 3-5 kernel launches instead of 25
 * and one host wait instead of two.  *n_source / *n_target: the cloud sizes.
 * depth_target == NULL: the previous frame is the one this context received as depth_source in its last
 * icpk_backproject_pair call (SLAM.cpp:305, previous = filtered.clone(): the caller hands the same frame back) --
 * its image, and its filtered copy if the filter settings are unchanged, are still on the device, so only ONE
 * image crosses PCIe.  Same results as passing the frame again.  ICPK_E_NOT_SET if no frame of this size is
 * resident (first call, other rows / cols, or the image buffers were used by another call in between). */
int icpk_backproject_pair(icpk_ctx *ctx, const uint16_t *depth_source, const uint16_t *depth_target,
                          int32_t rows, int32_t cols, float fx, float cx, const float offset[3],
                          const float R[9], const float t[3], int32_t filter, int32_t max_d, int32_t min_d,
                          int32_t morph, int32_t anchor_x, int32_t anchor_y, int32_t *n_source,
                          int32_t *n_target);

/* ---- many depth streams in lock step: icpk_backproject_pair + icpk_align for N independent streams ---------------
 * One job = one stream's next frame pair (icp.cpp:38-71 then :98-268).  Job k's T_out[16 k ..], stats[k] and
 * icpk_get_frames_trace(ctx, k, ...) equal, bit for bit, what icpk_backproject_pair(depth_source, depth_target, rows,
 * cols, fx, cx, offset, R, t, filter, max_d ... anchor_y) followed by icpk_align with *p -- last_rotation /
 * last_translation taken from the job -- return on a context whose resident frame is the stream's previous frame.
 * The jobs advance ICPK_BATCH_GROUP (at most 16) at a time: one launch per stage for the whole group, back-projection
 * included (as icpk_align_batch).
 *   - stream: 0 <= stream < ICPK_MAX_FRAME_STREAMS, distinct within a call (else ICPK_E_ARG, nothing runs).  Every
 *     stream named in a call keeps its depth_source (and its filtered copy) on the device as its new resident frame;
 *     streams not named, the context's own clouds and its icpk_backproject_pair frame are not touched.
 *   - depth_target == NULL: the stream's resident frame.  A job whose stream has none of this rows x cols gets
 *     stats[k].status = ICPK_E_NOT_SET and does not stop the others.
 *   - p: ICPK_NN_GRID, the device-side loop (host_loop = 0), reference or Kabsch flavour, no log callback: anything
 *     else is ICPK_E_ARG (there is no one-by-one fallback).
 *   - the depth buffers are host memory and may be reused as soon as the call returns.
 *   - icpk_set_subsample: stream s draws its patterns as a context of its own would that had the same
 *     icpk_set_subsample and made only this stream's icpk_backproject_pair calls -- the image counter k of the key
 *     counts this stream's images (source, then target, per job) since icpk_set_subsample.
 * Returns the first negative job status, else the largest. */
#define ICPK_MAX_FRAME_STREAMS 256
typedef struct icpk_frame_job {
  int32_t stream;
  const uint16_t *depth_source;  /* current frame (host)                                          */
  const uint16_t *depth_target;  /* previous frame (host), or NULL: the stream's resident frame   */
  float R[9], t[3];              /* camera pose applied to both clouds (icp.cpp:58-59, 70-71)     */
  float last_rotation[9], last_translation[3]; /* this stream's icpk_params fields (icp.cpp:23-25, 176-177) */
} icpk_frame_job;
int icpk_align_frames_batch(icpk_ctx *ctx, int32_t n_jobs, const icpk_frame_job *jobs, int32_t rows,
                            int32_t cols, float fx, float cx, const float offset[3], int32_t filter,
                            int32_t max_d, int32_t min_d, int32_t morph, int32_t anchor_x, int32_t anchor_y,
                            const icpk_params *p, float *T_out /* 16 x n_jobs */, icpk_stats *stats /* n_jobs or NULL */);
/* icpk_get_trace of job `job` of the last icpk_align_frames_batch call (ICPK_E_ARG outside it) */
int icpk_get_frames_trace(icpk_ctx *ctx, int32_t job, int32_t *n_iter, float *R_out, float *t_out,
                          int32_t *pairs_out, float *mse_out);
/* frees every stream's resident images (the next job of any stream must pass depth_target) */
int icpk_release_frame_streams(icpk_ctx *ctx);

/* ---- voxel certainty map: map::Map (map.hpp, map.cpp) on the device ------- */
/* One map per context, allocated on first use: a 300^3 uint8 certainty grid (`world`, map.hpp:25; 27 MB) and an int32
 * slot per voxel (`pointLookupTable`, map.hpp:24; 108 MB) that holds (list index << 1) | list of the point that filled
 * it, -1 while empty.  Two point lists grow on the device: the key points (mapCloud.keypoints) and the points
 * (mapCloud.points).  Storage order of the grid is world[x][y][z]: offset (x * 300 + y) * 300 + z.
 * Empty slot: the reference compares the slot with a default color_point_t (zero point, black) and this library drops
 * colour, so a slot here is empty until a point fills it.  The two differ only for a point at exactly (0, 0, 0), which
 * the reference would treat as never filling its slot: PARITY UNPINNED there.  Slots persist across updates and are
 * shared by both lists; they keep their (list, index) when icpk_map_set_points replaces the point list. */
#define ICPK_MAP_HEIGHT 300          /* map.hpp:9  MAP_HEIGHT                                   */
#define ICPK_MAP_PHYSICAL_HEIGHT 10.0f /* map.hpp:10 PHYSICAL_HEIGHT (cell c = float(10 / 300)) */
#define ICPK_MAP_MAX_CONFIDENCE 180  /* map.hpp:13                                               */
#define ICPK_MAP_DELTA_CONFIDENCE 25 /* map.hpp:11                                               */
#define ICPK_MAP_CELLS (ICPK_MAP_HEIGHT * ICPK_MAP_HEIGHT * ICPK_MAP_HEIGHT)
/* lists */
#define ICPK_MAP_KEYPOINTS 0 /* mapCloud.keypoints */
#define ICPK_MAP_POINTS 1    /* mapCloud.points    */
/* the cloud of the context an update reads */
#define ICPK_MAP_FROM_SOURCE 0 /* the working source, as icpk_get_source returns it */
#define ICPK_MAP_FROM_TARGET 1 /* the target, as icpk_get_target returns it         */
/* update rules; per point, in input order (d = delta, 1 <= d <= 255; cert = the voxel's certainty):
 *   ADD_CLOUD         map.cpp:220-269 (icp.cpp:62):  cert = min(255, cert + d); then if the slot is empty and
 *                     cert >= 180, fill it and append the point to the KEY-POINT list
 *   ADD_ASSOCIATED    map.cpp:88-119:  if cert > 255 - d: cert = 255 and, if the slot is empty, fill it and append
 *                     the point to the POINT list; else cert += d
 *   ADD_UNASSOCIATED  map.cpp:122-206 (icp.cpp:271):  if cert >= 180 - d: cert = 255 and, if the slot is empty, fill
 *                     it and append the point to the KEY-POINT list; else cert += d
 * A batch leaves grid, slots and lists exactly as applying its points one by one in index order would, however many
 * of them share a voxel. */
#define ICPK_MAP_ADD_CLOUD 0
#define ICPK_MAP_ADD_ASSOCIATED 1
#define ICPK_MAP_ADD_UNASSOCIATED 2

/* map.cpp:17-31 Map::Map(): certainty 0, every slot empty, both lists empty (allocates the map on first use) */
int icpk_map_reset(icpk_ctx *ctx);
/* frees the map's device memory (the next map call starts from an empty map) */
int icpk_map_release(icpk_ctx *ctx);
/* the points of the context's source or target (ICPK_MAP_FROM_*) through `rule` with delta d, read where they lie.
 * indices: host list of n point indices (repeats allowed, applied in order); NULL: the whole cloud in order (n is then
 * ignored).  ICPK_E_ARG for a bad rule, d outside [1, 255] or an index outside the cloud. */
int icpk_map_update(icpk_ctx *ctx, int32_t rule, int32_t from, const int32_t *indices, int32_t n, int32_t delta);
/* same for n points in host arrays */
int icpk_map_update_points(icpk_ctx *ctx, int32_t rule, const float *x, const float *y, const float *z, int32_t n,
                           int32_t delta);
/* icp.cpp:63 map.mapCloud.points = previousCloud.points: the point list becomes a copy of the context's source or
 * target (device-to-device).  Grid and slots are not touched. */
int icpk_map_set_points(icpk_ctx *ctx, int32_t from);
/* length of a list (ICPK_MAP_KEYPOINTS / ICPK_MAP_POINTS); 0 before the map exists, negative on a bad argument */
int32_t icpk_map_size(icpk_ctx *ctx, int32_t list);
/* a list to host arrays of icpk_map_size(list) entries, in list order */
int icpk_map_get_list(icpk_ctx *ctx, int32_t list, float *x, float *y, float *z);
/* the whole certainty grid (ICPK_MAP_CELLS bytes, world[x][y][z] order) to host memory */
int icpk_map_get_certainty(icpk_ctx *ctx, uint8_t *out);
/* per point of n host points: the certainty of its voxel, isOccupied (map.cpp:441-444: cert >= 180), and the slot's
 * list and index (-1, -1: empty).  Any output may be NULL. */
int icpk_map_query(icpk_ctx *ctx, const float *x, const float *y, const float *z, int32_t n, uint8_t *cert_out,
                   uint8_t *occupied_out, int32_t *slot_list_out, int32_t *slot_index_out);
/* a list becomes the context's target (device-to-device), ready for icpk_nn, icpk_associate_keypoints and icpk_align */
int icpk_map_list_to_target(icpk_ctx *ctx, int32_t list);
/* map.cpp:55-85 getVoxelCoordinates on the host: per axis q = p / c (float), i = int(q) with the x86 conversion
 * (NaN, +-inf and |q| >= 2^31 give INT_MIN), clamped to [0, 299] */
void icpk_map_voxel(const float p[3], int32_t v[3]);
/* The live body of icp::getTransformation (icp.cpp:98-271) against the map:
 *   source = the context's source (the frame's posed key points); target = the map's key-point list, copied
 *   device-to-device: THE CONTEXT'S TARGET IS REPLACED.  The loop is icpk_align's with p->max_nn_dist as the
 *   acceptance (the reference's MAX_NN_KEYPOINT_DISTANCE, 0.1): T_out, stats, icpk_get_trace and the aligned source are
 *   those of icpk_align on the same two clouds, bit for bit.  Every association sweep the loop ran (the initial one,
 *   :98, and one per completed iteration, :255; none after the min_pairs fallback, :163-182) contributes its rejected
 *   source points, at their positions in that sweep, to one list (`nonAssociations`, never cleared within the call,
 *   :507-509); then, if the last sweep accepted at least one pair (map.cpp:124-126), that list goes through
 *   ICPK_MAP_ADD_UNASSOCIATED with `delta` (:271).
 * Empty key-point list: returns ICPK_W_EMPTY_MAP with identity T_out, no iteration, the working source reset to the
 * uploaded one and the map untouched -- what the reference gives: findGlobalKeyPointAssociations returns at
 * :490-491, meanSquareError of no errors is 0 (:622-638) so the loop does not run, and map.update returns on no
 * associations.  Reference and Kabsch flavours (ICPK_E_ARG for point-to-plane: the map has no normals). */
int icpk_align_to_map(icpk_ctx *ctx, const icpk_params *p, int32_t delta, float T_out[16], icpk_stats *stats);

/* ---- mapped nearest neighbours (K9): icp.cpp:347-486 over the device map -----------------------------------------
 * getNearestMappedPoint for a query q, restated exactly; c = float(10 / 300), the voxel rule of icpk_map_voxel:
 *   constants  maxRadius = int(1.5f / c) = 44 (1.5f / c is 44.999996): radii 1 .. 43; the walk starts from
 *              shortest = 0.75f (MAX_NN_COLOR_DISTANCE) and stops below 0.2f (MIN_NN_COLOR_DISTANCE); the distance is
 *              icp.cpp:606-620 with colour weight 0 (double sum of squares, correctly rounded float sqrt)
 *   centre     voxel v = (vx, vy, vz) of q is processed; if then shortest < 0.75 the walk ends (even at >= 0.2)
 *   shells     for r = 1, 2, ... while shortest >= 0.2 and r < 44, in this order:
 *              block 1  for y in [vy-r, vy+r), z in [vz-r, vz+r): (vx-r, y, z) then (vx+r, y, z); the step is skipped
 *                       if vx-r or vx+r lies outside [0, 300) or y does -- z is NOT checked (icp.cpp tests y twice)
 *              block 2  for x in [vx-r+1, vx+r-1), z in [vz-r, vz+r): (x, vy-r, z) then (x, vy+r, z); skipped if x or
 *                       z lies outside [0, 300) or either of vy-r, vy+r does
 *              block 3  for x in [vx-r+1, vx+r-1), y in [vy-r+1, vy+r-1): (x, y, vz-r) then (x, y, vz+r); skipped if
 *                       x or y lies outside [0, 300) or either of vz-r, vz+r does
 *              (half-open ranges: shells are incomplete and asymmetric, as in the reference)
 *   voxel      processVoxel (:476-486): a filled slot yields the point it names, read from its list as the list stands
 *              now; an EMPTY slot yields the zero point (0, 0, 0) -- the reference's emptiness test compares a uchar
 *              with -1 and is always true.  A candidate replaces the best only if d < shortest: the earliest voxel in
 *              visit order wins ties.
 *   overrun    block 1 reads pointLookupTable[x][y][z] with z outside [0, 300) at flat offset (x*300 + y)*300 + z --
 *              another voxel -- as the reference's x86 build does.  Where that offset leaves the table (x = y = 0,
 *              z < 0; x = y = 299, z >= 300) the reference reads memory outside it: such reads are skipped here,
 *              PARITY UNPINNED.
 * Slots name (list, index) (K7); the reference copied the point into the table when it filled the slot.  The two agree
 * unless icpk_map_set_points replaces the point list after ADD_ASSOCIATED has filled slots (the reference assigns it
 * only at the seed, before any such slot exists): the slots then name entries of the new list, and one whose index is
 * past the new list's end reads as empty -- PARITY UNPINNED.  A map never allocated behaves as an empty one. */
#define ICPK_MAP_NN_EMPTY (-1) /* an empty voxel's zero point won                     */
#define ICPK_MAP_NN_NONE (-2)  /* nothing beat 0.75: dist 0.75f                       */
/* getNearestMappedPoint for n host points: per point the distance (0.75f when nothing beat it), the list
 * (ICPK_MAP_KEYPOINTS / ICPK_MAP_POINTS / ICPK_MAP_NN_EMPTY / ICPK_MAP_NN_NONE) and the list index (-1 for the last
 * two).  Any output may be NULL. */
int icpk_map_nearest(icpk_ctx *ctx, const float *x, const float *y, const float *z, int32_t n, float *dist_out,
                     int32_t *list_out, int32_t *index_out);
/* the context's target becomes [key-point list | point list | (0, 0, 0)] (device to device), marked as the lookup
 * target of the map as it stands: icpk_nn, icpk_align and icpk_associate_keypoints accept ICPK_NN_MAP while no map
 * change and no other target has come in between (else ICPK_E_ARG).  An ICPK_NN_MAP sweep's index is the element of
 * this target the walk found; an empty voxel's win and "nothing" both point at the zero point, the latter with
 * d = 0.75f (never accepted: ICPK_NN_MAP needs max_nn_dist <= 0.75).  The loop runs K3 unfused, as for
 * ICPK_NN_EXACT.  Point-to-plane, max_nn_dist > 0.75, icpk_align_batch* and icpk_align_query_sharded: ICPK_E_ARG. */
int icpk_map_lookup_to_target(icpk_ctx *ctx);
/* icp::getTransformation with the mapped association (icp.cpp:155-257 with :150 and :254 enabled): the lookup target,
 * then icpk_align with ICPK_NN_MAP (T_out, stats, trace and aligned source are icpk_align's).  Then, if delta > 0, the
 * data points the LAST sweep accepted (d < p->max_nn_dist, :363), at the positions that sweep saw -- after a min_pairs
 * fallback not the returned source -- go through ICPK_MAP_ADD_ASSOCIATED with delta, in source order (map.cpp:88-119);
 * delta 0 leaves the map alone.  No special case for an empty map (the reference's dense path has no early return).
 * Reference and Kabsch flavours, max_nn_dist <= 0.75 (else ICPK_E_ARG).  THE CONTEXT'S TARGET IS REPLACED. */
int icpk_align_to_map_dense(icpk_ctx *ctx, const icpk_params *p, int32_t delta, float T_out[16], icpk_stats *stats);

/* ---- FAST key points on the device (K8): SLAM.cpp:255-256 + pointcloud.cpp:60-98 -------------------------------
 * cv::cvtColor(BGR -> GRAY) then cv::FAST(gray, keypoints, threshold, nonmax, type), restated from OpenCV 3.2's scalar
 * FAST_t (parity with OpenCV itself is UNPINNED: no OpenCV build is available to compare with).
 *   grey     Y = (1868 B + 9617 G + 4899 R + 8192) >> 14 (8-bit BGR, interleaved, row-major)
 *   corners  pixels with 3 <= y <= rows - 4, 3 <= x <= cols - 4; threshold clamped to [0, 255]; OpenCV's quick test on
 *            circle positions (0,8), (2,10), (4,12), (6,14), then (1,9) ... (7,15) of the wrapped table (for 7_12 this
 *            rejects some pixels with a qualifying arc), then more than P/2 consecutive darker / brighter pixels
 *   score    M - 1, M = the largest over the P arcs of P/2 + 1 circle pixels of max(min(v - x), min(x - v))
 *   nonmax   kept if its score is strictly greater than the score of each of its 8 neighbours (non-corners score 0);
 *            without suppression every corner is kept with response 0
 *   order    row-major (y ascending, then x), key point = (x, y) as floats */
#define ICPK_FAST_TYPE_5_8 0 /* out of scope: ICPK_E_ARG */
#define ICPK_FAST_TYPE_7_12 1
#define ICPK_FAST_TYPE_9_16 2
/* test hook: the grey conversion alone on the device; bgr: rows x cols x 3 bytes, gray_out: rows x cols bytes */
int icpk_bgr_to_gray(icpk_ctx *ctx, const uint8_t *bgr, int32_t rows, int32_t cols, uint8_t *gray_out);
/* FAST on a host image (channels 3: BGR, converted to grey first; 1: grey).  The key points stay on the device as the
 * context's detected list (input of icpk_detected_to_cloud).  kp_xy (2 floats per key point) and response may be NULL;
 * otherwise at most `capacity` entries are written.  *n_out (may be NULL) = the full count.  ICPK_E_ARG for a bad type,
 * channel count, size or a NULL image; an image with fewer than 7 rows or columns has no key points. */
int icpk_detect_fast(icpk_ctx *ctx, const uint8_t *image, int32_t rows, int32_t cols, int32_t channels,
                     int32_t threshold, int32_t nonmax, int32_t type, int32_t capacity, float *kp_xy, float *response,
                     int32_t *n_out);
/* The detected list back-projected from a depth image (d_rows x d_cols CV_16UC1, may differ in size from the colour
 * image) by icpk_backproject_keypoints's rule, posed by p <- fl32(fl32(R p) + t) (K3's arithmetic), and made the
 * context's source (which = 0) or target (which = 1), all on the device with one host wait.  Equivalent, bit for bit,
 * to icpk_backproject_keypoints on the detected list, the pose on the host, then icpk_set_source / icpk_set_target.
 * *n_out (may be NULL) = the number of points.  ICPK_E_NOT_SET before the first icpk_detect_fast. */
int icpk_detected_to_cloud(icpk_ctx *ctx, const uint16_t *depth, int32_t d_rows, int32_t d_cols, float fx, float cx,
                           const float R[9], const float t[3], int32_t which, int32_t *n_out);

/* ---- point-to-plane extension (BASELINE config 3; not in the reference) ---- */
#define ICPK_NORMALS_CROSS 0     /* normalised cross product of back-projected central differences */
#define ICPK_NORMALS_REFERENCE 1 /* SLAM.cpp:421-425 getNormalMap formula, interior pixels          */
/* target cloud AND one normal per point from a depth image (as icpk_backproject
 * with which = 1); pixels without a normal get (0,0,0) and never pair. */
int icpk_backproject_with_normals(icpk_ctx *ctx, const uint16_t *depth, int32_t rows, int32_t cols,
                                  float fx, float cx, const float offset[3], int32_t normals_mode);
/* normals for the current target cloud from host arrays (n must equal the target size) */
int icpk_set_target_normals(icpk_ctx *ctx, const float *nx, const float *ny, const float *nz, int32_t n);
int icpk_get_target_normals(icpk_ctx *ctx, float *nx, float *ny, float *nz);
/* K5: the 28 canonical sums of the linearised point-to-plane step over the
 * associations of the last sweep (see ICPK_NP2L) */
int icpk_reduce_p2l(icpk_ctx *ctx, float max_dist, double *sums, int64_t *count);
/* host solve of the step: 0 ok, ICPK_W_DEGENERATE if not positive definite */
int icpk_solve_point_to_plane(const double sums[28], double R[9], double t[3]);

/* ---- voxel-grid downsampling (K11; extension: the reference plans it, TODO:3 "subsample points better - Grid") ----
 * Replaces one of the context's clouds by one point per occupied cube of edge `leaf`.  Unlike icpk_set_subsample it
 * works on any cloud the context holds, however it got there, and thins by space, not by pixel.  The rule, with
 * L = (double)leaf and float64 arithmetic throughout; the n input points are taken in index order:
 *   voxel     per axis u = (double)p / L, v = floor(u); the point's voxel is (vx, vy, vz).  A point with a non-finite
 *             coordinate, or with |v| > 2^20 on any axis, is DROPPED: it belongs to no voxel (n_dropped counts them)
 *   order     voxels are ordered by the lowest input index among their members; output point k belongs to the k-th
 *             voxel in that order (so the output keeps the input's order, image order included)
 *   FIRST     output k = the member with the lowest input index, its three floats unchanged
 *   CENTROID  per axis f = u - v (exact, in [0, 1)), q = (int64)rint(f * 2^30) (ties to even), S = the sum of q over
 *             the members (exact, int64), m = the member count:
 *               output coordinate = (float)(((double)v + ((double)S / (double)m) / 2^30) * L)
 *             The sum is an integer so that it does not depend on the order in which the members arrive: the same
 *             bits on every run.  Against the float64 mean of the members a coordinate moves by at most leaf * 2^-30
 *             plus the rounding to float.
 *   normals   (which = 1 and the context holds target normals; their components are finite) FIRST: the
 *             representative's normal unchanged.  CENTROID: per component N = the sum over the members of
 *             (int64)rint((double)n_c * 2^30); g = sqrt(Nx^2 + Ny^2 + Nz^2) in float64; the output normal is
 *             (float)(N_c / g), or (0, 0, 0) when g == 0 (such a point never pairs)
 * An empty cloud gives an empty cloud; if every point is dropped the cloud becomes empty (the next alignment reports
 * what it reports for an empty source or target).
 * After the call the downsampled cloud IS the context's cloud, as after icpk_set_source_device / icpk_set_target_device
 * on the result: for the source it is both the uploaded and the working source; for the target the normals, if any,
 * are replaced by the downsampled ones; everything derived from the old cloud is dropped (associations, seeds, the
 * target's indexes; ICPK_NN_MAP needs a new icpk_map_lookup_to_target).  One host wait (the two counts).
 * Where it does not apply: nothing downsamples inside icpk_backproject*, icpk_align_batch / _device or
 * icpk_align_frames_batch (their clouds never become the context's own between back-projection and loop). */
#define ICPK_VOXEL_FIRST 0
#define ICPK_VOXEL_CENTROID 1
/* which: 0 = the working source (as icpk_get_source returns it), 1 = the target (as icpk_get_target returns it).
 * n_out / n_dropped: either may be NULL.  ICPK_E_ARG for another `which` or mode, or a leaf that is not finite and
 * > 0 (nothing changes); ICPK_E_NOT_SET if that cloud has not been set. */
int icpk_voxel_downsample(icpk_ctx *ctx, int32_t which, float leaf, int32_t mode, int32_t *n_out, int32_t *n_dropped);
/* The grouping of the last icpk_voxel_downsample on this context (it stays on the device until asked for):
 *   first_index[n_out], count[n_out]   per output point: lowest member index, member count
 *   out_of_point[n_in]                 per input point: the output point of its voxel, -1 if dropped
 * Any may be NULL; ICPK_E_NOT_SET before the first call. */
int icpk_get_voxel_groups(icpk_ctx *ctx, int32_t *n_in, int32_t *n_out, int32_t *first_index, int32_t *count,
                          int32_t *out_of_point);

/* ---- target normals from the target's own geometry (K12; extension: the reference plans it, TODO:9 "Look into Point
 * to Plane") ----
 * ICPK_SOLVE_POINT_TO_PLANE needs one normal per target point.  icpk_backproject_with_normals gives them to a cloud
 * that is still a depth image, icpk_set_target_normals takes them from the host; this call computes them on the device
 * for ANY target the context holds (icpk_set_target*, a downsampled one, icpk_map_list_to_target, a broadcast key
 * frame): per point the plane fitted to its neighbours within a radius, oriented towards a viewpoint, written where
 * those two calls write theirs.  The rule, for target points p_0 .. p_{n-1} (floats, as icpk_get_target returns them),
 * r = radius and F = 2^15:
 *   neighbourhood  of i: every j (i itself and duplicates included) with d(i, j) <= r, d the pair distance of
 *                  icp.cpp:606-620 exactly as every NN search here evaluates it (float differences, float64 sum of
 *                  squares, narrowed, correctly rounded float sqrt), `<=` a float compare.  A point with a non-finite
 *                  coordinate is in no neighbourhood and has an empty one.  m_i = its size.
 *   moments        per neighbour and axis u = ((double)p_j - (double)p_i) / (double)r, q = (int64)rint(u * F) (ties to
 *                  even); S_a = sum q_a (3 words), S_ab = sum q_a q_b (6 words, a <= b), all int64.  Integers, so that
 *                  they do not depend on the order in which the neighbours arrive: the same bits on every run and for
 *                  every order of the cloud.  |q| <= F + 1 and m < 2^31, so |S_a| < 2^47 and S_ab < 2^62: nothing
 *                  overflows for any cloud an int32 size can describe.
 *   covariance     float64: C_ab = (double)S_ab - (double)S_a * (double)S_b / (double)m.  The offsets are taken from
 *                  p_i, which lies inside the neighbourhood, so the difference does not cancel catastrophically.
 *   eigen-solve    of the symmetric 3x3 C in float64 on the device (cyclic Jacobi): eigenvalues l0 <= l1 <= l2, unit
 *                  eigenvector e0 of l0
 *   no normal      (0, 0, 0), which never pairs: when m < min_neighbors, when l1 <= 2^-20 * l2 as the device computed
 *                  them (the neighbourhood is a line or a point), or when anything above is not finite
 *   orientation    with a viewpoint v: s = e0 . ((double)v - (double)p_i); s < 0 flips e0.  Without one (NULL), or when
 *                  s == 0: the sign that makes the component of largest magnitude positive (lowest axis on a tie).
 *                  The normal is the three components narrowed to float.
 *   curvature      (float)(l0 / (l0 + l1 + l2)) ("surface variation"), 0 where there is no normal
 * The moments, the counts and hence the m-test are exact; e0, the line test and the curvature carry the rounding of the
 * float64 eigen-solve.
 * Stream-ordered, no host wait.  The search walks the uniform grid ICPK_NN_GRID indexes the target with and builds it
 * if the target has none yet: the alignment that follows finds it built.  Afterwards the context holds target normals
 * exactly as after icpk_set_target_normals (icpk_transform_target rotates them, icpk_voxel_downsample carries them
 * along, icpk_get_target_normals returns them); an empty target gets empty normals.
 * ICPK_E_NOT_SET without a target; ICPK_E_ARG for a radius that is not finite and > 0, min_neighbors < 3 or an unknown
 * flag (nothing changes). */
#define ICPK_NORMALS_KEEP_MOMENTS 1 /* flags: keep the 10 int64 per point for icpk_get_normal_stats */
int icpk_estimate_target_normals(icpk_ctx *ctx, float radius, int32_t min_neighbors, const float viewpoint[3] /* or NULL */,
                                 int32_t flags);
/* What the last icpk_estimate_target_normals found (it stays on the device until asked for; this call waits):
 *   n, n_valid       target points, and how many of them got a normal
 *   count[n]         m_i
 *   curvature[n]
 *   moments[10 * n]  per point i the ten words moments[10 i ..]: m, S_x, S_y, S_z, S_xx, S_xy, S_xz, S_yy, S_yz, S_zz
 * Any may be NULL.  The record belongs to the target it was estimated on: ICPK_E_NOT_SET before the first estimate and
 * after any later change of the target or its normals (a new target -- icpk_tsdf_surface_to_target and
 * icpk_tsdf_raycast_to_target are two: they bring normals of their own and no record --, icpk_transform_target,
 * icpk_voxel_downsample, icpk_set_target_normals); ICPK_E_ARG for `moments` when the estimate ran without
 * ICPK_NORMALS_KEEP_MOMENTS. */
int icpk_get_normal_stats(icpk_ctx *ctx, int32_t *n, int32_t *n_valid, int32_t *count, float *curvature,
                          int64_t *moments);

/* ---- outlier removal (K13; extension: the reference plans it, TODO:16 "Filter points better") ----
 * Removes stray points from one of the context's clouds, whichever way it got there: the statistical filter on the mean
 * distance to the k nearest neighbours, or the radius filter on the neighbour count.  A filter acts on POINTS, once per
 * cloud, before the index, the normals and the loop see them (icpk_set_robust acts on pairs, every iteration).
 * The rule.  Input: the n points of the cloud in index order, as icpk_get_source / icpk_get_target return them.
 * d(i, j) is the pair distance of icp.cpp:606-620 exactly as every NN search here evaluates it (float differences,
 * float64 sum of squares, narrowed, correctly rounded float sqrt) -- the function K12's neighbourhood test uses.
 *   dropped      a point with a non-finite coordinate belongs to no neighbourhood, has none, and is removed (n_dropped
 *                counts them; its statistics read value = 0, kth = 0).  N = the number of finite points.
 *   STATISTICAL  (k, alpha = std_ratio) for finite point i, k' = min(k, N - 1).  Its neighbours are the finite j != i
 *                (by INDEX: a duplicate at the same position is a neighbour at distance 0), ordered by (d(i, j), j).
 *                D_i = the float64 sum of the first k' distances, added in ascending order; mean_i = D_i / k' (float64),
 *                kth_i = the k'-th distance (float).  Both depend only on the multiset of the k' smallest distances, so
 *                ties at the k-th place do not matter.  k' = 0 (N = 1): mean_i = 0, kth_i = 0.
 *                S1 = sum mean_i and S2 = sum mean_i^2 over the points in index order through the canonical reduction
 *                tree (ICPK_RED_THREADS / ICPK_RED_MAX_BLOCKS, the tree of icpk_reduce, with n elements; a dropped point
 *                contributes +0.0 at its index).  mu = S1 / N; variance = max(0, (S2 - S1 * S1 / N) / (N - 1)), 0 when
 *                N < 2; sigma = sqrt(variance); T = mu + (double)alpha * sigma; all float64 (N = 0: mu = sigma = T = 0).
 *                Point i is KEPT iff mean_i <= T.
 *   RADIUS       (r, min_neighbors) m_i = #{ finite j : d(i, j) <= r }, i itself and duplicates included -- K12's
 *                neighbourhood, K12's float `<=`.  Kept iff m_i >= min_neighbors.
 *   output       the kept points in input order, their three floats unchanged; for which = 1 with target normals held,
 *                each kept point's normal unchanged.
 * What is exact: kth_i, mean_i and m_i (hence RADIUS's keep mask) for every order of the cloud; and, for a GIVEN order of
 * the cloud, S1, S2, T and STATISTICAL's keep mask -- the same bits on every run.  S1 / S2 follow the index order: a
 * permuted cloud may move T in its last bits.
 * Afterwards (unless ICPK_FILTER_STATS_ONLY) the filtered cloud IS the context's cloud exactly as after
 * icpk_voxel_downsample: everything derived from the old cloud is dropped (associations, seeds, indexes, K12's statistics
 * record; ICPK_NN_MAP needs a new icpk_map_lookup_to_target).  One host wait (the two counts).  With
 * ICPK_FILTER_STATS_ONLY the cloud, its normals and its index stay as they are; only the statistics record is replaced.
 * An empty cloud gives an empty cloud; if every point is removed the cloud becomes empty (the next alignment reports what
 * it reports for one).  The search walks the uniform grid of ICPK_NN_GRID: for the target the context's own (built if the
 * target has none yet, and found built by the alignment that follows a STATS_ONLY call), for the source one in buffers
 * of the filter's own -- the target's index is not disturbed.
 * Where it does not apply: nothing filters inside icpk_backproject*, icpk_align_batch / _device or
 * icpk_align_frames_batch (their clouds never become the context's own between back-projection and loop). */
#define ICPK_FILTER_STATISTICAL 0
#define ICPK_FILTER_RADIUS 1
#define ICPK_FILTER_MAX_K 64
#define ICPK_FILTER_STATS_ONLY 1 /* flags: compute and keep the statistics, leave the cloud as it is */
typedef struct icpk_outlier_filter {
  int32_t kind;          /* ICPK_FILTER_*                                              */
  int32_t k;             /* STATISTICAL: neighbours per point, 1 .. ICPK_FILTER_MAX_K  */
  float std_ratio;       /* STATISTICAL: alpha >= 0, finite                            */
  float radius;          /* RADIUS: finite, > 0                                        */
  int32_t min_neighbors; /* RADIUS: >= 1                                               */
} icpk_outlier_filter;
/* which: 0 = the working source, 1 = the target (as icpk_voxel_downsample).  n_out / n_dropped: either may be NULL.
 * Only the fields of f->kind are read.  ICPK_E_ARG for another `which`, kind or flag, k outside 1 .. ICPK_FILTER_MAX_K,
 * a negative or non-finite std_ratio, a non-finite or non-positive radius, min_neighbors < 1, a NULL f (nothing
 * changes); ICPK_E_NOT_SET if that cloud has not been set. */
int icpk_remove_outliers(icpk_ctx *ctx, int32_t which, const icpk_outlier_filter *f, int32_t flags, int32_t *n_out,
                         int32_t *n_dropped);
/* What the last icpk_remove_outliers on this context found (it stays on the device until asked for; this call waits):
 *   value[n_in]      STATISTICAL: mean_i; RADIUS: (double)m_i; 0 for a dropped point
 *   kth[n_in]        STATISTICAL: the distance of the k'-th neighbour; RADIUS: not written
 *   out_index[n_in]  the point's position in the filtered cloud, -1 if removed or dropped
 *   summary[4]       STATISTICAL: N, mu, sigma, T; RADIUS: N, 0, 0, min_neighbors
 * Any may be NULL; ICPK_E_NOT_SET before the first call. */
int icpk_get_outlier_stats(icpk_ctx *ctx, int32_t *n_in, int32_t *n_out, double *value, float *kth, int32_t *out_index,
                           double summary[4]);

/* ---- plane-to-plane (generalized) ICP (K14; extension: the estimator of Segal, Haehnel and Thrun, "Generalized-ICP",
 * RSS 2009, as pcl::GeneralizedIterativeClosestPoint and Open3D's registration_generalized_icp offer it) ----
 * ICPK_SOLVE_POINT_TO_PLANE models the target's surface only.  This flavour models both: every point is a sample of a
 * locally planar patch, known well along its normal and badly in the plane, and a pair's residual is weighed by the
 * combined uncertainty of the two patches.  It needs one normal per point of BOTH clouds.
 *
 * Source normals.  They belong to the UPLOADED source -- the cloud icpk_align and icpk_reset_source start from --, are
 * stored in the caller's order and stay as they are under icpk_transform_source, icpk_reset_source and the loop: the
 * step rotates them by the accumulated pose itself.  (0,0,0) means "no normal".
 *   icpk_estimate_source_normals  K12's rule (icpk_estimate_target_normals above), word for word, applied to the
 *       uploaded source: neighbourhood, integer moments with F = 2^15, float64 Jacobi, line test, orientation, (0,0,0)
 *       for no normal.  The search walks a uniform grid over the source in buffers of its own: the target's index is not
 *       disturbed.  Stream-ordered, no host wait.  flags must be 0: there is no statistics record for the source, and
 *       icpk_get_normal_stats stays the target's.  Argument errors as icpk_estimate_target_normals; ICPK_E_NOT_SET
 *       without a source.
 *   icpk_set_source_normals       from host arrays; n must equal the source size (else ICPK_E_ARG)
 *   icpk_get_source_normals       to host arrays of icpk_source_size entries
 *   lifetime   every call that replaces or re-indexes the uploaded source drops them: icpk_set_source*,
 *       icpk_backproject* into the source, icpk_backproject_pair, icpk_detected_to_cloud(which = 0),
 *       icpk_commit_source, and icpk_voxel_downsample / icpk_remove_outliers with which = 0 (unless STATS_ONLY).  The
 *       getter, the hook and the flavour then return ICPK_E_NOT_SET.  Estimate after thinning and filtering.  The calls
 *       that replace the TARGET alone leave them as they are: icpk_set_target*, icpk_map_list_to_target,
 *       icpk_map_lookup_to_target, icpk_comm_broadcast_target, and icpk_tsdf_surface_to_target /
 *       icpk_tsdf_raycast_to_target, whose target comes with its own normals (the flavour can run at once).
 *
 * The setting.  icpk_set_plane_to_plane holds epsilon (the default, 1e-3, is the paper's): the variance a patch is given
 * along its normal when the variance in its plane is 1.  ICPK_E_ARG unless it is finite and in (0, 1]; the setting is
 * then left as it was.
 *
 * The rule, per sweep and per pair (i, j = the nearest target of working source point i, d their NN distance), float64
 * throughout; every product and sum below is one rounded operation, in the association the parentheses show, and none
 * is fused:
 *   inputs     p = working source point i, q = target point j, a = source normal i, b = target normal j, all floats
 *              widened.  R = R_acc, the rotation of the pose the loop has accumulated so far as icpk_align would return
 *              it (the nine floats T_out[0..2], [4..6], [8..10] at that moment; the identity at the first sweep),
 *              widened.  c = 1.0 - (double)epsilon.
 *   m          m_u = (R[3u] a_0 + R[3u+1] a_1) + R[3u+2] a_2, u = 0, 1, 2.  Not renormalised.
 *   S          the sum of the two patches' models C(n) = I - (1 - epsilon) n n^T (= V diag(epsilon, 1, 1) V^T for a unit
 *              normal, I for the zero normal), upper triangle:
 *                g_uv = m_u m_v + b_u b_v;   S_uu = 2.0 - c g_uu;   S_uv = 0.0 - c g_uv  (u < v)
 *   M = S^-1   by the adjugate of the symmetric 3x3 and one determinant:
 *                K_00 = S_11 S_22 - S_12 S_12    K_01 = S_02 S_12 - S_01 S_22    K_02 = S_01 S_12 - S_02 S_11
 *                K_11 = S_00 S_22 - S_02 S_02    K_12 = S_01 S_02 - S_00 S_12    K_22 = S_00 S_11 - S_01 S_01
 *                det = (S_00 K_00 + S_01 K_01) + S_02 K_02;   inv = 1.0 / det;   M_uv = K_uv inv  (M_vu = M_uv)
 *   accepted   iff d < max_nn_dist (the float compare of icp.cpp:553) and det is finite and > 0.  A missing normal does
 *              not reject a pair: a zero normal makes that side isotropic.  The determinant test can only fail for
 *              non-unit normals given from the host.
 *   step       r = p - q (r_u = p_u - q_u), J = [-[p]x | I] (3x6; the motion is x = (rotation vector, translation) and
 *              p + J x its first order).  J is not formed; with
 *                w_u  = (M_u0 r_0 + M_u1 r_1) + M_u2 r_2
 *                B_0c = p_1 M_2c - p_2 M_1c;   B_1c = p_2 M_0c - p_0 M_2c;   B_2c = p_0 M_1c - p_1 M_0c   (B = [p]x M)
 *                A_a0 = p_1 B_a2 - p_2 B_a1;   A_a1 = p_2 B_a0 - p_0 B_a2;   A_a2 = p_0 B_a1 - p_1 B_a0   (A = B [p]x^T)
 *              the pair adds these 28 terms (6 + 9 + 6 entries of J^T M J, 6 of J^T M r, the distance):
 *                [0..5]   A_00 A_01 A_02 B_00 B_01 B_02      [15..17] M_00 M_01 M_02
 *                [6..10]  A_11 A_12 B_10 B_11 B_12           [18..19] M_11 M_12
 *                [11..14] A_22 B_20 B_21 B_22                [20]     M_22
 *                [21..23] p_1 w_2 - p_2 w_1,  p_2 w_0 - p_0 w_2,  p_0 w_1 - p_1 w_0     [24..26] w_0 w_1 w_2
 *                [27]     (double)d
 *              which is the ICPK_NP2L layout: [0..20] the upper triangle of sum J^T M J row-major, [21..26] sum J^T M r,
 *              [27] sum d.  The sums go through the canonical tree (ICPK_RED_THREADS / ICPK_RED_MAX_BLOCKS) over the
 *              source points in index order, a pair that is not accepted adding nothing.
 *   solve      icpk_solve_point_to_plane's, unchanged ((sum J^T M J) x = -(sum J^T M r), Rodrigues); the loop takes the
 *              path it takes for point-to-plane: the motion applied and recorded in float, accumulated in float64,
 *              ICPK_W_DEGENERATE with the transform so far when the 6x6 is not positive definite, min_pairs and the
 *              loop test on the accepted pairs, mse from [27].
 * epsilon = 1 gives M = I/2 exactly and the step of point-to-point least squares; so do zero normals on both sides.
 * Where it applies: icpk_align with ICPK_NN_EXACT / FILTERED / PRUNED / GRID and host_loop 0 and 1 -- every combination
 * returns the same bits.  ICPK_E_NOT_SET without source or target normals.  ICPK_E_ARG with ICPK_NN_MAP, while
 * icpk_set_robust is on (robust weights for this flavour are not implemented), and in icpk_align_batch / _device,
 * icpk_align_frames_batch, icpk_align_query_sharded and icpk_align_to_map*: those clouds carry no normals. */
int icpk_estimate_source_normals(icpk_ctx *ctx, float radius, int32_t min_neighbors, const float viewpoint[3] /* or NULL */,
                                 int32_t flags);
int icpk_set_source_normals(icpk_ctx *ctx, const float *nx, const float *ny, const float *nz, int32_t n);
int icpk_get_source_normals(icpk_ctx *ctx, float *nx, float *ny, float *nz);
int icpk_set_plane_to_plane(icpk_ctx *ctx, float epsilon);
/* test hook: the 28 sums of the rule above and the accepted count over the associations of the last icpk_nn (as
 * icpk_reduce_p2l), with the context's epsilon and the given R_acc (row-major; NULL: the identity) */
int icpk_reduce_plane_to_plane(icpk_ctx *ctx, float max_dist, const float R_acc[9], double sums[28], int64_t *count);

/* ---- colored ICP (K17; extension: the estimator of Park, Zhou and Koltun, "Colored Point Cloud Registration
 * Revisited", ICCV 2017, as Open3D's registration_colored_icp offers it) ----
 * Geometry alone leaves a wall, a floor or a table top free to slide in its plane, and on an exact plane the 6x6 of
 * ICPK_SOLVE_POINT_TO_PLANE is singular (ICPK_W_DEGENERATE at the first step).  A depth camera comes with a colour
 * frame; this setting of the point-to-plane flavour keeps its residual and adds a photometric one along the target's
 * tangent plane.  It needs one intensity per point of both clouds and one intensity gradient per target point.
 *
 * Intensities.  One float in [0, 1] per point; icpk_intensity_from_bgr makes them from n BGR triples as
 * (float)(((double)b + (double)g + (double)r) / 765.0) (host helper, no device work).
 *   icpk_set_target_colors / icpk_set_source_colors   n must equal the cloud's size, every value must be finite and in
 *       [0, 1] (a host scan before the upload; the bound is what keeps the integer sums below from overflowing), else
 *       ICPK_E_ARG and nothing changes; ICPK_E_NOT_SET without that cloud.  Setting the target's drops its gradients.
 *   icpk_get_target_colors / icpk_get_source_colors   to a host array of icpk_target_size / icpk_source_size entries;
 *       ICPK_E_NOT_SET when the cloud has none.
 *   lifetime   the source's belong to the UPLOADED source in the caller's order, as K14's source normals do.  An
 *       intensity does not depend on the pose: both clouds' survive icpk_transform_*, icpk_reset_source,
 *       icpk_commit_source and the loop.  Every call that replaces or re-indexes a cloud drops that cloud's
 *       intensities, and for the target its gradients too: icpk_set_source* / icpk_set_target*, icpk_backproject* and
 *       icpk_detected_to_cloud into that cloud, icpk_backproject_pair (both), icpk_voxel_downsample /
 *       icpk_remove_outliers on it (unless STATS_ONLY), icpk_map_list_to_target, icpk_map_lookup_to_target,
 *       icpk_tsdf_surface_to_target, icpk_tsdf_raycast_to_target and icpk_comm_broadcast_target on every rank but the
 *       root (the root's target is not replaced: it keeps its intensities, gradients and kept sums).  The two TSDF
 *       hand-overs drop the old target's intensities, gradients and kept sums like any new target; from a volume with
 *       ICPK_TSDF_COLOR the new target then holds the volume's intensities (one per handed-over point) and no
 *       gradients: estimate them again.  They are not carried through thinning: gather them on the host by
 *       icpk_get_voxel_groups' first_index or icpk_get_outlier_stats' out_index and set them again.
 *
 * Gradients.  icpk_estimate_target_color_gradients fits, per target point, the intensity of its neighbours as a linear
 * function over its tangent plane.  It needs a target, target normals and target intensities (else ICPK_E_NOT_SET);
 * ICPK_E_ARG for a radius that is not finite and > 0, min_neighbors < 1 or an unknown flag (nothing changes).
 * Stream-ordered, no host wait; it walks the uniform grid ICPK_NN_GRID indexes the target with and builds it if the
 * target has none yet.  The rule for target point i with normal n (floats widened), r = radius, F = 2^15:
 *   usable normal  nn = (n_0 n_0 + n_1 n_1) + n_2 n_2 in float64 lies in [1 - 2^-10, 1 + 2^-10] (false for NaN): the
 *                  zero normal and a grossly non-unit host normal are not usable.
 *   neighbourhood  K12's, word for word: every j with d(i, j) <= r, d the pair distance of icp.cpp:606-620, `<=` a float
 *                  compare, i itself and duplicates included, a non-finite point in none and with none.  m = its size.
 *   per neighbour  (only with a usable normal) float64, one rounded operation per symbol, none fused:
 *                    e_a = (double)p_j,a - (double)p_i,a;   h = (e_0 n_0 + e_1 n_1) + e_2 n_2;   u_a = e_a - h n_a
 *                    q_a = (int64)rint((u_a / r) F);        c = (int64)rint(((double)I_j - (double)I_i) F)
 *   sums           int64: S_ab = sum q_a q_b (a <= b), T_a = sum q_a c; all zero without a usable normal.  With m that is
 *                  ten words per point: m, S_00 S_01 S_02 S_11 S_12 S_22, T_0 T_1 T_2.  |u| <= |e| for a usable normal,
 *                  so |q| <= 2^15 + 2^7 with room to spare, |c| <= 2^15 because the intensities lie in [0, 1], and
 *                  m < 2^31: every sum stays below 2^62.  Integers: the same bits on every run and for every order of
 *                  the cloud.
 *   solve          float64: w = (double)m F, w2 = w w, H_ab = (double)S_ab + (w2 n_a) n_b -- the reference method's extra
 *                  row that pins the component along the normal to zero --; the adjugate K of H and det exactly as K14
 *                  writes them for S (K_00 = H_11 H_22 - H_12 H_12, ..., det = (H_00 K_00 + H_01 K_01) + H_02 K_02),
 *                  inv = 1.0 / det, g'_a = ((K_a0 T_0 + K_a1 T_1) + K_a2 T_2) inv, gradient_a = (float)(g'_a / r):
 *                  intensity per metre.
 *   no gradient    (0, 0, 0) when m < min_neighbors, without a usable normal, when det is not finite or <= 0, or when
 *                  a component of the result is not finite.  A zero gradient removes the photometric term of a pair,
 *                  not the pair.
 * icpk_get_target_color_gradients returns them; with the flag ICPK_COLOR_KEEP_SUMS icpk_get_color_gradient_sums returns
 * the ten words per point (10 * n int64; ICPK_E_NOT_SET without the flag, or once the target has changed or moved).
 * icpk_transform_target rotates the gradients as it rotates the normals.  They are those of the normals and
 * intensities they were estimated with: setting the intensities again drops them, changing the normals does not --
 * estimate again.
 *
 * The joint step.  icpk_set_colored(on, lambda_geometric): off by default, lambda_geometric 0.968 (Open3D's value) by
 * default; it must be finite and in [0, 1], else ICPK_E_ARG and the setting stays.  While it is on,
 * ICPK_SOLVE_POINT_TO_PLANE in icpk_align runs the joint step; the other flavours ignore the setting.  Per sweep and
 * pair (i = working source point p, j = its nearest target q with normal n, gradient g and intensity I_t, I_s the
 * intensity of source point i, d the NN distance), float64, unfused, lg = (double)lambda_geometric, lc = 1.0 - lg:
 *   accepted   exactly when point-to-plane accepts the pair: d < max_nn_dist and n != (0, 0, 0)
 *   geometric  e_a = p_a - q_a;  h = (e_0 n_0 + e_1 n_1) + e_2 n_2;  G = [p x n | n]  (p x n = (p_1 n_2 - p_2 n_1,
 *              p_2 n_0 - p_0 n_2, p_0 n_1 - p_1 n_0)): K5's operations and signs
 *   photometric u_a = e_a - h n_a;  rc = (I_t + ((g_0 u_0 + g_1 u_1) + g_2 u_2)) - I_s;
 *              gn = (g_0 n_0 + g_1 n_1) + g_2 n_2;  M_a = g_a - gn n_a;  C = [p x M | M]
 *   sums       ICPK_NP2L's layout through the canonical tree: [0..20] += lg (G_a G_b) + lc (C_a C_b) (a <= b, row-major),
 *              [21..26] += lg (G_a h) + lc (C_a rc), [27] += (double)d
 *   solve      icpk_solve_point_to_plane's; the loop, the trace, min_pairs, ICPK_W_DEGENERATE and final_mse are the
 *              point-to-plane path's, unchanged.
 * lambda_geometric = 1 gives the sums of icpk_reduce_p2l bit for bit.
 * Where it applies: icpk_align with ICPK_NN_EXACT / FILTERED / PRUNED / GRID and host_loop 0 and 1 -- every combination
 * returns the same bits.  While the setting is on and solve is ICPK_SOLVE_POINT_TO_PLANE: ICPK_E_NOT_SET without source
 * intensities, target intensities, target normals or gradients; ICPK_E_ARG with ICPK_NN_MAP and while icpk_set_robust
 * is on.  icpk_align_query_sharded and icpk_align_to_map* refuse point-to-plane as they always did; the batch paths
 * carry no colours and ignore the setting. */
#define ICPK_COLOR_KEEP_SUMS 1 /* flags: keep the 10 int64 per point for icpk_get_color_gradient_sums */
void icpk_intensity_from_bgr(const uint8_t *bgr, int32_t n, float *out);
int icpk_set_target_colors(icpk_ctx *ctx, const float *intensity, int32_t n);
int icpk_set_source_colors(icpk_ctx *ctx, const float *intensity, int32_t n);
int icpk_get_target_colors(icpk_ctx *ctx, float *intensity);
int icpk_get_source_colors(icpk_ctx *ctx, float *intensity);
int icpk_estimate_target_color_gradients(icpk_ctx *ctx, float radius, int32_t min_neighbors, int32_t flags);
int icpk_get_target_color_gradients(icpk_ctx *ctx, float *gx, float *gy, float *gz);
int icpk_get_color_gradient_sums(icpk_ctx *ctx, int64_t *sums);
int icpk_set_colored(icpk_ctx *ctx, int32_t on, float lambda_geometric);
/* test hook: the 28 sums of the joint step and the accepted count over the associations of the last icpk_nn (as
 * icpk_reduce_p2l), with the context's lambda_geometric (whether or not the setting is on) */
int icpk_reduce_colored(icpk_ctx *ctx, float max_dist, double sums[28], int64_t *count);

/* ---- pose scoring (K15; extension: what Open3D's evaluate_registration / GetInformationMatrixFromPointClouds and PCL's
 * getFitnessScore answer) ----
 * How good is a pose?  For every one of n_poses candidate poses: how many source points find a target within max_dist,
 * how far away, and the eleven sums from which fitness, inlier RMSE, mean distance and the 6x6 information matrix of
 * the pair follow.  Many poses are scored in one call (one launch covers poses x source points); the context's state
 * is not touched, and no seeds are needed: a candidate pose may be anywhere.  The rule:
 *   points     for pose k, T_k = T[16 k ..] row-major with R = entries [0..2], [4..6], [8..10] and t = [3], [7], [11]
 *              (row 3 is ignored).  Source point i of the UPLOADED source (the cloud icpk_align and icpk_reset_source
 *              start from) gives p = fl32(fl32(R s) + t): icpk_transform_source's arithmetic, operation for operation.
 *              T == NULL requires n_poses == 1 and scores the WORKING source exactly as it stands (no transform): after
 *              icpk_align this scores the alignment just computed.
 *   partner    the target j that minimises (d, j) lexicographically, d the pair distance of icp.cpp:606-620 exactly as
 *              every NN search here evaluates it (float differences, float64 sum of squares, narrowed, correctly
 *              rounded float sqrt), among the targets with d < max_dist (the float compare of icp.cpp:553).  If there is
 *              none the point is not an inlier.  A non-finite p, or a non-finite target, never pairs.  For an inlier
 *              this is the pair icpk_nn would report for p, bit for bit.
 *   terms      per inlier, with q = target j widened to float64 and dd = (double)d, the ICPK_NSCORE = 11 terms
 *                [0] dd   [1] dd dd   [2..4] q_x q_y q_z   [5..10] q_x q_x, q_x q_y, q_x q_z, q_y q_y, q_y q_z, q_z q_z
 *              each product one rounded operation.  A point that is not an inlier adds +0.0.
 *   sums       per pose each term through the canonical reduction tree (ICPK_RED_THREADS / ICPK_RED_MAX_BLOCKS, the tree
 *              of icpk_reduce) over the source points in index order: sums[ICPK_NSCORE k ..].  inliers[k] is the exact
 *              count.
 *   metrics    (icpk_score_metrics; float64, then narrowed) fitness = inliers / n_source (0 for n_source <= 0);
 *              inlier_rmse = sqrt(sums[1] / inliers); mean_dist = sums[0] / inliers; both 0 with no inliers.
 *   information (icpk_information_matrix; row-major 6x6, order: rotation vector, translation) sum G^T G over the
 *              inliers with G = [-[q]x | I], the matrix Open3D's GetInformationMatrixFromPointClouds forms, assembled
 *              from the sums (Sxx = sums[5] and so on, Sx = sums[2] ...), symmetric:
 *                rotation block              [0][0] = Syy + Szz   [0][1] = -Sxy        [0][2] = -Sxz
 *                                            [1][1] = Sxx + Szz   [1][2] = -Syz        [2][2] = Sxx + Syy
 *                rotation / translation      [0][3] = 0    [0][4] = -Sz  [0][5] = Sy
 *                                            [1][3] = Sz   [1][4] = 0    [1][5] = -Sx
 *                                            [2][3] = -Sy  [2][4] = Sx   [2][5] = 0
 *                translation block           inliers * I
 * What is exact: every partner and distance for any order of the target; inliers; and, for a given order of the
 * source, every sum -- the same bits on every run.
 * The call leaves the working source, the uploaded source, both normals, the associations and the seeds of the last
 * sweep and the target's index exactly as they were.  The search walks the uniform grid of ICPK_NN_GRID and builds it
 * if the target has none yet: the alignment that follows finds it built.  Stream-ordered, one host wait (the results).
 * ICPK_E_ARG (nothing changes) for n_poses outside 1 .. ICPK_SCORE_MAX_POSES, T == NULL with n_poses != 1, a max_dist
 * that is not finite and > 0, an unknown flag, NULL sums or inliers; ICPK_E_NOT_SET without a source or a target; an
 * empty target returns what icpk_nn returns for it; an empty source gives zero sums and zero inliers; a pose with a
 * non-finite entry simply scores zero inliers wherever that entry reaches a point. */
#define ICPK_SCORE_MAX_POSES 4096
#define ICPK_NSCORE 11
#define ICPK_SCORE_KEEP_ASSOC 1 /* flags: keep every pose's (index, distance) for icpk_get_score_associations */
int icpk_score_poses(icpk_ctx *ctx, int32_t n_poses, const float *T /* 16 * n_poses, or NULL */, float max_dist,
                     int32_t flags, double *sums /* ICPK_NSCORE * n_poses */, int64_t *inliers /* n_poses */);
/* Pose `pose` of the last icpk_score_poses made with ICPK_SCORE_KEEP_ASSOC (8 bytes per pose and source point stay on
 * the device until the next such call): per source point the partner's index and distance, -1 and +inf for a point
 * without one.  Either array may be NULL.  ICPK_E_NOT_SET before such a call, or after the uploaded source or the
 * target changed -- every call that replaces or re-indexes one of them: icpk_set_source* / icpk_set_target*,
 * icpk_backproject*, icpk_backproject_pair, icpk_detected_to_cloud, icpk_commit_source, icpk_voxel_downsample /
 * icpk_remove_outliers (unless STATS_ONLY), icpk_transform_target, icpk_map_list_to_target,
 * icpk_map_lookup_to_target, icpk_tsdf_surface_to_target, icpk_tsdf_raycast_to_target, icpk_comm_broadcast_target off
 * the root --; ICPK_E_ARG for a pose outside that call. */
int icpk_get_score_associations(icpk_ctx *ctx, int32_t pose, int32_t *idx_out, float *dist_out);
/* host only (no device work): the metrics and the information matrix of the rule above from one pose's sums; any
 * output of icpk_score_metrics may be NULL */
void icpk_score_metrics(const double sums[ICPK_NSCORE], int64_t inliers, int32_t n_source, float *fitness,
                        float *inlier_rmse, float *mean_dist);
void icpk_information_matrix(const double sums[ICPK_NSCORE], int64_t inliers, double info[36]);

/* ---- global registration (K16; extension: what Open3D's compute_fpfh_feature + registration_ransac_based_on_feature_
 * matching and PCL's FPFHEstimation + SampleConsensusPrerejective answer) ----
 * Every alignment above needs a starting pose inside ICP's basin of convergence.  These calls find one without any:
 * a local shape descriptor per point (FPFH: Rusu, Blodow, Beetz, "Fast Point Feature Histograms (FPFH) for 3D
 * Registration", ICRA 2009), descriptor matching, and a seeded RANSAC whose hypotheses icpk_score_poses (K15) ranks.
 * The rules are this library's own restatement: integer wherever an order could matter, so that every result is the
 * same bits on every run and the bits of the CPU model in tests/fpfh_model.py.
 *
 * 1. icpk_compute_fpfh(ctx, which, radius, flags).  which = 0: the UPLOADED source with its source normals (K14's
 * lifetime rules); which = 1: the target with its target normals.  d(i, j) is the pair distance of icp.cpp:606-620 as
 * every search here evaluates it, a float; "<=" on it is a float compare.  Everything else is float64, every product,
 * sum and quotient one rounded operation, none fused; x . y = (x0 y0 + x1 y1) + x2 y2; x X y = (x1 y2 - x2 y1,
 * x2 y0 - x0 y2, x0 y1 - x1 y0).
 *   described  point i is described iff its coordinates and its normal are finite and the normal is not (0, 0, 0).
 *   stage 1 (SPFH counts, integers)  for a described i and every described j with 0 < d(i, j) <= r:
 *              dp = p_j - p_i (floats widened);  f4 = sqrt((dp0^2 + dp1^2) + dp2^2);  skip if f4 == 0
 *              a1 = (n_i . dp) / f4;  a2 = (n_j . dp) / f4
 *              if |a1| < |a2|: (n1, n2) = (n_j, n_i), dp = -dp, f3 = -a2;  else: (n1, n2) = (n_i, n_j), f3 = a1
 *              v = dp X n1;  vn = sqrt(v . v);  skip if vn == 0;  v = v / vn (per component)
 *              w = n1 X v;  f2 = v . n2;  a = w . n2;  b = n1 . n2
 *              B2 = bin(f2), B3 = bin(f3) with bin(f) = t >= 10 ? 10 : (t >= 1 ? (int)t : 0),
 *                t = floor(11.0 * ((f + 1.0) * 0.5))        (clamp((int)floor(.), 0, 10); NaN gives 0)
 *              B1 = the sector of atan2(a, b) among 11 equal sectors of [-pi, pi], WITHOUT any libm call: with
 *                beta_k = -pi + 2 pi k / 11 and C_k, S_k the doubles nearest cos(beta_k), sin(beta_k) (tabulated as hex
 *                literals in csrc/fpfh_table.h, which the model parses) and e_k = C_k a - S_k b:
 *                  a == 0 and b == 0:  B1 = 5
 *                  else a >= 0:        B1 = 5 + #{k in 6..10 : e_k >= 0}
 *                  else:               B1 = 5 - #{k in 1..5 : e_k < 0}
 *              c_i[B1]++, c_i[11 + B2]++, c_i[22 + B3]++, m_i++
 *   stage 2 (FPFH)  g_j[b] = m_j > 0 ? (c_j[b] * 32768) / m_j : 0  (integer division; <= 32768, 16 bits).
 *              For a described i and every j with 0 < d(i, j) <= r and m_j > 0:
 *                u = ((double)r (double)r) / ((double)d (double)d);  q = (int64)rint(fmin(u, 16384.0) * 1024.0)
 *                A_i[b] += q g_j[b];  Q_i += q        (int64; no overflow below 2^23 neighbours)
 *              raw_b = (double)g_i[b] + (Q_i > 0 ? (double)A_i[b] / (double)Q_i : 0.0)
 *              per sub-histogram (bins 0..10, 11..21, 22..32) tot = the 11 raw values added in bin order;
 *              out_b = tot > 0 ? (float)((100.0 raw_b) / tot) : 0
 *   valid      iff described and m_i > 0.  Every other point gets 33 zeros and is never matched.
 * Deviations from PCL / Open3D: the neighbour weights are r^2 / d^2, capped at 2^14 and normalised by their sum (theirs:
 * 1 / d^2 divided by the neighbour count, which depends on the unit of length); zero-distance neighbours are skipped
 * (theirs divide by zero or special-case them); the histograms are fixed-point (theirs: float accumulation in search
 * order); the sector B1 is decided by signs against tabulated boundaries instead of atan2.
 * The source walks a uniform grid in buffers of its own (K14's), the target the context's grid (ICPK_NN_GRID), built
 * if absent: the alignment that follows finds it built.  Stream-ordered, no host wait.  An empty cloud gives empty
 * descriptors.  ICPK_E_NOT_SET without that cloud or its normals; ICPK_E_ARG for another `which`, a radius that is not
 * finite and > 0, or an unknown flag.
 * icpk_get_fpfh: desc n x ICPK_FPFH_BINS floats in the caller's point order, valid n bytes, *n the count; any may be
 * NULL.  icpk_get_spfh (after ICPK_FPFH_KEEP_SPFH, else ICPK_E_ARG): counts n x 33 and m n int32.  Both wait, and both
 * return ICPK_E_NOT_SET once the cloud or its normals have changed: the events that drop K12's statistics record (target;
 * icpk_tsdf_surface_to_target and icpk_tsdf_raycast_to_target among them: a new target with new normals) and K14's
 * source normals (source).
 *
 * 2. icpk_match_features(ctx, flags).  Both clouds must hold current descriptors (else ICPK_E_NOT_SET).  For every valid
 * source i: the valid target j that minimises (D, j) lexicographically, D = (float)(sum over b = 0..32 in order of
 * ((double)fs_b - (double)ft_b)^2), the sum starting from +0.0.  With ICPK_MATCH_MUTUAL the pair is kept only if i is, by
 * the same rule with the roles exchanged, the best source of j.  The kept pairs, in source order, stay on the device for
 * icpk_register_global; icpk_get_feature_matches (waits; arrays of icpk_source_size entries or NULL) brings them to the
 * host as (src_index, tgt_index, D).  No valid point on one side gives zero pairs, not an error.  Stream-ordered.
 *
 * 3. icpk_register_global(ctx, p, out).  Per hypothesis h = 0 .. n_hypotheses - 1:
 *   draws      d = 0 .. 15:  z = seed + (h + 1) * 0x9E3779B97F4A7C15 + d * 0xD1B54A32D192ED03, then icpk_set_subsample's
 *              finaliser (z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31);
 *              c = (uint32)(z >> 32) % n_matches.  The first three DISTINCT c in draw order are the sample; fewer than
 *              three in 16 draws: the hypothesis is invalid.
 *   edges      for the pairs (0,1), (0,2), (1,2) of the sample: ls, lt = icpk_distance3 of the two source points and of
 *              the two target points; valid iff ls >= e lt and lt >= e ls for all three (float products,
 *              e = edge_similarity).
 *   pose       icpk_solve_kabsch(3, sum a, sum b, sum a b^T) with a the source and b the target points widened, every sum
 *              started at +0.0 and added in sample order (the convention icpk_reduce's Kabsch path feeds the solve: the
 *              pose moves source onto target), narrowed to a row-major float 4x4 with the last row (0, 0, 0, 1).
 *   scoring    the valid hypotheses, in order of h, through icpk_score_poses in chunks of ICPK_SCORE_MAX_POSES at
 *              p->max_dist.  The best pose has the most inliers, then the smallest sums[1], then the lowest h.
 * Fewer than 3 matches, or no valid hypothesis: ICPK_W_TOO_FEW_PAIRS with the identity and hypothesis = -1.
 * ICPK_E_ARG for n_hypotheses outside 1 .. ICPK_GLOBAL_MAX_HYPOTHESES, a max_dist that is not finite and > 0 or an
 * edge_similarity outside [0, 1]; ICPK_E_NOT_SET without current matches.  The call leaves clouds, normals, associations
 * and seeds exactly as icpk_score_poses leaves them; refine with icpk_transform_source(R, t of out->T) + icpk_align.
 * icpk_global_hypotheses is the draw on its own, host only (no device work, no context): hypotheses h0 .. h0 + count - 1
 * over the given matches and point arrays; samples 3 per hypothesis (indices into the matches, -1 where the draws gave
 * none), valid one byte, T 16 floats (the identity unless valid); any output may be NULL. */
#define ICPK_FPFH_BINS 33
#define ICPK_FPFH_KEEP_SPFH 1 /* flags of icpk_compute_fpfh: keep the counts and m for icpk_get_spfh */
#define ICPK_MATCH_MUTUAL 1   /* flags of icpk_match_features */
#define ICPK_GLOBAL_MAX_HYPOTHESES (1 << 20)
typedef struct icpk_global_params {
  uint64_t seed;
  int32_t n_hypotheses;  /* 1 .. ICPK_GLOBAL_MAX_HYPOTHESES */
  float max_dist;        /* the inlier distance of the scoring */
  float edge_similarity; /* in [0, 1]; icpk_default_global_params: 0.9 */
  int32_t reserved;
} icpk_global_params;
typedef struct icpk_global_result {
  float T[16];         /* row-major 4x4: moves the uploaded source onto the target */
  int32_t hypothesis;  /* the winner's h, -1: none */
  int32_t n_valid;     /* hypotheses that passed the draw and the edge check */
  int32_t n_matches;
  int32_t reserved;
  int64_t inliers;
  double sums[ICPK_NSCORE]; /* the winner's sums as icpk_score_poses returns them */
} icpk_global_result;
void icpk_default_global_params(icpk_global_params *p); /* 4096 hypotheses, seed 0, max_dist 0.75, edge_similarity 0.9 */
int icpk_compute_fpfh(icpk_ctx *ctx, int32_t which, float radius, int32_t flags);
int icpk_get_fpfh(icpk_ctx *ctx, int32_t which, float *desc, uint8_t *valid, int32_t *n);
int icpk_get_spfh(icpk_ctx *ctx, int32_t which, int32_t *counts, int32_t *m);
int icpk_match_features(icpk_ctx *ctx, int32_t flags);
int icpk_get_feature_matches(icpk_ctx *ctx, int32_t *src_index, int32_t *tgt_index, float *D, int32_t *n);
int icpk_register_global(icpk_ctx *ctx, const icpk_global_params *p, icpk_global_result *out);
int icpk_global_hypotheses(const int32_t *match_src, const int32_t *match_tgt, int32_t n_matches, const float *sx,
                           const float *sy, const float *sz, int32_t ns, const float *tx, const float *ty,
                           const float *tz, int32_t nt, uint64_t seed, float edge_similarity, int64_t h0, int32_t count,
                           int32_t *samples, uint8_t *valid, float *T);

/* ---- pose-graph optimisation (extension, K18) ------------------------------------------------------------------
 * The consumer of K15's information matrix and of K16's loop closures: a graph of pairwise alignments, each weighted
 * by its information matrix, optimised by Levenberg-Marquardt with a line process that switches wrong loop closures
 * off (multiway registration).  Everything is float64 on the host and on the device; poses are 4 x 4, row-major.
 *
 * THE RULE
 *   nodes      P_i, i in [0, n_nodes), maps node i's cloud into the world.
 *   edges      (s, t, T_st, L, uncertain).  T_st moves cloud s onto cloud t: what icpk_align returns with s as source
 *              and t as target.  The edge is satisfied when P_s = P_t T_st.  L is the 6 x 6 information matrix,
 *              rotation first and translation second: icpk_information_matrix's order (G = [-[q]x | I], q in the
 *              target's frame).  Only finiteness is asked of L; the rule reads all 36 entries as given.
 *   residual   E = P_t^-1 P_s T_st^-1 (the error on the left, in the target's frame: the frame L is expressed in);
 *              r = (rotation vector of R_E, t_E) in R^6; chi2 = r^T L r.  The inverse of a pose [R | t] is taken as
 *              [R^T | -R^T t].  Rotation vector: v = (R32 - R23, R13 - R31, R21 - R12) / 2, s = |v|,
 *              c = (trace R - 1) / 2, theta = the angle of (c, s), w = v * (theta / s); for s < 1e-8 and c > 0:
 *              w = v * (1 + s^2 / 6); s = 0 otherwise: w = 0.  (theta -> pi is not treated: an edge whose error is a
 *              half turn says nothing.)
 *   no libm    The rule is +, -, *, / and sqrt in a fixed order, so that it gives the same bytes on the device and on
 *              any IEEE host (tests/posegraph_model.py restates it operation for operation).  The angle of (c, s):
 *              atan(s / c) for c > 0, else pi/2 + atan(-c / s); atan(x), x >= 0: the reciprocal above 1 (pi/2 - ...),
 *              three halvings x <- x / (1 + sqrt(1 + x^2)), then 8 x (1 - x^2/3 + ... - x^26/27) by Horner.
 *              sin(th) / th and (1 - cos th) / th^2: their power series in th^2, 20 terms in nested form
 *              (1 - th^2/(2 3) (1 - th^2/(4 5) (...))): accurate to a few ulps for th <= pi (held against libm in
 *              tests/test_posegraph_host.py), usable to 2 pi.  Well beyond 2 pi the 20 terms no longer reach the
 *              series' tail and Rodrigues(w) is no rotation; the rule does not bound |w| of an LM step (a step of
 *              more than a turn means the linearisation said nothing, and the gain ratio rejects it or not as for
 *              any other step).
 *              Every 3-term product is (a0 b0 + a1 b1) + a2 b2, every longer one is summed left to right from 0.
 *   line process (uncertain edges, mu = preference_loop_closure > 0): l = (mu / (mu + chi2))^2, recomputed from the
 *              poses at every evaluation and held constant inside a linearisation; every other edge, and every edge
 *              when mu = 0, has l = 1.  Cost = sum over certain edges of chi2 + sum over uncertain edges of
 *              (l chi2 + mu (sqrt(l) - 1)^2), the edges' terms summed in edge order through the canonical tree
 *              (ICPK_RED_THREADS / ICPK_RED_MAX_BLOCKS) with n_edges elements.
 *   update     P_i <- Exp(d_i) P_i, d = (w, v), Exp(d) = [Rodrigues(w) | v]: R' = Rodrigues(w) R, t' = Rodrigues(w) t
 *              + v -- the same split as the residual; the full SE(3) exponential is not needed.  Rodrigues(w) = I +
 *              a [w]x + b [w]x^2, a = sin(th) / th, b = (1 - cos(th)) / th^2 (th = |w|; the series above).  d of
 *              reference_node is identically zero: that pose comes back with the bytes it
 *              went in with.
 *   Jacobians  analytic and exact to first order.  With B = P_s T_st^-1 and th = rotation vector of R_E:
 *              J_s = [ Jl^-1(th) R_t^T , 0 ; -R_t^T [t_B]x , R_t^T ],  J_t = -J_s,  where Jl^-1(th) = I - [th]x / 2 +
 *              k [th]x^2 is the inverse left Jacobian of SO(3), k = 1 / |th|^2 - (1 + cos|th|) / (2 |th| sin|th|)
 *              with sin and cos from the series above (|th| < 1e-2: k = 1/12 + |th|^2 / 720 + |th|^4 / 30240).  Because J_t = -J_s an edge contributes ONE
 *              block A = J_s^T (l L) J_s and one vector b = J_s^T (l L) r: H_ss = H_tt = A, H_st = H_ts = -A, g_s = b,
 *              g_t = -b.  A node sums its incident edges' A and +-b in ascending edge index.
 *   LM         Nielsen's schedule on (H + lambda diag H) d = -g: lambda_0 = tau max diag(H), nu = 2.  Gain ratio
 *              rho = (F - F_trial) / pred, pred = sum_i d_i . (lambda diag(H_ii) d_i - g_i) (canonical tree over the
 *              nodes); a step is accepted when pred > 0 and rho > 0: lambda <- lambda max(1/3, 1 - (2 rho - 1)^3),
 *              nu = 2; otherwise lambda <- lambda nu, nu <- 2 nu.  The loop stops before its first iteration when
 *              |g|inf < gradient_tolerance; after an accepted step when (F - F_trial) / F < cost_tolerance,
 *              max |d| < step_tolerance or |g|inf < gradient_tolerance; after a rejected one when max |d| <
 *              step_tolerance; and at max_iterations, which returns ICPK_W_NOT_CONVERGED.
 *   linear solve  preconditioned conjugate gradients from d = 0, the preconditioner block Jacobi (one 6 x 6 Cholesky
 *              of H_ii + lambda diag H_ii per node; a pivot that is not > 0 is replaced by 1 and its column's
 *              off-diagonal entries by 0).  It stops when |residual|_2 <= pcg_tolerance |g|_2 (checked before the
 *              first iteration too) or at max_pcg_iterations.  H p is a gather per node: sum over the incident edges
 *              in ascending index of A (p_i - p_other), plus lambda diag(H_ii) p_i.  The dot products go through the
 *              canonical tree over the nodes (a node's term is its six products added in order).  The rows of
 *              reference_node are those of the identity with right-hand side 0.
 *   pruning    (ICPK_PG_PRUNE) after convergence the uncertain edges with l < edge_prune_threshold are dropped and the
 *              optimisation runs once more from where it stands over the remaining edges (lambda starts again from
 *              tau max diag H).  The final l and chi2 of EVERY edge, dropped ones included, are evaluated at the final
 *              poses.  When the remaining edges would no longer join every node to reference_node (the dropped ones
 *              were the only way to some node), nothing is pruned: the mask is all zero, n_pruned is 0, there is no
 *              second run and the first run's poses are the result.
 *   exact      no floating-point atomics; the same bytes on every run and on every context.
 *
 * icpk_pose_graph_check is the host-side refusal both calls start with (no device work, no context): ICPK_E_ARG for a
 * NULL pointer, n_nodes < 2 or > ICPK_PG_MAX_NODES, n_edges < 1 or > ICPK_PG_MAX_EDGES, an edge with s == t or an index
 * out of range, a non-finite pose, T_st or L, a node the reference node cannot reach through the edges, a
 * reference_node out of range, an unknown flag, max_iterations < 0, max_pcg_iterations < 1, or a tolerance, tau,
 * preference_loop_closure or edge_prune_threshold that is negative or not finite (tau must be > 0).  params may be NULL
 * (icpk_default_pg_params).  Nothing is launched and nothing written when it refuses.
 *
 * icpk_pose_graph_optimize   poses: in, out.  result and the three per-edge outputs may be NULL.  Returns ICPK_OK, or
 *     ICPK_W_NOT_CONVERGED when a run of the loop ended at max_iterations.  One host wait per LM iteration.
 * icpk_pose_graph_evaluate   one edge pass and one node pass at the given poses, nothing moves: per edge chi2 and l
 *     (mu as preference_loop_closure; every edge counts as given by its `uncertain`), the cost and the gradient
 *     (6 n_nodes: g_i = sum of +-b, reference node included; any output may be NULL).
 * icpk_get_pose_graph_trace  per LM iteration of the last optimize: the cost after it, the lambda it ran with, its PCG
 *     iterations and whether its step was accepted.  Arrays need room for *n_iter entries as returned by a call with
 *     NULL arrays (at most 2 max_iterations); any may be NULL.
 * The calls read and write nothing else the context holds. */
#define ICPK_W_NOT_CONVERGED 4 /* icpk_pose_graph_optimize ran into max_iterations */
#define ICPK_PG_PRUNE 1        /* flags of icpk_pg_params */
#define ICPK_PG_MAX_NODES (1 << 20)
#define ICPK_PG_MAX_EDGES (1 << 22)
typedef struct icpk_pg_edge {
  int32_t source, target;
  int32_t uncertain; /* != 0: a loop closure the line process may switch off */
  int32_t reserved;
  double T[16];    /* row-major 4x4: moves cloud `source` onto cloud `target` */
  double info[36]; /* row-major 6x6, rotation first */
} icpk_pg_edge;
typedef struct icpk_pg_params {
  int32_t max_iterations;     /* 100 */
  int32_t max_pcg_iterations; /* 200 */
  double pcg_tolerance;       /* 1e-8 */
  double tau;                 /* 1e-3 */
  double cost_tolerance;      /* 1e-9 */
  double step_tolerance;      /* 1e-10 */
  double gradient_tolerance;  /* 1e-10 */
  double preference_loop_closure; /* 0: no line process */
  double edge_prune_threshold;    /* 0.25 */
  int32_t reference_node;     /* 0 */
  int32_t flags;              /* 0 */
} icpk_pg_params;
typedef struct icpk_pg_result {
  int32_t iterations;     /* LM iterations, both runs of a pruning call */
  int32_t accepted;       /* ... of which accepted */
  int32_t pcg_iterations; /* total */
  int32_t n_pruned;
  double initial_cost, final_cost;
  double final_lambda;
} icpk_pg_result;
void icpk_default_pg_params(icpk_pg_params *p);
int icpk_pose_graph_check(int32_t n_nodes, const double *poses, int32_t n_edges, const icpk_pg_edge *edges,
                          const icpk_pg_params *params);
int icpk_pose_graph_optimize(icpk_ctx *ctx, int32_t n_nodes, double *poses /* in, out: 16 * n_nodes */, int32_t n_edges,
                             const icpk_pg_edge *edges, const icpk_pg_params *params, icpk_pg_result *result,
                             double *edge_weight_out, double *edge_chi2_out, uint8_t *pruned_out);
int icpk_pose_graph_evaluate(icpk_ctx *ctx, int32_t n_nodes, const double *poses, int32_t n_edges,
                             const icpk_pg_edge *edges, double mu, double *chi2_out, double *weight_out,
                             double *cost_out, double *gradient_out /* 6 * n_nodes or NULL */);
int icpk_get_pose_graph_trace(icpk_ctx *ctx, int32_t *n_iter, double *cost_out, double *lambda_out,
                              int32_t *pcg_iterations_out, int32_t *accepted_out);

/* ---- TSDF volume (extension, K19 - K23) ---------------------------------------------------------------------------
 * What the poses of K18 are for: the posed depth frames fused into one model.  One dense volume of truncated signed
 * distances per context, owned by it like the map: created by icpk_tsdf_create, released by icpk_tsdf_release or
 * icpk_destroy, and touched by no other call.  Every voxel is owned by one thread: no atomic, the same bytes on every
 * run and on every context.
 *
 * THE PER-VOXEL RULE (icpk_tsdf_integrate; float32, every operation rounded once, in the order written; no fused
 * multiply-add, correctly rounded division, no libm).  Voxel (i, j, k), linear index i + dims[0] (j + dims[1] k):
 *   1. centre   p_a = fl(fl((float)i_a + 0.5f) * voxel) + origin_a for the three axes.
 *   2. camera   q_r = fl(fl(fl(R_r0 p_x + R_r1 p_y) + R_r2 p_z) + t_r) for the three rows of the INVERTED pose.  The
 *               pose is double[16], row-major, camera-to-world [R | t] (icpk_pose_graph_optimize's layout); the library
 *               inverts it on the host in double, R' = R^T and t'_r = -((R_0r t_0 + R_1r t_1) + R_2r t_2), and rounds
 *               the twelve numbers to float once (icpk_tsdf_invert_pose).
 *   3. q_z <= 0 (or NaN) leaves the voxel alone.
 *   4. pixel    u = fl(fl(q_x fx) / q_z) + cx,  v = fl(fl(q_y fx) / q_z) + cx: cx and fx serve both axes, as in
 *               icpk_backproject (pointcloud.cpp:37-39), so that a back-projected pixel projects onto itself.
 *   5. col = floor(u + 0.5f), row = floor(v + 0.5f); outside [0, cols) x [0, rows), or depth d == 0 there: alone.
 *   6. sdf = fl((float)d / depth_scale) - q_z;  sdf < -trunc: alone.
 *   7. f = min(1, sdf / trunc).
 *   8. tsdf <- fl(fl(fl(tsdf * (float)w) + f) / fl((float)w + 1)), w the voxel's weight before the frame.
 *   9. with ICPK_TSDF_COLOR the voxel's intensity takes the pixel's intensity the same way.
 *  10. w <- min(w + 1, max_weight).
 *  11. n_updated = the number of voxels written (an integer count).
 * A fresh or reset volume holds tsdf = 0, w = 0, intensity = 0 everywhere.  A voxel is computed from its own indices.
 *
 * THE SURFACE RULE (icpk_tsdf_extract_surface).  For every voxel V with w >= min_weight (min_weight >= 1), in ascending
 * linear index, and for its +1 neighbour N along x, then y, then z, where N is in bounds and has w >= min_weight too:
 *   crossing   iff (f_V < 0) != (f_N < 0);  t = f_V / (f_V - f_N).
 *   point      V's centre (rule 1), plus fl(t * voxel) along the axis.
 *   intensity  I_V + fl(t * fl(I_N - I_V)) on a colour volume, else 0.
 *   gradient   of a voxel: g_a = tsdf(+1 along a) - tsdf(-1 along a), a = x, y, z (not scaled: only its direction is
 *              used); defined only where all six neighbours are in bounds with w >= min_weight.
 *   normal     m_a = g_V,a + fl(t * fl(g_N,a - g_V,a));  len = sqrt(fl(fl(m_x m_x + m_y m_y) + m_z m_z));  n = m / len
 *              (correctly rounded sqrt and division).  It points towards positive distance: towards the cameras.
 *   A crossing one of whose ends lacks a gradient, or with len == 0, is not listed and counted in n_no_normal.
 *   order      ascending linear voxel index, then axis: fixed by a count pass, a scan of the chunk counts and a scatter.
 * The list stays on the device until the next extraction, icpk_tsdf_create, _reset or _release.
 *
 * icpk_tsdf_create   ICPK_E_ARG for a dim < 1, more than ICPK_TSDF_MAX_VOXELS voxels, a voxel, trunc or depth_scale
 *     that is not finite and > 0, a non-finite origin, max_weight outside 1 .. 65535 or an unknown flag; the volume the
 *     context held stays then.  Otherwise it replaces that volume.  params NULL: icpk_default_tsdf_params.
 * icpk_tsdf_reset    the volume back to its fresh state (ICPK_E_NOT_SET without one); icpk_tsdf_release frees it (fine
 *     without one).
 * icpk_tsdf_integrate   depth: rows x cols host uint16, or NULL: the frame icpk_backproject_pair left resident on this
 *     context -- its filtered copy when the filter was on -- and ICPK_E_NOT_SET when there is none of this size.
 *     intensity: rows x cols host floats, finite and in [0, 1]; ICPK_E_ARG when given on a volume without
 *     ICPK_TSDF_COLOR, missing on one with it, or out of range.  ICPK_E_ARG also for a non-finite pose, fx that is not
 *     finite and > 0, a non-finite cx, rows or cols < 1 or more than 2^28 pixels.  ICPK_E_NOT_SET without a volume.
 *     n_updated may be NULL; with the resident frame, no intensity and n_updated == NULL the call does not wait.
 * icpk_tsdf_get      the planes as float32 / uint16 / float32 (the last: ICPK_E_ARG on a volume without colour), each
 *     of dims[0] dims[1] dims[2] entries; any pointer may be NULL.
 * icpk_tsdf_extract_surface   ICPK_E_ARG for min_weight outside 1 .. 65535, or when more than ICPK_TSDF_MAX_SURFACE
 *     crossings would be listed.  One host wait (the counts).  Either output may be NULL; n_no_normal stops at INT32_MAX.
 * icpk_tsdf_get_surface   the list of the last extraction (ICPK_E_NOT_SET before it): arrays of n_points entries, any
 *     may be NULL.  voxel_index: V's linear index; axis: 0, 1, 2.
 * icpk_tsdf_surface_to_target   the list becomes the context's target, its normals the target's normals and, on a colour
 *     volume, its intensities the target's colours: device-to-device, as icpk_map_list_to_target hands a list over,
 *     and everything a new target invalidates is invalidated the same way.  An empty list: ICPK_E_EMPTY_TARGET and the
 *     target stays.  ICPK_E_NOT_SET before the first extraction.
 * icpk_tsdf_voxel_update   host only, no context: rules 1 - 10 for the `count` voxels from linear index `first`, given
 *     the inverted float pose (R, t), the image and the voxels' state (tsdf, weight, intensity_value: arrays of `count`
 *     entries, in and out; intensity and intensity_value both NULL without colour).  Compiled from the header the
 *     kernel includes (csrc/tsdf_rule.h).  Returns the number of voxels written, or ICPK_E_ARG.
 * Integration and extraction read and write nothing else the context holds.
 *
 * THE RAY RULE (icpk_tsdf_raycast, K20): the surface visible from one pose, as vertex and normal maps of rows x cols
 * pixels -- the prediction step of frame-to-model tracking.  float32, every operation rounded once, in the order
 * written; no fused multiply-add, correctly rounded / and sqrt, no libm; a floor is a comparison and a truncating
 * conversion of a non-negative number.  Pixel (row, col) of a camera with fx, cx (cx and fx serve both axes, rule 4
 * above):
 *   0. pose     double[16], row-major, camera-to-world [R | c]; its nine R and three c are rounded to float once.
 *               Nothing is inverted.
 *   1. a = fl(fl((float)col - cx) / fx),  b = fl(fl((float)row - cx) / fx).
 *   2. direction per unit depth  d_r = fl(fl(fl(R_r0 a) + fl(R_r1 b)) + R_r2).  It is not normalised: the ray's
 *               parameter is the camera-frame depth z.
 *   3. samples  z_n = fl(fl((float)n step) + z_near), n = 0 .. N - 1, N = floor((z_far - z_near) / step) + 1 computed
 *               on the host in double from the float parameters.  Nothing is accumulated along the ray.
 *   4. point    p_r(z) = fl(c_r + fl(z d_r)).
 *   5. SAMPLE(p)   g_a = fl(fl(fl(p_a - origin_a) / voxel) - 0.5f); in range iff g_a >= 0 && g_a < (float)(dims_a - 1)
 *               on all three axes (NaN compares false; a volume with a dim of 1 is never in range).  i_a = (int)g_a,
 *               w_a = fl(g_a - (float)i_a).  KNOWN iff in range and all eight voxels (i_x + {0,1}, i_y + {0,1},
 *               i_z + {0,1}) have weight >= min_weight.  Its value is the trilinear interpolation of their tsdf with
 *               lerp(u, v, w) = fl(u + fl(w fl(v - u))): along x for the four (y, z) pairs, then along y, then along z.
 *   6. march    in ascending n.  An unknown sample forgets the previous one.  Two consecutive known samples with
 *               !(f_prev < 0) and f_cur < 0 are a crossing (the surface rule's sign convention); with f_prev < 0 and
 *               !(f_cur < 0) they end the ray without a hit (a back face).  Anything else goes on; a ray that uses up
 *               its samples has no hit.
 *   7. hit      t = fl(f_prev / fl(f_prev - f_cur)) (the divisor is > 0), z* = fl(z_prev + fl(t fl(z_cur - z_prev))),
 *               p* = p(z*).  The bracket is not refined.
 *   8. normal and intensity at p*: in SAMPLE's cell at p*, the surface rule's gradient at the eight corners (same
 *               min_weight); m_a = the trilinear lerp of the eight g_a; len = sqrt(fl(fl(m_x m_x + m_y m_y) + m_z m_z));
 *               n = m / len.  The intensity is the trilinear lerp of the intensity plane, or 0 without colour.  A
 *               crossing whose cell at p* is out of range or not known, one of whose eight corners lacks a gradient,
 *               or with len not > 0 is NOT LISTED and counted in n_no_normal; its ray ends there.
 *   9. output   eight planes of rows x cols floats: x, y, z, nx, ny, nz, depth (= z*), intensity.  A pixel without a
 *               listed hit holds 0 in all eight; depth > 0 is the validity test (z_near > 0).  Two integer counts:
 *               n_hits (listed) and n_no_normal.
 * One thread owns one pixel; the samples sit on the fixed lattice z_n, so the bits do not depend on how the image is
 * cut into workgroups.  The maps are a snapshot: they stay on the device until the next ray cast, icpk_tsdf_create,
 * _reset or _release; integration leaves them alone.
 *
 * icpk_tsdf_raycast   params NULL: icpk_default_tsdf_raycast_params.  step == 0: trunc / 2.  ICPK_E_NOT_SET without a
 *     volume.  ICPK_E_ARG for a NULL or non-finite pose; rows or cols < 1, fx that is not finite and > 0, a non-finite
 *     cx, more than ICPK_TSDF_MAX_RAYCAST_PIXELS pixels; z_near, z_far or step that is not finite; z_near <= 0,
 *     z_far <= z_near or step < 0; N > ICPK_TSDF_MAX_RAY_SAMPLES; min_weight outside 1 .. 65535.  A refused call leaves
 *     the maps of the last ray cast, the target and the volume as they were.  Either count may be NULL; with both NULL
 *     the call does not wait on the host.  It reads the planes and writes only its maps: nothing else the context
 *     holds is touched, the surface list of icpk_tsdf_extract_surface included.
 * icpk_tsdf_get_raycast   the eight planes of the last ray cast, rows x cols floats each, any pointer may be NULL.
 *     ICPK_E_NOT_SET without a volume, before the first ray cast and after icpk_tsdf_create, _reset or _release;
 *     ICPK_E_ARG when intensity is asked from a volume without colour.
 * icpk_tsdf_raycast_to_target   the valid pixels of the maps (depth > 0), in row-major pixel order, become the
 *     context's target, their normals the target's normals and, on a colour volume, their intensities the target's
 *     colours: exactly what icpk_tsdf_surface_to_target does with its list, device to device.  The order is a function
 *     of the maps alone (a count per 256 consecutive pixels, a scan, a scatter).  ICPK_E_NOT_SET as for
 *     icpk_tsdf_get_raycast; no valid pixel: ICPK_E_EMPTY_TARGET and the target stays.
 * icpk_tsdf_raycast_pixels   host only, no context: rules 0 - 9 for the `count` pixels from row-major pixel `first`,
 *     over host planes (intensity NULL exactly when params has no ICPK_TSDF_COLOR).  out: 8 planes of `count` floats.
 *     Compiled from the header the kernel includes (csrc/tsdf_rule.h).  Returns the number of listed hits, or
 *     ICPK_E_ARG: for what icpk_tsdf_create and icpk_tsdf_raycast refuse, a NULL array, first < 0, count < 0 or
 *     first + count > rows cols.
 *
 * THE MESH RULE (icpk_tsdf_extract_mesh, K21): the surface as a triangle mesh, by marching tetrahedra over the Kuhn
 * (Freudenthal) split of every cell.  float32, every operation rounded once, in the order written, no fused
 * multiply-add, no libm, as the surface rule.  A corner or an edge type is a mask e = x + 2 y + 4 z (bit 0: +x).
 *   1. cell     C = (i, j, k), 0 <= i_a <= dims_a - 2, with the corners C + e, e = 0 .. 7 (rule 5's order above).  KNOWN
 *               iff all eight have w >= min_weight.  Only known cells emit triangles; a dim of 1 has no cells.
 *   2. tetrahedra   six per cell, one per permutation (a, b, c) of the axes in lexicographic order xyz, xzy, yxz, yzx,
 *               zxy, zyx: v0 = 0, v1 = 1 << a, v2 = v1 | 1 << b, v3 = 7.  xyz, yzx, zxy are EVEN, the others ODD.
 *               Every edge of a tetrahedron joins a voxel V to V + m, m in 1 .. 7: V OWNS the edge, m is its type.
 *   3. vertex   on edge (V, m), N = V + m: a crossing iff (f_V < 0) != (f_N < 0);  t = f_V / (f_V - f_N).
 *               point      V's centre, plus fl(t * voxel) along every axis in m.
 *               intensity  I_V + fl(t * fl(I_N - I_V)) on a colour volume, else 0.
 *               normal     the surface rule's, from the gradients of V and N.  Where an end lacks a gradient or len is
 *                          not > 0 the normal is (0, 0, 0) and the vertex is counted in n_no_normal -- and STILL LISTED.
 *               listed     iff it is a crossing and at least one KNOWN cell contains the edge: the cells V - u, u & m == 0,
 *                          that are in range (four for an axis edge, two for a face diagonal, one for the body diagonal).
 *               order      ascending linear index of V, then ascending m.
 *   4. triangles   the known cells in ascending linear index of their lower corner, their tetrahedra in rule 2's order.
 *               The case is the mask whose bit n is f(v_n) < 0.  For an EVEN tetrahedron, pq naming the vertex on the
 *               edge between positions p and q:
 *                  0, 15  none                      8   (30,32,31)
 *                  1   (01,02,03)                   9   (01,02,32) (01,32,31)
 *                  2   (10,13,12)                   10  (10,32,12) (10,30,32)
 *                  3   (02,03,13) (02,13,12)        11  (20,23,21)
 *                  4   (20,21,23)                   12  (20,21,31) (20,31,30)
 *                  5   (01,23,03) (01,21,23)        13  (10,12,13)
 *                  6   (10,13,23) (10,23,20)        14  (01,03,02)
 *                  7   (30,31,32)
 *               An ODD tetrahedron swaps the second and the third vertex of every triangle.  With this winding
 *               (b - a) x (c - a) points towards positive distance, as the normals do.  Behind the table: a position p
 *               alone on its side gives the triangle on its edges to the other three in ascending order, second and
 *               third swapped iff (p odd) != (the lone one is the positive one); two negative positions p < q and two
 *               others r < s give (pr, ps, qs) (pr, qs, qr), both swapped iff p + q is even.
 *               A triangle is three int32 indices into the vertex list.  A voxel Z with f == 0 puts the vertices of all
 *               crossing edges into Z at Z in exact arithmetic: triangles without area, which are kept so that the mesh
 *               stays closed.  IN FLOAT32 they coincide bit for bit only where centre(V) + voxel == centre(V + 1)
 *               exactly, i.e. on a dyadic voxel and origin.  Elsewhere such a triangle is a sliver of rounding-error
 *               size whose winding is decided by the rounding and may face inwards (voxel 0.05, a sphere through 30
 *               lattice points: 152 triangles of area 0, 76 slivers, 39 of them inwards).  A consumer that needs strict
 *               orientation drops triangles below an area threshold; the index list stays orientable either way.
 *   5. counts   n_vertices, n_triangles, n_no_normal: integers.
 * The mesh is closed inside the known cells -- open where the surface leaves them or the volume -- and consistently
 * oriented: no directed edge occurs twice.  A vertex on an axis edge (m = 1, 2, 4) with a normal is the surface rule's crossing (V, log2 m), bit
 * for bit.
 *
 * icpk_tsdf_extract_mesh   ICPK_E_NOT_SET without a volume; ICPK_E_ARG for min_weight outside 1 .. 65535, or when more
 *     than ICPK_TSDF_MAX_SURFACE vertices or triangles would be listed.  Any output may be NULL.  One host wait (the
 *     counts).  The mesh stays on the device until the next mesh extraction, icpk_tsdf_create, _reset, _set or _release.
 *     It reads the planes and writes only the mesh: the surface list, the ray-cast maps and everything else the context
 *     holds stay as they are, and icpk_tsdf_extract_surface and icpk_tsdf_raycast leave the mesh alone.
 * icpk_tsdf_get_mesh   the mesh of the last extraction (ICPK_E_NOT_SET before it): arrays of n_vertices entries, edge the
 *     type m; triangles: 3 n_triangles indices.  Any pointer may be NULL.
 * icpk_tsdf_set      the counterpart of icpk_tsdf_get: the planes from host arrays of dims[0] dims[1] dims[2] entries (a
 *     saved model, or an analytic field).  ICPK_E_NOT_SET without a volume; ICPK_E_ARG for a NULL tsdf or weight, a tsdf
 *     that is not finite or outside [-1, 1], intensity given to a volume without colour, missing on one with it, or
 *     outside [0, 1]; the volume stays then.  It drops the surface list, the ray-cast maps and the mesh, as _reset does.
 * icpk_tsdf_mesh_host   host only, no context: rules 1 - 5 over host planes (intensity NULL exactly when params has no
 *     ICPK_TSDF_COLOR), compiled from the header the kernels include (csrc/tsdf_rule.h).  counts = {n_vertices,
 *     n_triangles, n_no_normal} is always filled once the arguments are accepted; the arrays (any may be NULL) are filled
 *     when n_vertices <= cap_vertices and n_triangles <= cap_triangles, else ICPK_E_ARG.  ICPK_E_ARG also for what
 *     icpk_tsdf_create and icpk_tsdf_extract_mesh refuse, a NULL tsdf, weight or counts, or a negative capacity.
 *
 * THE SHIFT RULE (icpk_tsdf_shift, K23): the volume follows the camera by whole voxels (KinectFusion's moving volume).
 * A volume remembers the origin it was created with, origin0 (float[3]), and a cumulative shift, total (int64[3]; zero
 * after icpk_tsdf_create and after icpk_tsdf_reset; icpk_tsdf_set leaves it).  icpk_tsdf_shift(ctx, s):
 *   content     the new voxel (i, j, k) takes tsdf, weight and (ICPK_TSDF_COLOR) intensity of the old voxel
 *               (i + s_x, j + s_y, k + s_z) where that voxel is in bounds; elsewhere it is fresh (0, 0, 0).  Any sign;
 *               |s_a| >= dims_a empties the volume; s = 0 is a no-op that succeeds (and drops nothing).
 *   origin      total += s;  origin_a = (float)((double)origin0_a + (double)total_a * (double)voxel): always from
 *               origin0 and total, never accumulated, so shifting there and back returns the creation origin bit for
 *               bit.  Every other rule (rule 1, the ray rule's SAMPLE, the mesh rule) reads this origin exactly as it
 *               read params.origin before.
 *   dropped     the surface list, the ray-cast maps and the mesh (they index the old volume): their getters answer
 *               ICPK_E_NOT_SET afterwards, as after icpk_tsdf_reset.  Nothing else the context holds is touched: source
 *               and target (even a target handed over from this volume earlier), normals, colours, associations, seeds,
 *               map lists, the resident frame.  Stream-ordered: no host wait.  The first shift allocates a second set
 *               of planes (the move is out of place; the two sets change places), which the volume keeps.
 * THE LEAVING LIST (icpk_tsdf_extract_leaving): the surface rule on the volume as it stands, restricted to the crossings
 * a shift by s would lose.  stays(v): s_a <= v_a < dims_a + s_a on all three axes, for an old voxel index v.  A listed
 * crossing (V, N) is KEPT by the shift iff stays holds for V, for N and for the six axis neighbours of each -- only then
 * does it still have both gradients in the shifted volume.  The leaving list is every crossing the surface rule lists
 * that is not kept, in the surface rule's order; n_no_normal counts the crossings dropped for want of a normal one of
 * whose ends (V or N) does not stay.  So the surface list before a shift is the leaving list plus the surface list after
 * it (voxel indices mapped back), exactly and disjointly; kept normals and intensities are the same bits, kept points
 * differ by the rounding of the new origin.  The result REPLACES the context's surface list: icpk_tsdf_get_surface and
 * icpk_tsdf_surface_to_target work on it unchanged, voxel_index is the OLD linear index.  A crossing streamed out from
 * the rim may be listed again later, when new frames re-fill the fresh slab next to it and give it back its gradients:
 * a consumer that stitches streamed lists must expect such repeats near slab borders.
 *
 * icpk_tsdf_shift    ICPK_E_NOT_SET without a volume, ICPK_E_ARG for a NULL s.  A refused call leaves everything as it
 *     was.
 * icpk_tsdf_extract_leaving   ICPK_E_NOT_SET without a volume; ICPK_E_ARG for a NULL s, min_weight outside 1 .. 65535, or
 *     when more than ICPK_TSDF_MAX_SURFACE crossings would be listed; a refused call leaves everything, the surface list
 *     included, as it was.  One host wait (the count), as icpk_tsdf_extract_surface.
 * icpk_tsdf_get_params   the parameters in force (with the CURRENT origin) and the cumulative shift; either pointer may
 *     be NULL.  ICPK_E_NOT_SET without a volume.
 * icpk_tsdf_get_box  the planes of the sub-box lo_a <= v_a < hi_a, x fastest, (hi_x - lo_x)(hi_y - lo_y)(hi_z - lo_z)
 *     entries each: a leaving slab can be archived losslessly with it.  Any plane pointer may be NULL.  ICPK_E_NOT_SET
 *     without a volume; ICPK_E_ARG for a NULL lo or hi, an empty or out-of-bounds box, or intensity on a volume without
 *     colour. */
#define ICPK_TSDF_COLOR 1 /* flags of icpk_tsdf_params: one intensity per voxel */
#define ICPK_TSDF_MAX_VOXELS (1 << 30)
#define ICPK_TSDF_MAX_SURFACE (1 << 28)
typedef struct icpk_tsdf_params {
  int32_t dims[3];   /* voxels, x fastest (256, 256, 256) */
  float voxel;       /* metres (0.02) */
  float origin[3];   /* world position of the corner of voxel (0, 0, 0) (-2.56, -2.56, 0) */
  float trunc;       /* metres (0.08) */
  int32_t max_weight; /* 1 .. 65535 (255) */
  float depth_scale; /* ICPK_DEPTH_SCALE */
  int32_t flags;     /* 0 */
} icpk_tsdf_params;
void icpk_default_tsdf_params(icpk_tsdf_params *p);
int icpk_tsdf_create(icpk_ctx *ctx, const icpk_tsdf_params *params);
int icpk_tsdf_reset(icpk_ctx *ctx);
int icpk_tsdf_release(icpk_ctx *ctx);
int icpk_tsdf_integrate(icpk_ctx *ctx, const uint16_t *depth, const float *intensity, int32_t rows, int32_t cols,
                        float fx, float cx, const double pose[16], int32_t *n_updated);
int icpk_tsdf_get(icpk_ctx *ctx, float *tsdf, uint16_t *weight, float *intensity);
int icpk_tsdf_extract_surface(icpk_ctx *ctx, int32_t min_weight, int32_t *n_points, int32_t *n_no_normal);
int icpk_tsdf_get_surface(icpk_ctx *ctx, float *x, float *y, float *z, float *nx, float *ny, float *nz,
                          float *intensity, int32_t *voxel_index, uint8_t *axis);
int icpk_tsdf_surface_to_target(icpk_ctx *ctx);
/* host only: the inverse of a camera-to-world pose as rule 2 takes it; ICPK_E_ARG for a non-finite pose */
int icpk_tsdf_invert_pose(const double pose[16], float R[9], float t[3]);
int icpk_tsdf_voxel_update(const icpk_tsdf_params *params, const float R[9], const float t[3], const uint16_t *depth,
                           const float *intensity, int32_t rows, int32_t cols, float fx, float cx, int64_t first,
                           int32_t count, float *tsdf, uint16_t *weight, float *intensity_value);
#define ICPK_TSDF_MAX_RAY_SAMPLES 4096
#define ICPK_TSDF_MAX_RAYCAST_PIXELS (1 << 21)
typedef struct icpk_tsdf_raycast_params {
  int32_t rows, cols; /* 480 x 640 */
  float fx, cx;       /* 468.60, 318.27 */
  float z_near, z_far; /* metres of camera depth; 0 < z_near < z_far (0.25, 6.0) */
  float step;         /* metres of camera depth; 0: trunc / 2 (0) */
  int32_t min_weight; /* 1 .. 65535 (1) */
} icpk_tsdf_raycast_params;
void icpk_default_tsdf_raycast_params(icpk_tsdf_raycast_params *p);
int icpk_tsdf_raycast(icpk_ctx *ctx, const icpk_tsdf_raycast_params *params, const double pose[16], int32_t *n_hits,
                      int32_t *n_no_normal);
int icpk_tsdf_get_raycast(icpk_ctx *ctx, float *x, float *y, float *z, float *nx, float *ny, float *nz, float *depth,
                          float *intensity);
int icpk_tsdf_raycast_to_target(icpk_ctx *ctx);
int icpk_tsdf_raycast_pixels(const icpk_tsdf_params *params, const icpk_tsdf_raycast_params *ray, const double pose[16],
                             const float *tsdf, const uint16_t *weight, const float *intensity, int64_t first,
                             int32_t count, float *out /* 8 x count */);
int icpk_tsdf_extract_mesh(icpk_ctx *ctx, int32_t min_weight, int32_t *n_vertices, int32_t *n_triangles,
                           int32_t *n_no_normal);
int icpk_tsdf_get_mesh(icpk_ctx *ctx, float *x, float *y, float *z, float *nx, float *ny, float *nz, float *intensity,
                       int32_t *voxel_index, uint8_t *edge, int32_t *triangles /* 3 x n_triangles */);
int icpk_tsdf_set(icpk_ctx *ctx, const float *tsdf, const uint16_t *weight, const float *intensity);
int icpk_tsdf_mesh_host(const icpk_tsdf_params *params, int32_t min_weight, const float *tsdf, const uint16_t *weight,
                        const float *intensity, int64_t cap_vertices, int64_t cap_triangles, float *x, float *y, float *z,
                        float *nx, float *ny, float *nz, float *intensity_out, int32_t *voxel_index, uint8_t *edge,
                        int32_t *triangles, int64_t counts[3]);
int icpk_tsdf_shift(icpk_ctx *ctx, const int32_t s[3]);
int icpk_tsdf_extract_leaving(icpk_ctx *ctx, int32_t min_weight, const int32_t s[3], int32_t *n_points,
                              int32_t *n_no_normal);
int icpk_tsdf_get_params(icpk_ctx *ctx, icpk_tsdf_params *out, int64_t total[3]);
int icpk_tsdf_get_box(icpk_ctx *ctx, const int32_t lo[3], const int32_t hi[3], float *tsdf, uint16_t *weight,
                      float *intensity);

/* ---- K30: signed updates of the volume -- de-integration, and several frames in one pass ---------------------------
 * What a pose graph's corrections (K18) are for: a frame fused at a drifted pose is taken out again and fused at the
 * corrected one, without resetting the volume.
 *
 * THE SIGNED UPDATE RULE (icpk_tsdf_apply; float32, one rounding per operation in the order written, no fused
 * multiply-add, correctly rounded division, no libm, like THE PER-VOXEL RULE).  A call carries n_frames images and
 * n_ops ops; an op is a sign, the index of one of the call's images and a pose.  Every voxel takes the ops
 * 0 .. n_ops - 1 in the order listed, each on the state the op before it left:
 *   - steps 1 - 7 of THE PER-VOXEL RULE with the op's pose (inverted by icpk_tsdf_invert_pose) and the op's image,
 *     unchanged: they produce the sample f (and the pixel's intensity) or leave the voxel alone;
 *   - sign == +1: steps 8 - 10 as they are;
 *   - sign == -1, on the voxel's weight w:
 *       w == 0     the voxel is left alone and not counted;
 *       w == 1     tsdf <- +0.0f, intensity <- +0.0f, w <- 0: the bytes of the fresh state;
 *       otherwise  tsdf <- clamp(fl(fl(fl(tsdf * (float)w) - f) / fl((float)w - 1)), -1, 1), with ICPK_TSDF_COLOR the
 *                  intensity the same way with the pixel's intensity, clamped to [0, 1], and w <- w - 1.
 *   - n_updated[k] = the number of voxels op k wrote.
 * One call with n ops gives, by construction, the bytes of n calls with one op each in that order, and a single +1 op
 * gives icpk_tsdf_integrate's bytes.  On a fresh voxel +A then -A gives the fresh bytes back.  Otherwise a removal is
 * the inverse of the integration up to rounding: a few ulp of 1 per op, amplified by w / (w - 1).  A voxel whose weight
 * has reached max_weight has forgotten how many frames it holds: the rule still applies there (w <- max_weight - 1) and
 * is NOT an inverse.
 *
 * icpk_tsdf_apply   depth: n_frames pointers to rows x cols host uint16 images; intensity: n_frames pointers to
 *     rows x cols host floats in [0, 1] on a volume with ICPK_TSDF_COLOR, NULL on one without.  The images go into one
 *     device stack the volume owns (reused while the shape fits), so that "remove at the old pose, add at the new one"
 *     uploads its frame once; the volume is then crossed once for all ops.  ICPK_E_ARG for n_ops outside
 *     1 .. ICPK_TSDF_MAX_OPS, n_frames outside 1 .. n_ops, a sign other than +1 and -1, a frame index outside
 *     0 .. n_frames - 1, a NULL image (the resident frame of icpk_backproject_pair is not taken here), a NULL ops, and
 *     everything icpk_tsdf_integrate refuses; ICPK_E_NOT_SET without a volume.  A refused call leaves the volume's bytes
 *     as they were.  n_updated: n_ops entries, or NULL.  The call waits for the device.  It uses the volume's CURRENT
 *     origin (K23) and, like integration, touches nothing else the context holds: the surface list, the ray-cast maps,
 *     the mesh, the pyramid and the frame view stay as they are (snapshots of the volume before the call).
 * icpk_tsdf_deintegrate   icpk_tsdf_integrate's signature (depth must not be NULL): one op with sign -1.
 * icpk_tsdf_voxel_apply   host only, no context: the rule for the `count` voxels from linear index `first`, given the
 *     images, the ops and the voxels' state (tsdf, weight, intensity_value: arrays of `count` entries, in and out;
 *     intensity and intensity_value both NULL without colour).  Compiled from the header the kernel includes
 *     (csrc/tsdf_rule.h).  n_updated: n_ops entries (or NULL), set to the counts over these voxels.  Returns ICPK_OK, or
 *     ICPK_E_ARG for what icpk_tsdf_create and icpk_tsdf_apply refuse, a NULL state array, first < 0, count < 0 or a
 *     range past the volume. */
#define ICPK_TSDF_MAX_OPS 16
typedef struct icpk_tsdf_op {
  int32_t sign;    /* +1 integrate, -1 de-integrate */
  int32_t frame;   /* index into the call's frames */
  double pose[16]; /* camera-to-world, row-major, as icpk_tsdf_integrate's */
} icpk_tsdf_op;
int icpk_tsdf_apply(icpk_ctx *ctx, int32_t n_frames, const uint16_t *const *depth, const float *const *intensity,
                    int32_t rows, int32_t cols, float fx, float cx, int32_t n_ops, const icpk_tsdf_op *ops,
                    int64_t *n_updated);
int icpk_tsdf_deintegrate(icpk_ctx *ctx, const uint16_t *depth, const float *intensity, int32_t rows, int32_t cols,
                          float fx, float cx, const double pose[16], int32_t *n_updated);
int icpk_tsdf_voxel_apply(const icpk_tsdf_params *params, int32_t n_frames, const uint16_t *const *depth,
                          const float *const *intensity, int32_t rows, int32_t cols, float fx, float cx, int32_t n_ops,
                          const icpk_tsdf_op *ops, int64_t first, int32_t count, float *tsdf, uint16_t *weight,
                          float *intensity_value, int64_t *n_updated);

/* ---- K22: smoothing a depth frame before its vertex and normal maps are made -----------------------------------------
 * KinectFusion's first stage: a bilateral filter in front of the cloud (and the cross-product normals) that tracking
 * reads, while the RAW frame is what goes into the volume.  K6 (icpk_filter_depth_image) repairs holes and leaves noise
 * alone; this one leaves holes alone and averages noise, never across a depth step.
 *
 * THE BILATERAL RULE (icpk_bilateral_depth_image; integers only, so the result is a function of the image and the two
 * tables alone: tile shape, tap order and who computes it do not matter).
 *   Parameters (icpk_bilateral_params; defaults from icpk_default_bilateral_params):
 *     radius        1 .. ICPK_BILATERAL_MAX_RADIUS (3): the window is (2 radius + 1)^2 pixels
 *     sigma_space   pixels, finite and > 0 (2.0)
 *     sigma_range   depth units, finite and > 0 (30: 6 mm at ICPK_DEPTH_SCALE)
 *     range_cutoff  0, or 1 .. ICPK_BILATERAL_MAX_RANGE (0).  0: K = floor(3 sigma_range) + 1; otherwise K = range_cutoff.
 *                   A K above ICPK_BILATERAL_MAX_RANGE is refused, not clamped.
 *   Tables, computed once per call on the host in double (icpk_bilateral_tables returns them):
 *     ws[dy][dx] = (int)floor(4096 exp(-(dx^2 + dy^2) / (2 sigma_space^2)) + 0.5)   for dy, dx = -radius .. radius
 *     wr[k]      = (int)floor(4096 exp(-k^2 / (2 sigma_range^2)) + 0.5)             for k = 0 .. K - 1
 *     Both centres are 4096.
 *   Pixel p of depth d_p:
 *     d_p == 0 gives 0: holes are not filled.
 *     Otherwise tap q of the window contributes iff it lies inside the image, d_q != 0 and k = |d_q - d_p| < K.
 *     Its weight is W = ws * wr[k] (<= 2^24).  S_w = sum W (< 2^32 at 169 taps), S_wd = sum W d_q (< 2^48).
 *     out = floor((2 S_wd + S_w) / (2 S_w)): the weighted mean, rounded to nearest, halves up.
 *   The centre always contributes, so S_w > 0, out >= 1 and |out - d_p| <= K - 1: the validity mask of the image is
 *   preserved exactly, and a depth step of K or more is never averaged across.
 *
 * icpk_bilateral_depth_image   depth_in / depth_out: host arrays of rows x cols (may be the same array).  params NULL:
 *     the defaults.
 * icpk_backproject_smoothed    upload, filter, back-project, without the image leaving the device: as icpk_backproject
 *     (normals_mode < 0) or icpk_backproject_with_normals (normals_mode >= 0, which must be 1) on the smoothed image --
 *     icpk_backproject_filtered's convention.  Equivalent, bit for bit, to icpk_bilateral_depth_image followed by that
 *     call.  Both calls use the image buffers icpk_backproject_pair keeps its resident frame in: as after
 *     icpk_backproject_filtered, no frame is resident afterwards.
 * icpk_bilateral_tables        host only: ws receives (2 radius + 1)^2 entries, row-major (room for 169 covers every
 *     radius), wr receives *K entries (room for ICPK_BILATERAL_MAX_RANGE covers every K).  ws, wr or K may be NULL.
 * icpk_bilateral_host          host only: the rule over a host image, through the header the kernel includes
 *     (csrc/bilateral_rule.h).  depth_out may be depth_in.
 * Refusals (ICPK_E_ARG; a refused call leaves the context, its clouds and the output array as they were): a NULL
 *     image; rows or cols < 1, or more than 2^28 pixels; a radius outside 1 .. ICPK_BILATERAL_MAX_RADIUS; a sigma_space
 *     or sigma_range that is not finite and > 0; a range_cutoff outside 0 .. ICPK_BILATERAL_MAX_RANGE, or K above it;
 *     for icpk_backproject_smoothed also `which` outside 0 / 1, normals_mode >= 0 with which == 0, and a normals_mode
 *     icpk_backproject_with_normals does not know. */
#define ICPK_BILATERAL_MAX_RADIUS 6
#define ICPK_BILATERAL_MAX_RANGE 4096
typedef struct icpk_bilateral_params {
  int32_t radius;       /* 1 .. ICPK_BILATERAL_MAX_RADIUS (3) */
  float sigma_space;    /* pixels (2.0) */
  float sigma_range;    /* depth units (30) */
  int32_t range_cutoff; /* 0: floor(3 sigma_range) + 1 (0) */
} icpk_bilateral_params;
void icpk_default_bilateral_params(icpk_bilateral_params *p);
int icpk_bilateral_depth_image(icpk_ctx *ctx, const icpk_bilateral_params *params, const uint16_t *depth_in,
                               uint16_t *depth_out, int32_t rows, int32_t cols);
int icpk_backproject_smoothed(icpk_ctx *ctx, const uint16_t *depth, int32_t rows, int32_t cols, float fx, float cx,
                              const float offset[3], int32_t which, int32_t normals_mode,
                              const icpk_bilateral_params *params);
int icpk_bilateral_tables(const icpk_bilateral_params *params, uint16_t *ws, uint16_t *wr, int32_t *K);
int icpk_bilateral_host(const icpk_bilateral_params *params, const uint16_t *depth_in, int32_t rows, int32_t cols,
                        uint16_t *depth_out);

/* ---- K24: a depth pyramid on the device, for coarse-to-fine tracking ------------------------------------------------
 * KinectFusion's second stage: the frame at half and a quarter of its size, so that the first iterations of an
 * alignment run on a sixteenth of the points through a wide gate and only the last ones on the full frame through a
 * tight one.  The pyramid stays on the device; each level is back-projected from where it lies.
 *
 * THE PYRAMID RULE (icpk_depth_pyramid_build; integers only, so the result is a function of the image and K alone:
 * tile shape, tap order and who computes it do not matter).
 *   Parameters (icpk_pyramid_params; defaults from icpk_default_pyramid_params):
 *     levels        1 .. ICPK_PYRAMID_MAX_LEVELS (3): the number of images, level 0 included
 *     range_cutoff  K, 1 .. 65536 (91, the K of the bilateral defaults)
 *   Level 0 is the input image, uint16, 0 a hole.  Level l + 1 has (rows_l + 1) / 2 by (cols_l + 1) / 2 pixels; a level
 *   that has shrunk to 1 x 1 stays 1 x 1.
 *   Pixel (r, c) of level l + 1 is centred on pixel (2 r, 2 c) of level l, of depth d_c; that pixel is always inside
 *   the image.
 *     d_c == 0 gives 0.
 *     Otherwise tap (dy, dx) in {-1, 0, 1}^2 counts iff (2 r + dy, 2 c + dx) lies inside the image, its depth d_q != 0
 *     and |d_q - d_c| < K.  Its weight is w = (2 - |dy|)(2 - |dx|): 1, 2 or 4.
 *     S = sum w (4 .. 16), D = sum w (d_q - d_c);  out = d_c + floor((2 D + S) / (2 S)), floor towards minus infinity:
 *     the weighted mean, rounded to nearest, halves up.
 *   Consequences:
 *     the validity mask of a level is the mask of the level below, subsampled exactly (out != 0 iff d_c != 0);
 *     |out - d_c| <= K - 1;
 *     K == 1 is plain subsampling: level l + 1 is level l at its even rows and columns;
 *     a depth step of K or more is never averaged across.
 *   The window is symmetric about the centre pixel, so pixel (r, c) of level l IS pixel (r 2^l, c 2^l) of level 0, and
 *   the level's intrinsics are fx / 2^l and cx / 2^l, both exact in float.  (A rule that averages the 2 x 2 block, with
 *   block-centre intrinsics, is biased towards one corner by any range gate wherever the depths of one block differ by
 *   more than K, as on a slanted floor; the centred window is not.)  On the noiseless 120 x 160 room of
 *   synth.render_room_depth (fx, cx = 117.15, 79.5), against a direct render at the level's shape and intrinsics:
 *   K = 1 gives the render exactly at levels 1 and 2; K = 91 differs by at most 36 units at level 1 and 29 at level 2.
 *
 * icpk_depth_pyramid_build     depth: a host image of rows x cols.  params NULL: the defaults.  smooth NULL: level 0 is
 *     the frame as given, uploaded straight into the pyramid; otherwise level 0 is the frame after K22 with these
 *     parameters (the upload then goes through the image buffers icpk_backproject_pair keeps its resident frame in,
 *     and, as after icpk_bilateral_depth_image, no frame is resident afterwards).  The call touches no cloud, no
 *     association and no seed; when it returns the caller's image has been consumed.  The pyramid replaces the previous
 *     one and stays resident until the next build; it is freed with the context.
 * icpk_depth_pyramid_shape     rows, cols of a level (either may be NULL).
 * icpk_depth_pyramid_get       out: a host array of the level's rows x cols.
 * icpk_depth_pyramid_backproject  fx, cx: the LEVEL-0 intrinsics.  In every effect on the context it equals
 *     icpk_backproject (normals_mode < 0) or icpk_backproject_with_normals (normals_mode >= 0, which must be 1) of
 *     icpk_depth_pyramid_get(level) at (fx / 2^level, cx / 2^level): the cloud, the normals, the subsample key it draws,
 *     the associations and seeds it drops, the resident frame it gives up.  Returns the number of points.
 * icpk_depth_pyramid_host      host only: level `level` of the pyramid of depth_in, through the header the kernel
 *     includes (csrc/pyramid_rule.h), into out, a host array of exactly that level's size.
 * ICPK_E_NOT_SET: shape, get or backproject before the first build.
 * Refusals (ICPK_E_ARG; a refused call leaves the context, its clouds, the pyramid and the output array as they were):
 *     a NULL context or image; rows or cols < 1, or more than 2^28 pixels; levels outside 1 .. ICPK_PYRAMID_MAX_LEVELS;
 *     range_cutoff outside 1 .. 65536; bilateral parameters THE BILATERAL RULE refuses; a level the pyramid does not
 *     have; for icpk_depth_pyramid_backproject also `which` outside 0 / 1, normals_mode >= 0 with which == 0, and a
 *     normals_mode icpk_backproject_with_normals does not know. */
#define ICPK_PYRAMID_MAX_LEVELS 8
typedef struct icpk_pyramid_params {
  int32_t levels;       /* 1 .. ICPK_PYRAMID_MAX_LEVELS (3) */
  int32_t range_cutoff; /* K: 1 .. 65536 (91) */
} icpk_pyramid_params;
void icpk_default_pyramid_params(icpk_pyramid_params *p);
int icpk_depth_pyramid_build(icpk_ctx *ctx, const uint16_t *depth, int32_t rows, int32_t cols,
                             const icpk_pyramid_params *params, const icpk_bilateral_params *smooth);
int icpk_depth_pyramid_shape(icpk_ctx *ctx, int32_t level, int32_t *rows, int32_t *cols);
int icpk_depth_pyramid_get(icpk_ctx *ctx, int32_t level, uint16_t *out);
int icpk_depth_pyramid_backproject(icpk_ctx *ctx, int32_t level, float fx, float cx, const float offset[3],
                                   int32_t which, int32_t normals_mode);
int icpk_depth_pyramid_host(const icpk_pyramid_params *params, const uint16_t *depth_in, int32_t rows, int32_t cols,
                            int32_t level, uint16_t *out);

/* ---- K25: projective frame-to-model alignment on the resident depth pyramid ----------------------------------------
 * KinectFusion's data association: a pixel of the frame is paired with the pixel of the ray-cast view of the model it
 * projects onto.  A pixel that projects outside the view, or onto a hole of it, has no pair, so nothing pairs with
 * the view's border.  Both inputs lie on the device already -- a level of the pyramid (K24) and the eight planes of the
 * last ray cast (K20) -- and no list, no index and no search is made.
 *
 * THE PROJECTIVE RULE.  float32; every operation rounded once, in the order written (fl(.) is one rounding); no fused
 * multiply-add; correctly rounded / and sqrt; a floor is a comparison plus a truncating conversion of a value already
 * known to be in range.
 *   Inputs:
 *     level l of the resident pyramid, rows_s x cols_s, uint16, seen through fx_s = fx / 2^l, cx_s = cx / 2^l (fx, cx:
 *       the LEVEL-0 intrinsics of icpk_projective_params, as for icpk_depth_pyramid_backproject);
 *     the planes x, y, z, nx, ny, nz, depth of the last icpk_tsdf_raycast (rows_v x cols_v; the shape need not equal the
 *       level's) with that ray cast's own fx_v, cx_v and pose P_v, which the context keeps next to the maps;
 *     an estimate E, double[16], camera-to-world: its nine R and three t rounded to float once;
 *     (Q, s) = P_v inverted by icpk_tsdf_invert_pose.
 *   Source pixel i = r cols_s + c; the first failing test decides its code (ICPK_PROJ_*, negative):
 *     1. d == 0: NO_DEPTH.
 *     2. the vertex, K4's arithmetic: v_z = fl((float)d / 5000.0f), v_x = fl(fl(fl((float)c - cx_s) v_z) / fx_s),
 *        v_y = fl(fl(fl((float)r - cx_s) v_z) / fx_s)   (cx_s for the rows as well).
 *     3. the world point: p_a = fl(fl(fl(fl(E_a0 v_x) + fl(E_a1 v_y)) + fl(E_a2 v_z)) + t_a)   (integration rule 2's form).
 *     4. q = the same form with (Q, s) and p.  !(q_z > 0): BEHIND.
 *     5. u = fl(fl(fl(q_x fx_v) / q_z) + cx_v), v = fl(fl(fl(q_y fx_v) / q_z) + cx_v); a = fl(u + 0.5f), b = fl(v + 0.5f);
 *        !(a >= 0 && a < (float)cols_v && b >= 0 && b < (float)rows_v): OUTSIDE (in float, before any conversion; NaN
 *        fails).  col = (int)a, row = (int)b.
 *     6. j = row cols_v + col; !(depth_v[j] > 0): NO_MODEL.
 *     7. e_a = fl(p_a - m_a), m = (x, y, z)[j]; dist = sqrt(fl(fl(fl(e_x e_x) + fl(e_y e_y)) + fl(e_z e_z)));
 *        !(dist < max_dist): TOO_FAR.
 *     8. only when min_normal_cos > -1 (default -2: off): s = the ICPK_NORMALS_CROSS normal of pixel (r, c) of the level
 *        through (fx_s, cx_s); zero (a border pixel, a hole among the four neighbours, a zero cross product): NO_NORMAL.
 *        s is negated when fl(fl(fl(s_x v_x) + fl(s_y v_y)) + fl(s_z v_z)) > 0 (the cross normal points away from the
 *        camera, the model's normals towards it), rotated by E's R in the 3-term form (a0 b0 + a1 b1) + a2 b2, and
 *        cosv = its 3-term dot with (nx, ny, nz)[j]; !(cosv >= min_normal_cos): NORMAL.
 *     9. accepted: the pair (i, j, dist).  Its terms are K5's with p, m, n = (nx, ny, nz)[j] widened to double:
 *        J = [p x n ; n], r = (p - m) . n, in the ICPK_NP2L layout with [27] = (double)dist.  A pixel without a pair adds
 *        +0.0.  The sums go through the canonical tree (ICPK_RED_THREADS / ICPK_RED_MAX_BLOCKS) over i = 0 ..
 *        rows_s cols_s - 1; the count is an exact integer.
 *   The loop (icpk_align_projective): E_0 = the given pose.  Iteration k: sums and count at E_k; count < min_pairs stops
 *   with ICPK_W_TOO_FEW_PAIRS and E stays; a solve (icpk_solve_point_to_plane) that fails stops with ICPK_W_DEGENERATE
 *   and E stays; otherwise E_{k+1} = dT E_k in double: R' = dR R with 3-term products,
 *   t'_r = ((dR_r0 t_0 + dR_r1 t_1) + dR_r2 t_2) + dt_r.  Exactly max_iterations iterations run otherwise: there is no
 *   threshold test.  No working source is moved: every iteration recomputes the vertices from the level and E_k.
 *   The gate must be wider than the frame's displacement: a wall that slides sideways is at nearest-neighbour distance
 *   0 but at projective distance equal to the slide.  Hence the default of 0.5 m.
 *
 * icpk_projective_associate  per source pixel, at `pose`: pixel[i] = j or the code, dist[i] = the distance (0 without a
 *     pair).  Host arrays of rows_s cols_s entries; either may be NULL.
 * icpk_projective_reduce     one evaluation at `pose`: the ICPK_NP2L sums and the count.
 * icpk_align_projective      the loop; pose_out (double[16], last row 0 0 0 1) is the last estimate.  The result's count
 *     and mean_dist (sums[27] / count, 0 for no pair) are those of the LAST EVALUATED iteration, i.e. taken at the
 *     estimate before the last update, not at pose_out.  iterations: the updates made.  Returns the status.
 * icpk_get_projective_trace  the evaluated iterations of the last icpk_align_projective, at most cap of them: E_k, the
 *     sums and count at E_k, and ICPK_OK or the warning that stopped the loop there.  Returns their number.
 * icpk_projective_pixels     host only, no context: rules 1 - 9 for `count` source pixels from pixel `first` over a host
 *     level (rows_s x cols_s: the level's own shape; params->level only scales fx, cx) and seven host planes view[0..6]
 *     = x, y, z, nx, ny, nz, depth of rows_v x cols_v.  pixel / dist: count entries; terms (or NULL): count x ICPK_NP2L
 *     doubles, zeros for a pixel without a pair.  Returns the number of pairs.  Compiled from the header the kernel
 *     includes (csrc/projective_rule.h).
 * None of these calls touches the context's source, target, associations, records, seeds, surface list or ray-cast
 * maps; they use scratch of their own.
 * ICPK_E_NOT_SET: no volume, no ray cast (as icpk_tsdf_get_raycast), or no pyramid.
 * Refusals (ICPK_E_ARG; a refused call leaves everything as it was): a NULL or non-finite pose; a level the pyramid
 *     lacks; fx not finite and > 0; a non-finite cx; max_dist not > 0; min_pairs < 1; max_iterations outside
 *     1 .. ICPK_PROJECTIVE_MAX_ITERATIONS; a NaN min_normal_cos. */
#define ICPK_PROJECTIVE_MAX_ITERATIONS 64
#define ICPK_PROJ_NO_DEPTH (-1)
#define ICPK_PROJ_BEHIND (-2)
#define ICPK_PROJ_OUTSIDE (-3)
#define ICPK_PROJ_NO_MODEL (-4)
#define ICPK_PROJ_TOO_FAR (-5)
#define ICPK_PROJ_NO_NORMAL (-6)
#define ICPK_PROJ_NORMAL (-7)
typedef struct icpk_projective_params {
  int32_t level;          /* of the resident pyramid (0) */
  float fx, cx;           /* LEVEL-0 intrinsics (468.60, 318.27) */
  int32_t max_iterations; /* 1 .. ICPK_PROJECTIVE_MAX_ITERATIONS (10) */
  float max_dist;         /* the gate, metres (0.5) */
  float min_normal_cos;   /* > -1: the normal gate (-2: off) */
  int32_t min_pairs;      /* >= 1 (6) */
} icpk_projective_params;
typedef struct icpk_projective_result {
  int32_t status;     /* ICPK_OK, ICPK_W_TOO_FEW_PAIRS, ICPK_W_DEGENERATE */
  int32_t iterations; /* updates made */
  int64_t count;      /* pairs of the last evaluated iteration ... */
  double mean_dist;   /* ... and their mean distance */
} icpk_projective_result;
typedef struct icpk_projective_iter {
  double pose[12];         /* E_k: rows of [R | t] */
  double sums[ICPK_NP2L];  /* at E_k */
  int64_t count;
  int32_t status;
  int32_t reserved;
} icpk_projective_iter;
void icpk_default_projective_params(icpk_projective_params *p);
int icpk_projective_associate(icpk_ctx *ctx, const icpk_projective_params *params, const double pose[16],
                              int32_t *pixel, float *dist);
int icpk_projective_reduce(icpk_ctx *ctx, const icpk_projective_params *params, const double pose[16],
                           double sums[ICPK_NP2L], int64_t *count);
int icpk_align_projective(icpk_ctx *ctx, const icpk_projective_params *params, const double pose_in[16],
                          double pose_out[16], icpk_projective_result *result);
int icpk_get_projective_trace(icpk_ctx *ctx, icpk_projective_iter *out, int32_t cap);
int icpk_projective_pixels(const icpk_projective_params *params, const double pose[16], const uint16_t *level,
                           int32_t rows_s, int32_t cols_s, const float *const view[7], int32_t rows_v, int32_t cols_v,
                           float fx_v, float cx_v, const double view_pose[16], int64_t first, int32_t count,
                           int32_t *pixel, float *dist, double *terms);

/* ---- K26: the photometric term in projective frame-to-model alignment ------------------------------------------------
 * K25 is purely geometric: a wall, a floor or a table top leaves the in-plane motion free, and on an exact plane its
 * 6x6 is singular.  K26 adds K17's photometric term to it.  It needs three things beside K25's inputs: an intensity
 * per pixel of the pyramid level, the intensity of the ray-cast view (plane 8 of K20's maps, from a volume with
 * ICPK_TSDF_COLOR), and the gradient of that intensity over the view's surface.
 *
 * THE INTENSITY PYRAMID RULE (icpk_depth_pyramid_set_intensity; integers up to one final division, so the result is a
 * function of the two images and K alone).  K is the range_cutoff the resident depth pyramid was built with.
 *   Level 0 is the input image: one float in [0, 1] per pixel of depth level 0.
 *   Pixel (r, c) of level l + 1 is 0.0 where pixel (r, c) of depth level l + 1 is 0, i.e. where d_c, the depth of pixel
 *   (2 r, 2 c) of level l, is 0.
 *   Otherwise the taps that count are exactly those that count in THE PYRAMID RULE at that pixel: (2 r + dy, 2 c + dx)
 *   inside the image, d_q != 0 and |d_q - d_c| < K, d the DEPTH level l; the weights are the same,
 *   w = (2 - |dy|)(2 - |dx|).
 *     c_q = (int32)rint((double)I_q * 32768.0), I_q the intensity of level l at the tap (rint: to nearest, ties to even);
 *     N = sum w c_q (int32: at most 16 * 32768), S = sum w (4 .. 16);
 *     out = (float)((double)N / ((double)S * 32768.0)).
 *   Consequences: a depth step of K or more is never averaged across in intensity either; the validity mask is the
 *   depth level's mask; K == 1 is plain subsampling up to the quantisation (out = (float)(c_q / 32768.0) of the centre)
 *   wherever no other tap has the centre's very depth -- with K == 1 a tap counts iff its depth equals the centre's,
 *   which averages the depth to itself but not the intensity; the result lies in [0, 1].
 * icpk_depth_pyramid_set_intensity  after icpk_depth_pyramid_build: a host image of level 0's shape (else ICPK_E_ARG;
 *     ICPK_E_NOT_SET without a pyramid), every value finite and in [0, 1] (a host scan before the upload, else ICPK_E_ARG
 *     and nothing changes).  It builds every level the depth pyramid has, one launch per level (the launch runs once per
 *     frame; see csrc/kernels_pyramid_color.hip), from the depth levels as they lie on the device -- after a build with
 *     `smooth` those are the smoothed depths; the intensity is never smoothed.  The next icpk_depth_pyramid_build drops
 *     the intensity levels.
 * icpk_depth_pyramid_get_intensity  out: a host array of the level's rows x cols floats; ICPK_E_NOT_SET without
 *     intensity levels, ICPK_E_ARG for a level the pyramid lacks.
 * icpk_intensity_pyramid_host       host only: level `level` of the intensity pyramid of (depth_in, intensity_in), the
 *     depth pyramid taken without smoothing, through the header the kernel includes (csrc/pyramid_rule.h), into out, a
 *     host array of exactly that level's size.  Refusals as icpk_depth_pyramid_host's, and an intensity outside [0, 1].
 *
 * THE VIEW GRADIENT RULE (icpk_tsdf_raycast_color_gradients) is K17's gradient rule with the neighbourhood replaced.
 *   Pixel j = (r, c) of the last ray cast has a gradient only where depth[j] > 0.  Its point is (x, y, z)[j], its normal
 *   n = (nx, ny, nz)[j], its intensity I_j = intensity[j].
 *   neighbourhood  the view pixels q = (r + dy, c + dx), dy, dx in {-1, 0, 1}, that lie inside the view, have
 *                  depth[q] > 0, and whose distance to pixel j's point in the form of projective rule 7 -- float32:
 *                  f_a = fl(p_q,a - p_j,a), d = sqrt(fl(fl(fl(f_x f_x) + fl(f_y f_y)) + fl(f_z f_z))) -- is <= radius
 *                  (a float compare; NaN fails).  Pixel j itself counts.  m = the neighbourhood's size (1 .. 9).
 *   From there on the rule is K17's, word for word (colored ICP above), F = 2^15, r = radius:
 *   usable normal  nn = (n_0 n_0 + n_1 n_1) + n_2 n_2 in float64 lies in [1 - 2^-10, 1 + 2^-10] (false for NaN).
 *   per neighbour  (only with a usable normal) float64, one rounded operation per symbol, none fused:
 *                    e_a = (double)p_q,a - (double)p_j,a;   h = (e_0 n_0 + e_1 n_1) + e_2 n_2;   u_a = e_a - h n_a
 *                    q_a = (int64)rint((u_a / r) F);        c = (int64)rint(((double)I_q - (double)I_j) F)
 *   sums           int64: S_ab = sum q_a q_b (a <= b), T_a = sum q_a c; ten words per pixel: m, S_00 S_01 S_02 S_11 S_12
 *                  S_22, T_0 T_1 T_2; all nine sums zero without a usable normal, m kept; all ten zero for a non-hit
 *                  pixel.  The distance test bounds |e| by the radius, so K17's overflow argument carries over (|q| <=
 *                  2^15 + 2^7, and m <= 9).  The ray cast's intensity is a lerp of values in [0, 1], so |c| <= 2^15.
 *   solve          float64: w = (double)m F, w2 = w w, H_ab = (double)S_ab + (w2 n_a) n_b; the adjugate K of H and det as
 *                  K14 writes them (K_00 = H_11 H_22 - H_12 H_12, K_01 = H_02 H_12 - H_01 H_22, K_02 = H_01 H_12 -
 *                  H_02 H_11, K_11 = H_00 H_22 - H_02 H_02, K_12 = H_01 H_02 - H_00 H_12, K_22 = H_00 H_11 - H_01 H_01,
 *                  det = (H_00 K_00 + H_01 K_01) + H_02 K_02), inv = 1.0 / det,
 *                  g'_a = ((K_a0 T_0 + K_a1 T_1) + K_a2 T_2) inv, gradient_a = (float)(g'_a / r): intensity per metre.
 *   no gradient    (0, 0, 0) when m < min_neighbors, without a usable normal, when det is not finite or <= 0, or when
 *                  a component of the result is not finite.  Every non-hit pixel gets (0, 0, 0).
 * icpk_tsdf_raycast_color_gradients  stream-ordered, no host wait: three float planes gx, gy, gz of the last ray cast's
 *     shape, kept by the context behind the maps.  flags: ICPK_COLOR_KEEP_SUMS keeps the ten int64 per pixel.
 *     ICPK_E_NOT_SET without a volume or a ray cast; ICPK_E_ARG on a volume without ICPK_TSDF_COLOR, for a radius that is
 *     not finite and > 0, min_neighbors < 1 or an unknown flag (nothing changes).  The next icpk_tsdf_raycast drops the
 *     gradients and the kept sums, and so does everything that drops the maps.
 * icpk_tsdf_get_raycast_color_gradients      three host planes of rows x cols floats (any may be NULL); ICPK_E_NOT_SET
 *     without gradients of the current ray cast.
 * icpk_tsdf_get_raycast_color_gradient_sums  10 int64 per pixel, pixel-major; ICPK_E_NOT_SET without the flag.
 * icpk_raycast_color_gradients_host  host only, no context: the rule for `count` pixels from row-major pixel `first`
 *     over eight host planes view[0..7] = x, y, z, nx, ny, nz, depth, intensity of rows x cols.  sums (or NULL): count x
 *     10 int64; g (or NULL): count x 3 floats, (gx, gy, gz) per pixel.  Returns the number of pixels with a non-zero
 *     gradient.  Compiled from the header the kernel includes (csrc/raycast_color_rule.h).
 *
 * THE COLOURED PROJECTIVE RULE.  Rules 1 - 8 of THE PROJECTIVE RULE decide the pair, unchanged: the coloured path accepts
 * exactly the pixels K25 accepts, so counts, codes and [27] are K25's.  Rule 9 becomes K17's joint terms, float64,
 * unfused, lg = (double)lambda_geometric, lc = 1.0 - lg.  With p the world point of rule 3, q = m = (x, y, z)[j],
 * n = (nx, ny, nz)[j], g the view gradient at j, I_t = intensity_v[j] and I_s the intensity level's pixel i, all widened:
 *   geometric   e_a = p_a - q_a;  h = (e_0 n_0 + e_1 n_1) + e_2 n_2;  G = [p x n | n]
 *   photometric u_a = e_a - h n_a;  rc = (I_t + ((g_0 u_0 + g_1 u_1) + g_2 u_2)) - I_s;
 *               gn = (g_0 n_0 + g_1 n_1) + g_2 n_2;  M_a = g_a - gn n_a;  C = [p x M | M]
 *   sums        [0..20] += lg (G_a G_b) + lc (C_a C_b) (a <= b, row-major), [21..26] += lg (G_a h) + lc (C_a rc),
 *               [27] += (double)dist, through the canonical tree over the pixel index.
 * lambda_geometric = 1 gives icpk_projective_reduce's sums bit for bit.  A zero gradient removes a pair's photometric
 * term, not the pair.  The loop is THE PROJECTIVE RULE's loop exactly: the same state, the same step launch,
 * 2 max_iterations launches enqueued up front, one copy and one wait, the same stop rules and the same
 * icpk_get_projective_trace; only the reduce launch differs.
 * icpk_projective_reduce_colored / icpk_align_projective_colored  as their K25 namesakes; color NULL: the defaults.
 *     ICPK_E_ARG for a lambda_geometric that is not finite and in [0, 1] and on a volume without ICPK_TSDF_COLOR;
 *     ICPK_E_NOT_SET without an intensity pyramid or without view gradients for the current ray cast; everything K25
 *     refuses is refused the same way, first.  None of these calls touches source, target, associations, records,
 *     seeds, surface list, maps, pyramid or volume.
 * icpk_projective_pixels_colored  host only: icpk_projective_pixels with the coloured rule 9; level_intensity: rows_s x
 *     cols_s floats, view_intensity and gradient[0..2] = gx, gy, gz: rows_v x cols_v floats each. */
typedef struct icpk_projective_color_params {
  float lambda_geometric; /* [0, 1] (0.968) */
} icpk_projective_color_params;
void icpk_default_projective_color_params(icpk_projective_color_params *c);
int icpk_depth_pyramid_set_intensity(icpk_ctx *ctx, const float *intensity, int32_t rows, int32_t cols);
int icpk_depth_pyramid_get_intensity(icpk_ctx *ctx, int32_t level, float *out);
int icpk_intensity_pyramid_host(const icpk_pyramid_params *params, const uint16_t *depth_in, const float *intensity_in,
                                int32_t rows, int32_t cols, int32_t level, float *out);
int icpk_tsdf_raycast_color_gradients(icpk_ctx *ctx, float radius, int32_t min_neighbors, int32_t flags);
int icpk_tsdf_get_raycast_color_gradients(icpk_ctx *ctx, float *gx, float *gy, float *gz);
int icpk_tsdf_get_raycast_color_gradient_sums(icpk_ctx *ctx, int64_t *sums);
int icpk_raycast_color_gradients_host(const float *const view[8], int32_t rows, int32_t cols, float radius,
                                      int32_t min_neighbors, int64_t first, int32_t count, int64_t *sums, float *g);
int icpk_projective_reduce_colored(icpk_ctx *ctx, const icpk_projective_params *params,
                                   const icpk_projective_color_params *color, const double pose[16],
                                   double sums[ICPK_NP2L], int64_t *count);
int icpk_align_projective_colored(icpk_ctx *ctx, const icpk_projective_params *params,
                                  const icpk_projective_color_params *color, const double pose_in[16],
                                  double pose_out[16], icpk_projective_result *result);
int icpk_projective_pixels_colored(const icpk_projective_params *params, const double pose[16], const uint16_t *level,
                                   int32_t rows_s, int32_t cols_s, const float *const view[7], int32_t rows_v,
                                   int32_t cols_v, float fx_v, float cx_v, const double view_pose[16], int64_t first,
                                   int32_t count, int32_t *pixel, float *dist, double *terms,
                                   const float *level_intensity, const float *view_intensity,
                                   const float *const gradient[3], const icpk_projective_color_params *color);

/* ---- K27: fern keyframe relocalisation ------------------------------------------------------------------------------
 * A tracker that has lost the camera (a covered lens, a fast turn, dropped frames) finds it again by looking the frame
 * up among keyframes it harvested while it tracked (Glocker et al., "Real-time RGB-D camera relocalization via
 * randomized ferns for keyframe encoding").  A frame is a short binary code of a coarse level of the resident pyramid
 * (K24); the database of codes lies on the device, the pose of every keyframe on the host beside it.
 *
 * THE FERN RULE (integers only, so a code is a function of the level and the parameters alone and a search's answer a
 * function of the codes alone: block shape, and which thread looked at which keyframe, do not matter).
 *   Parameters (icpk_fern_params; defaults from icpk_default_fern_params):
 *     level          a level of the resident pyramid (2)
 *     n_ferns        F, a multiple of 8 in 8 .. ICPK_FERN_MAX_FERNS (256)
 *     seed           uint64 (27)
 *     d_min, d_max   uint16 depth units, 0 <= d_min < d_max <= 65535 (1000, 20000)
 *     capacity       1 .. ICPK_FERN_MAX_KEYFRAMES keyframes (4096)
 *     harvest_above  0 .. F (F / 5 = 51)
 *     min_valid      0 .. F (F / 2 = 128)
 *   The table is a function of the parameters and the level's shape rows x cols.
 *     draw(f, j) = (uint32)(mix(seed + (f + 1) * 0x9E3779B97F4A7C15 + j * 0xD1B54A32D192ED03) >> 32), mod 2^64, mix being
 *     icpk_set_subsample's finaliser (z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
 *     z ^= z >> 31).
 *     Fern f tests pixel (draw(f, 0) % rows, draw(f, 1) % cols); its thresholds are
 *     tau_k = d_min + draw(f, 2 + k) % (d_max - d_min), k = 0 .. 3.
 *   The code comes from the depth d of that pixel in the level (0 a hole):
 *     nibble n_f has bit k set iff d > tau_k (strict); a hole gives 0;
 *     V = the number of ferns with d != 0;
 *     packed: word w of F / 8 uint32 words holds fern 8 w + j in bits 4 j .. 4 j + 3.
 *   Dissimilarity: diss(a, b) = the number of ferns whose nibbles differ, 0 .. F.  On packed words:
 *     x = a ^ b; x |= x >> 1; x |= x >> 2; popcount(x & 0x11111111), summed over the words.
 *   Search: for a query code and keyframes 0 .. n - 1 the answer is the min(k, n) keyframes in ascending (diss, index)
 *     order; ties go to the lower index.
 *   Harvest: a frame's code becomes keyframe n iff V >= min_valid, n < capacity, and n == 0 or its smallest
 *     dissimilarity to the database exceeds harvest_above.
 *
 * A context holds one database and one "current code", the code of the last encode; both stay on the device.
 * icpk_fern_create        rows, cols: the shape of the level that will be encoded.  params NULL: the defaults.  Replaces
 *     any previous database of the context; the memory for `capacity` keyframes is taken here (65536 keyframes of 1024
 *     ferns: 32 MB, the largest).
 * icpk_fern_reset         empties the database.      icpk_fern_destroy  frees it.
 * icpk_fern_count         the number of keyframes (>= 0), or a negative status.
 * icpk_fern_encode        level params.level of the resident pyramid into the current code; code_out (F / 8 words) and
 *     valid_out may be NULL.
 * icpk_fern_query         the search with the current code: index_out, diss_out (k entries each), *n_out = min(k, n).
 * icpk_fern_add           appends the current code unconditionally, with its pose (camera-to-world, double[16]).
 * icpk_fern_process       the per-frame call: encode, search and -- when pose is not NULL and the harvest rule says so --
 *     append; *added_out is the new index or -1 (valid_out, added_out may be NULL).  The search it reports is the one
 *     BEFORE the append.  Three launches (encode, search, merge), one copy, one host wait, no host round trip between
 *     the launches; an append is a fourth launch nobody waits for.
 * icpk_fern_add_code      appends a host code (F / 8 words): restores a saved database.
 * icpk_fern_get_keyframe  one keyframe back: code_out (F / 8 words) and pose_out (double[16]), either may be NULL.
 * icpk_fern_table, icpk_fern_encode_host, icpk_fern_dissimilarity_host  host only, no context, no device, through the
 *     header the kernels include (csrc/fern_rule.h): the table as F x 6 int32 (row, col, tau_0 .. tau_3); the code and V
 *     of a host level of rows x cols; diss(a, b), >= 0 (or ICPK_E_ARG).  params NULL: the defaults.
 * No fern call touches the context's clouds, associations, records, seeds, surface list, ray-cast maps, the pyramid or
 * its intensity.  A pyramid build does not touch the database: it only invalidates the current code.
 * ICPK_E_NOT_SET: no database; no pyramid; no current code, or one that dates from before the last pyramid build.
 * Refusals (ICPK_E_ARG; a refused call leaves everything as it was): NULL arguments; parameters outside the ranges
 *     above; rows or cols < 1 or more than 2^28 pixels; a level the pyramid lacks; a resident level whose shape is not
 *     the database's; k outside 1 .. ICPK_FERN_MAX_K; a non-finite pose; an index outside 0 .. n - 1; icpk_fern_add /
 *     icpk_fern_add_code on a full database (icpk_fern_process on a full database adds nothing and is no error). */
#define ICPK_FERN_MAX_K 8
#define ICPK_FERN_MAX_FERNS 1024
#define ICPK_FERN_MAX_KEYFRAMES 65536
typedef struct icpk_fern_params {
  int32_t level;         /* of the resident pyramid (2) */
  int32_t n_ferns;       /* F: a multiple of 8 in 8 .. 1024 (256) */
  uint64_t seed;         /* (27) */
  int32_t d_min, d_max;  /* depth units (1000, 20000) */
  int32_t capacity;      /* keyframes: 1 .. 65536 (4096) */
  int32_t harvest_above; /* 0 .. F (F / 5) */
  int32_t min_valid;     /* 0 .. F (F / 2) */
  int32_t reserved;      /* 0 */
} icpk_fern_params;
void icpk_default_fern_params(icpk_fern_params *p);
int icpk_fern_create(icpk_ctx *ctx, const icpk_fern_params *params, int32_t rows, int32_t cols);
int icpk_fern_reset(icpk_ctx *ctx);
int icpk_fern_destroy(icpk_ctx *ctx);
int icpk_fern_count(icpk_ctx *ctx);
int icpk_fern_encode(icpk_ctx *ctx, uint32_t *code_out, int32_t *valid_out);
int icpk_fern_query(icpk_ctx *ctx, int32_t k, int32_t *index_out, int32_t *diss_out, int32_t *n_out);
int icpk_fern_add(icpk_ctx *ctx, const double pose[16], int32_t *index_out);
int icpk_fern_process(icpk_ctx *ctx, const double *pose, int32_t k, int32_t *index_out, int32_t *diss_out,
                      int32_t *n_out, int32_t *valid_out, int32_t *added_out);
int icpk_fern_add_code(icpk_ctx *ctx, const uint32_t *code, const double pose[16], int32_t *index_out);
int icpk_fern_get_keyframe(icpk_ctx *ctx, int32_t index, uint32_t *code_out, double *pose_out);
int icpk_fern_table(const icpk_fern_params *params, int32_t rows, int32_t cols, int32_t *table_out);
int icpk_fern_encode_host(const icpk_fern_params *params, const uint16_t *level, int32_t rows, int32_t cols,
                          uint32_t *code_out, int32_t *valid_out);
int icpk_fern_dissimilarity_host(const uint32_t *a, const uint32_t *b, int32_t n_ferns);

/* ---- K28: the frame view -- projective frame-to-frame odometry -----------------------------------------------------
 * K25 / K26 project a frame into "the view": eight planes x, y, z, nx, ny, nz, depth, intensity in world coordinates,
 * with a camera and a pose.  Until here the only view was the last ray cast of a TSDF volume.  The frame view is the
 * same eight planes made from a depth frame alone -- KinectFusion's frame-to-frame prediction, the vertex and normal
 * map of the previous frame --, one set per level of the resident pyramid (K24; with the intensities of K26 where the
 * pyramid carries them), kept as a snapshot the context owns so that the next frame's pyramid can overwrite the levels.
 * No volume is needed.
 *
 * THE FRAME VIEW RULE.  THE PROJECTIVE RULE's own arithmetic: float32; every operation rounded once, in the order
 * written (fl(.) is one rounding); no fused multiply-add; correctly rounded / and sqrt; no libm.
 *   Inputs: level l of the pyramid, rows x cols, uint16, seen through fx_l = fx / 2^l, cx_l = cx / 2^l (fx, cx: the
 *     LEVEL-0 intrinsics); a pose P, double[16], camera-to-world: its nine R and three t rounded to float once.
 *   Pixel (r, c), i = r cols + c, depth d:
 *     1. d == 0 (a hole): all eight planes hold 0 at i.
 *     2. the vertex, THE PROJECTIVE RULE's step 2: v_z = fl((float)d / 5000.0f),
 *        v_x = fl(fl(fl((float)c - cx_l) v_z) / fx_l), v_y = fl(fl(fl((float)r - cx_l) v_z) / fx_l).
 *     3. the normal: s = the ICPK_NORMALS_CROSS normal of pixel (r, c) of the level through (fx_l, cx_l), exactly
 *        THE PROJECTIVE RULE's step 8's.  Without one (a border pixel, a hole among the four neighbours, a zero cross
 *        product) all eight planes hold 0 at i and the pixel counts in n_no_normal: such a pixel can never be paired.
 *        s is negated when fl(fl(fl(s_x v_x) + fl(s_y v_y)) + fl(s_z v_z)) > 0, so that it faces the camera as a
 *        ray-cast normal does (a dot of exactly 0 leaves it).
 *     4. listed: (x, y, z)_a = fl(fl(fl(fl(R_a0 v_x) + fl(R_a1 v_y)) + fl(R_a2 v_z)) + t_a)   (step 3's form);
 *        (nx, ny, nz)_a = fl(fl(fl(R_a0 s_x) + fl(R_a1 s_y)) + fl(R_a2 s_z)); depth = v_z; intensity = the intensity
 *        pyramid's value at level l, pixel i, when the pyramid carries one, else 0.
 *   depth > 0 is the validity test, as for the ray cast.  n_valid counts the listed pixels.
 *   A consequence: with an estimate E == P, a listed pixel's world point (THE PROJECTIVE RULE's step 3) is the view's
 *   point bit for bit, so it pairs at distance exactly 0 whenever it projects onto itself.
 *
 * icpk_frame_view_build    snapshots every level the resident pyramid has, at `pose`, through (fx, cx).  One launch for
 *     all levels; buffers are reused while they fit.  n_valid / n_no_normal: one entry per level, or NULL; with both NULL
 *     the call does not wait.  A pyramid rebuilt afterwards leaves the snapshot as it was; so does every TSDF call.
 * icpk_frame_view_levels   the levels of the snapshot (0 without one).
 * icpk_frame_view_shape / icpk_frame_view_get   a level's shape; its planes into host arrays of rows cols floats (any
 *     may be NULL).
 * icpk_frame_view_release  drops the snapshot and its memory (icpk_destroy does too).
 * icpk_frame_view_color_gradients   THE VIEW GRADIENT RULE (K26), the same kernel, over the eight planes of one level;
 *     the three planes are kept beside that level until the next build.  flags must be 0.  No host wait.
 *     icpk_frame_view_get_color_gradients returns them.
 * icpk_projective_set_view  decides which planes icpk_projective_associate, icpk_projective_reduce,
 *     icpk_align_projective, icpk_projective_reduce_colored and icpk_align_projective_colored read (and so what
 *     icpk_get_projective_trace records).  ICPK_VIEW_RAYCAST (the default): the last ray cast, nothing changes, byte for
 *     byte; view_level is ignored.  ICPK_VIEW_FRAME: level view_level of the snapshot, with its own shape, fx / 2^view_level,
 *     cx / 2^view_level (the build's fx, cx) and the build's pose; the calls then need no volume.  The kernels are the
 *     same; they are handed other pointers.
 * icpk_frame_view_pixels   host only, no context: the rule for `count` pixels from row-major pixel `first` of a host
 *     image (rows x cols: the level's own shape; `level` only scales fx, cx).  intensity: the level's, or NULL.  out:
 *     8 x count floats, plane k at out + k count.  Returns the number of listed pixels; *n_no_normal (or NULL) the
 *     pixels of step 3.  Compiled from the header the kernel includes (csrc/frame_view_rule.h).
 * None of these calls touches the context's source, target, associations, seeds, surface list, ray-cast maps, pyramid
 * or fern database.
 * ICPK_E_NOT_SET: no pyramid (build); no snapshot, or a level it lacks (every other call, and the projective calls
 *     under ICPK_VIEW_FRAME); for the gradients and the coloured calls, a snapshot built without an intensity pyramid,
 *     no intensity pyramid, or no gradients of the level.
 * Refusals (ICPK_E_ARG; a refused call leaves everything as it was): a NULL or non-finite pose; fx not finite and > 0;
 *     a non-finite cx; an unknown `which`; a level outside 0 .. ICPK_PYRAMID_MAX_LEVELS - 1; radius not finite and > 0;
 *     min_neighbors < 1; flags != 0. */
#define ICPK_VIEW_RAYCAST 0
#define ICPK_VIEW_FRAME 1
int icpk_frame_view_build(icpk_ctx *ctx, float fx, float cx, const double pose[16], int32_t *n_valid,
                          int32_t *n_no_normal);
int icpk_frame_view_levels(icpk_ctx *ctx);
int icpk_frame_view_shape(icpk_ctx *ctx, int32_t level, int32_t *rows, int32_t *cols);
int icpk_frame_view_get(icpk_ctx *ctx, int32_t level, float *const planes[8]);
int icpk_frame_view_release(icpk_ctx *ctx);
int icpk_frame_view_color_gradients(icpk_ctx *ctx, int32_t level, float radius, int32_t min_neighbors, int32_t flags);
int icpk_frame_view_get_color_gradients(icpk_ctx *ctx, int32_t level, float *gx, float *gy, float *gz);
int icpk_projective_set_view(icpk_ctx *ctx, int32_t which, int32_t view_level);
int icpk_frame_view_pixels(float fx, float cx, int32_t level, const double pose[16], const uint16_t *depth,
                           const float *intensity, int32_t rows, int32_t cols, int64_t first, int32_t count, float *out,
                           int32_t *n_no_normal);

/* ---- K29: depth frames tracked directly against the TSDF, with no ray cast ------------------------------------------
 * Every tracker above reaches the volume through a ray cast: a march of up to N samples per view pixel, per level, per
 * frame, and a view that holds only what the last pose could see.  The volume already holds what an alignment needs at
 * any world point: the signed distance D to the surface, and its gradient, the surface normal there.  Direct alignment
 * against the distance field (Bylow, Sturm, Kerl, Kahl, Cremers: "Real-time camera tracking and 3D reconstruction using
 * signed distance functions", RSS 2013) minimises sum_i D(E v_i)^2 over the frame's pixels: no view, no pairs, no
 * search, sub-voxel residuals from the trilinear interpolant, and everything fused so far takes part.  With
 * n = grad D / |grad D| and r = D(p) the Gauss-Newton step is K5's point-to-plane step, term for term.
 *
 * THE SDF TRACKING RULE.  THE PROJECTIVE RULE's conventions: float32; every operation rounded once, in the order written
 * (fl(.) is one rounding); no fused multiply-add; correctly rounded / and sqrt; no libm.
 *   Inputs:
 *     level l of the resident pyramid, rows_s x cols_s, uint16, seen through fx_s = fx / 2^l, cx_s = cx / 2^l (fx, cx:
 *       the LEVEL-0 intrinsics of icpk_sdf_params);
 *     the volume's tsdf and weight planes, its dims, voxel and trunc, and its CURRENT origin (K23: the origin after every
 *       shift made so far, what icpk_tsdf_get_params returns);
 *     min_weight; an estimate E, double[16], camera-to-world: its nine R and three t rounded to float once.
 *   Source pixel i = r cols_s + c; the first failing test decides its code (ICPK_SDF_*, negative):
 *     1. d == 0: NO_DEPTH.
 *     2. the vertex v: THE PROJECTIVE RULE's step 2.
 *     3. the world point p: THE PROJECTIVE RULE's step 3.
 *     4. THE RAY RULE's SAMPLE cell at p (its rule 5): g_a = fl(fl(fl(p_a - origin_a) / voxel) - 0.5f);
 *        !(g_a >= 0 && g_a < (float)(dims_a - 1)) on any axis: OUTSIDE (NaN fails; no index is formed before all three
 *        axes have passed).  c_a = (int)g_a, w_a = fl(g_a - (float)c_a), at = c_x + dims_x (c_y + dims_y c_z).  Any of
 *        the eight corner weights < min_weight: UNKNOWN.
 *     5. f = THE RAY RULE's trilinear value over the eight corners e[x + 2 y + 4 z] with the fractions w;
 *        D = fl(f trunc).  !(fabsf(f) < max_abs_tsdf): TOO_FAR.  The default max_abs_tsdf is 1.0: a fully saturated
 *        sample, f == +-1 exactly, is rejected and nothing else is.
 *     6. the gradient of that interpolant inside the cell, from the same eight corners.  With
 *        lerp(u, v, w) = fl(u + fl(w fl(v - u))); c00, c10, c01, c11 = the four lerps along x the trilinear value forms
 *        (c_yz = lerp(e[2 y + 4 z], e[1 + 2 y + 4 z], w_x)); b0 = lerp(c00, c10, w_y), b1 = lerp(c01, c11, w_y);
 *        dx_yz = fl(e[1 + 2 y + 4 z] - e[2 y + 4 z]):
 *          g_x = lerp(lerp(dx00, dx10, w_y), lerp(dx01, dx11, w_y), w_z),
 *          g_y = lerp(fl(c10 - c00), fl(c11 - c01), w_z),
 *          g_z = fl(b1 - b0);
 *        len = sqrt(fl(fl(fl(g_x g_x) + fl(g_y g_y)) + fl(g_z g_z))); !(len > 0): NO_GRADIENT.  n = g / len: it points
 *        towards positive distance, towards the cameras, as every model normal here does.
 *     7. only when min_normal_cos > -1 (default -2: off): THE PROJECTIVE RULE's step 8 with n in place of the view's
 *        normal -- the cross normal of pixel (r, c), the flip, the 3-term rotation by E's R, the 3-term dot with n;
 *        NO_NORMAL and NORMAL.
 *     8. accepted.  The pixel's entry is `at`, the linear index of its cell's lowest corner: >= 0 and < 2^30.  Its
 *        terms are K5's with p and n widened to double and r = (double)D: J = [p x n ; n], in the ICPK_NP2L layout with
 *        [27] = (double)fabsf(D).  A rejected pixel adds +0.0.  The sums go through the canonical tree
 *        (ICPK_RED_THREADS / ICPK_RED_MAX_BLOCKS) over i = 0 .. rows_s cols_s - 1; the count is an exact integer.
 *   The loop (icpk_align_sdf) is THE PROJECTIVE RULE's loop, word for word: the same count < min_pairs
 *   (ICPK_W_TOO_FEW_PAIRS), the same ICPK_W_DEGENERATE, the same E_{k+1} = dT E_k in double, exactly max_iterations
 *   iterations, no threshold test.  The step launch is K25's own.
 *
 * icpk_sdf_associate  per source pixel, at `pose`: cell[i] = at or the code, value[i] = D (0 when rejected).  Host arrays
 *     of rows_s cols_s entries; either may be NULL.
 * icpk_sdf_reduce     one evaluation at `pose`: the ICPK_NP2L sums and the count.
 * icpk_align_sdf      the loop; pose_out (double[16], last row 0 0 0 1) is the last estimate.  The result is K25's:
 *     count and mean_dist (the mean |D|, 0 for no accepted pixel) are those of the LAST EVALUATED iteration.  Returns
 *     the status.
 * icpk_get_sdf_trace  the evaluated iterations of the last icpk_align_sdf, as icpk_get_projective_trace's.
 * icpk_sdf_pixels     host only, no context: rules 1 - 8 for `count` source pixels from pixel `first` over a host level
 *     (rows_s x cols_s: the level's own shape; params->level only scales fx, cx) and the host planes tsdf, weight of
 *     `volume` (its dims, voxel, trunc and the origin TO USE; one entry per voxel).  cell / value: count entries; terms
 *     (or NULL): count x ICPK_NP2L doubles, zeros for a rejected pixel.  Returns the number of accepted pixels.  Compiled
 *     from the header the kernel includes (csrc/sdf_track_rule.h).
 * The device calls use scratch and a trace of their own: they leave the ray-cast maps, the surface list, the mesh, the
 * frame view, the trace of the last icpk_align_projective, and the source, target and associations bit for bit.
 * ICPK_E_NOT_SET: no volume, or no pyramid.
 * Refusals (ICPK_E_ARG; a refused call leaves everything as it was): a NULL or non-finite pose; a level the pyramid
 *     lacks; fx not finite and > 0; a non-finite cx; min_pairs < 1; max_iterations outside
 *     1 .. ICPK_PROJECTIVE_MAX_ITERATIONS; a NaN min_normal_cos; max_abs_tsdf not in (0, 1] (NaN included); min_weight
 *     outside 1 .. 65535. */
#define ICPK_SDF_NO_DEPTH (-1)
#define ICPK_SDF_OUTSIDE (-2)
#define ICPK_SDF_UNKNOWN (-3)
#define ICPK_SDF_TOO_FAR (-4)
#define ICPK_SDF_NO_GRADIENT (-5)
#define ICPK_SDF_NO_NORMAL (-6)
#define ICPK_SDF_NORMAL (-7)
typedef struct icpk_sdf_params {
  int32_t level;          /* of the resident pyramid (0) */
  float fx, cx;           /* LEVEL-0 intrinsics (468.60, 318.27) */
  int32_t max_iterations; /* 1 .. ICPK_PROJECTIVE_MAX_ITERATIONS (10) */
  float max_abs_tsdf;     /* in (0, 1]: |f| must stay below it (1.0) */
  int32_t min_weight;     /* 1 .. 65535 (1) */
  float min_normal_cos;   /* > -1: the normal gate (-2: off) */
  int32_t min_pairs;      /* >= 1 (6) */
} icpk_sdf_params;
void icpk_default_sdf_params(icpk_sdf_params *p);
int icpk_sdf_associate(icpk_ctx *ctx, const icpk_sdf_params *params, const double pose[16], int32_t *cell,
                       float *value);
int icpk_sdf_reduce(icpk_ctx *ctx, const icpk_sdf_params *params, const double pose[16], double sums[ICPK_NP2L],
                    int64_t *count);
int icpk_align_sdf(icpk_ctx *ctx, const icpk_sdf_params *params, const double pose_in[16], double pose_out[16],
                   icpk_projective_result *result);
int icpk_get_sdf_trace(icpk_ctx *ctx, icpk_projective_iter *out, int32_t cap);
int icpk_sdf_pixels(const icpk_sdf_params *params, const icpk_tsdf_params *volume, const double pose[16],
                    const uint16_t *level, int32_t rows_s, int32_t cols_s, const float *tsdf, const uint16_t *weight,
                    int64_t first, int32_t count, int32_t *cell, float *value, double *terms);

/* ---- K31: an exact Euclidean distance map of the TSDF volume ---------------------------------------------------------
 * Everything above reads the truncation band, |sdf| <= trunc; outside it a voxel holds tsdf = 1 or nothing.  "How far
 * is this point from anything solid?" -- the question a planner, a collision checker or a clearance query asks -- has
 * no answer in a truncated field.  The distance map (an ESDF, as voxblox and nvblox keep beside their TSDF) answers it:
 * per voxel the exact Euclidean distance, in whole voxels squared, to the nearest voxel of the other kind.  It is an
 * integer result: any correct algorithm gives the same bytes.
 *
 * THE DISTANCE RULE.  Integers only, up to the metric value of step 4.
 *   Parameters (icpk_esdf_params): min_weight, max_distance (metres), flags (ICPK_ESDF_UNKNOWN_OCCUPIED).
 *   0. The radius R = floor((double)max_distance / (double)voxel), on the host.  1 <= R <= ICPK_ESDF_MAX_RADIUS, else
 *      ICPK_E_ARG: it is not clamped.
 *   1. The class of voxel v with value f and weight w (uint8): 0 UNKNOWN: w < min_weight.  1 FREE: w >= min_weight &&
 *      !(f < 0).  2 OCCUPIED: w >= min_weight && f < 0.  (The surface rule's sign convention.)
 *   2. The obstacle set O: the voxels of class 2; with ICPK_ESDF_UNKNOWN_OCCUPIED every voxel whose class is not 1.
 *      Outside the volume there are no voxels, neither in O nor outside it.
 *   3. The signed squared distance q(v) (int32); |v - u|^2 is the squared Euclidean distance of the integer indices.
 *        v not in O: q = +min over u in O of |v - u|^2 if that is <= R^2, else +ICPK_ESDF_FAR (an empty O: +FAR);
 *        v in O:     q = -min over u not in O of |v - u|^2 if that is <= R^2, else -ICPK_ESDF_FAR.
 *      q is never 0.
 *   4. The metric distance m(q) (float32, one rounding per operation, no fused multiply-add): a = (float)|q| (exact:
 *      |q| <= 2^20); s = sqrtf(a), correctly rounded -- for +-FAR s = (float)(R + 1) --; m = +-fl(fl(s - 0.5f) voxel).
 *      The half voxel puts the zero between a free voxel and its occupied neighbour.  m is a function of q, R and voxel
 *      alone and is not stored.
 *   5. counts[4] = {n_unknown, n_free, n_occupied, n_far}, int64; n_far counts the voxels with |q| == FAR.
 *
 * THE QUERY RULE, for a world point p:
 *   THE RAY RULE's SAMPLE cell at p (its rule 5), read with the volume's CURRENT origin (K23).  Out of range, NaN
 *   included: dist = 0, grad = 0, status = 0x80.  Otherwise e[k] = m(q(corner k)) in the ray rule's corner order
 *   e[x + 2 y + 4 z]; dist = the ray rule's trilinear value of e at the fractions w; grad_a = fl(g_a / voxel) with g
 *   THE SDF TRACKING RULE's gradient (its rule 6) of the same e and w.  Status bit 0: a corner is FAR; bit 1: a corner
 *   is of class 0.
 *
 * The map is a SNAPSHOT, like the ray-cast maps: icpk_esdf_compute reads the tsdf and weight planes and writes buffers
 * of its own, behind a state of its own; it touches nothing else the context holds.  icpk_tsdf_create, _reset, _set,
 * _shift and _release drop it (its getters then answer ICPK_E_NOT_SET); icpk_esdf_release and icpk_destroy free it.
 * Integration, icpk_tsdf_apply, the extractions, the ray cast and the mesh leave it alone: after them it is STALE --
 * it describes the volume as it was -- until the next icpk_esdf_compute.
 *
 * icpk_esdf_compute     the map of the volume as it stands.  counts (or NULL: the call does not wait for the device).
 * icpk_esdf_get         sq (int32), cls (uint8), dist (float, m(q)): one entry per voxel, x fastest; any may be NULL.
 * icpk_esdf_get_box     the same of the sub-box lo <= (x, y, z) < hi, as icpk_tsdf_get_box's.
 * icpk_esdf_query       THE QUERY RULE for n <= 2^24 host points; any output may be NULL.
 * icpk_esdf_release     frees the map (ICPK_OK without one).
 * icpk_esdf_host        host only, no context: the distance rule over host planes (params: the volume's dims and
 *     voxel); sq, cls, dist, counts: any may be NULL.  Compiled from the header the kernels include (csrc/esdf_rule.h).
 * icpk_esdf_query_host  host only: THE QUERY RULE over host sq and cls planes (params: dims, voxel and the origin TO
 *     USE; esdf: max_distance gives R).
 * ICPK_E_NOT_SET: no volume; get, get_box and query before a compute.
 * Refusals (ICPK_E_ARG; a refused call leaves everything as it was): min_weight outside 1 .. 65535; max_distance not
 *     finite or not > 0; R outside 1 .. ICPK_ESDF_MAX_RADIUS; an unknown flag; an empty or out-of-bounds box; NULL
 *     coordinate arrays with n > 0; n < 0 or n > 2^24. */
#define ICPK_ESDF_UNKNOWN_OCCUPIED 1
#define ICPK_ESDF_MAX_RADIUS 1024
#define ICPK_ESDF_FAR INT32_MAX
typedef struct icpk_esdf_params {
  int32_t min_weight; /* 1 .. 65535 (1) */
  float max_distance; /* metres, finite and > 0 (2.0) */
  int32_t flags;      /* ICPK_ESDF_UNKNOWN_OCCUPIED (0) */
} icpk_esdf_params;
void icpk_default_esdf_params(icpk_esdf_params *p);
int icpk_esdf_compute(icpk_ctx *ctx, const icpk_esdf_params *params, int64_t counts[4]);
int icpk_esdf_get(icpk_ctx *ctx, int32_t *sq, uint8_t *cls, float *dist);
int icpk_esdf_get_box(icpk_ctx *ctx, const int32_t lo[3], const int32_t hi[3], int32_t *sq, uint8_t *cls, float *dist);
int icpk_esdf_query(icpk_ctx *ctx, const float *x, const float *y, const float *z, int32_t n, float *dist, float *gx,
                    float *gy, float *gz, uint8_t *status);
int icpk_esdf_release(icpk_ctx *ctx);
int icpk_esdf_host(const icpk_tsdf_params *params, const icpk_esdf_params *esdf, const float *tsdf,
                   const uint16_t *weight, int32_t *sq, uint8_t *cls, float *dist, int64_t counts[4]);
int icpk_esdf_query_host(const icpk_tsdf_params *params, const icpk_esdf_params *esdf, const int32_t *sq,
                         const uint8_t *cls, const float *x, const float *y, const float *z, int32_t n, float *dist,
                         float *gx, float *gy, float *gz, uint8_t *status);

/* ---- K32: oriented BRIEF descriptors of key points, Hamming matches ------------------------------------------------
 * A key point of icpk_detect_fast has a position and a response.  These calls give it a 256-bit appearance descriptor,
 * pair the descriptors of two frames by Hamming distance, and hand the pairs, as cloud indices, to icpk_register_global:
 * a pose between two frames without a prior.  A context holds two descriptor SLOTS, 0 the source side, 1 the target side.
 *
 * THE BRIEF RULE.  Integers only (committed tables: csrc/brief_table.h, handed out by icpk_brief_pattern and
 * icpk_brief_boundaries; stated once in csrc/brief_rule.h for the kernel and the host-only functions).
 *   Grey       three channels: K8's (1868 b + 9617 g + 4899 r + 8192) >> 14; one channel: the byte itself.
 *   Described  a key point (x, y) -- K8's are whole numbers; any other coordinate is rounded to nearest, ties to even,
 *              NaN and infinities describing nothing -- is described iff B <= x < cols - B and B <= y < rows - B, B = 15.
 *              Otherwise valid = 0, bin 0, words 0.  Entries are never dropped: descriptor k belongs to key point k.
 *   Bin        m10 = sum x I, m01 = sum y I over the disc x^2 + y^2 <= 225 around the key point (int32).  The bin k in
 *              0 .. 31 is the multiple of 11.25 degrees nearest to the direction (m10, m01) (x right, y down): bin k is
 *              the arc (b_{k-1}, b_k] between the boundaries b_j = (j + 1/2) 11.25 degrees, which ARE the eight committed
 *              integer directions and their quarter turns.  A direction exactly on b_j is in bin j, the lower one.  The
 *              direction is turned by quarter turns into x > 0, y >= 0; there the bin is the number of boundaries (bx, by)
 *              with (int64)bx * y - (int64)by * x > 0, plus 8 per quarter turn, mod 32.  m10 = m01 = 0: bin 0.
 *              ICPK_BRIEF_UPRIGHT: bin 0 everywhere.
 *   Pattern    256 tests, each a pair of offsets (a, b), a != b, every offset with x^2 + y^2 <= 169; table[k][t] =
 *              (ax, ay, bx, by) of test t in bin k, int8, 32 x 256 x 4 bytes.  Bin 0 was drawn with icpk_set_subsample's
 *              finaliser from a fixed seed, bin k is bin 0 turned by k 11.25 degrees and rounded into the disc
 *              (tools/make_brief_table.py).  The table is the rule, not the tool.
 *   Bits       S(q) = the sum of grey over the 5 x 5 box centred on q.  Bit t = S(p + a) < S(p + b) with the offsets of
 *              the key point's bin, stored as bit t & 31 of word t >> 5.  A descriptor is ICPK_BRIEF_WORDS uint32.
 *
 * THE MATCH RULE.  For every valid source descriptor i: j = the valid target descriptor minimising (H, j)
 * lexicographically, H the Hamming distance; H2 = the least distance to any OTHER valid target (257 if none).  The pair
 * is kept iff  1. H <= max_hamming;  2. if ratio_num > 0: H * ratio_den < H2 * ratio_num (integers);  3. with
 * ICPK_BRIEF_MUTUAL: i is, among the valid source descriptors, the one minimising (H, i) for target j.  Kept pairs come
 * out in source order; the list is the same bytes on every run.
 *
 * icpk_describe_keypoints   the detected list of the last icpk_detect_fast against its image, both where they lie on the
 *     device, into slot `which`.  Stream-ordered, no host wait.  ICPK_E_NOT_SET before a detection, or once
 *     icpk_bgr_to_gray has overwritten the image.
 * icpk_describe_points      the same for a caller's image (rows x cols x channels, channels 1 or 3) and n key points of
 *     any detector (x, y floats); n = 0 is legal.
 * icpk_get_descriptors / icpk_set_descriptors   a slot to the host (any array may be NULL; *n its size) and a stored one
 *     back (kp_xy or bin NULL: zeros): what a keyframe store needs.  Filling a slot, by either route, drops its cloud map
 *     and the descriptor matches.
 * icpk_described_to_cloud   icpk_detected_to_cloud's rule applied to the slot's key points: cloud `which` becomes, bit
 *     for bit, what icpk_detected_to_cloud would make of that list.  The map key point -> cloud index (-1 where the key
 *     point was dropped) stays on the device (icpk_get_descriptor_cloud_map reads it).  Whatever replaces cloud `which`
 *     afterwards drops the map, as it drops K16's descriptors.
 * icpk_match_descriptors    THE MATCH RULE over the two slots (params NULL: the defaults); *n_out (or NULL: no host
 *     wait) = the number of kept pairs.  With ICPK_BRIEF_TO_CLOUDS the kept pairs whose two key points both have cloud
 *     points are also written, as cloud indices with D = (float)H, into K16's match list, so that icpk_register_global
 *     and icpk_get_feature_matches run unchanged; without both maps ICPK_E_NOT_SET.
 * icpk_get_descriptor_matches   (src_kp, tgt_kp, H, H2) of the kept pairs, arrays of slot 0's size; any may be NULL.
 * icpk_brief_describe_host, icpk_brief_match_host   host only, no context: the two rules over host arrays (words, bin,
 *     valid of n entries; the match's outputs of ns entries, any may be NULL but n_out).  icpk_brief_bin: the bin of a
 *     pair of moments.
 * ICPK_E_ARG: another `which`, an unknown flag, a NULL image or key-point array with n > 0, rows or cols < 1, more than
 *     2^27 pixels, channels other than 1 or 3, n outside 0 .. ICPK_BRIEF_MAX_KEYPOINTS, max_hamming outside 0 .. 256,
 *     ratio_num outside 0 .. 65536, ratio_den outside 1 .. 65536, a stored valid byte above 1 or bin above 31.  Outputs
 *     are always initialised (counts to 0).  ICPK_E_NOT_SET: an empty slot. */
#define ICPK_BRIEF_WORDS 8
#define ICPK_BRIEF_MAX_KEYPOINTS 65536
#define ICPK_BRIEF_UPRIGHT 1   /* flags of the describe calls */
#define ICPK_BRIEF_MUTUAL 1    /* flags of icpk_brief_match_params */
#define ICPK_BRIEF_TO_CLOUDS 2
typedef struct icpk_brief_match_params {
  int32_t max_hamming; /* 0 .. 256 (48) */
  int32_t ratio_num;   /* 0: no ratio test (0) */
  int32_t ratio_den;   /* >= 1 (1) */
  int32_t flags;       /* ICPK_BRIEF_MUTUAL | ICPK_BRIEF_TO_CLOUDS (ICPK_BRIEF_MUTUAL) */
} icpk_brief_match_params;
void icpk_default_brief_match_params(icpk_brief_match_params *p);
int icpk_describe_keypoints(icpk_ctx *ctx, int32_t which, int32_t flags);
int icpk_describe_points(icpk_ctx *ctx, int32_t which, const uint8_t *image, int32_t rows, int32_t cols, int32_t channels,
                         const float *kp_xy, int32_t n, int32_t flags);
int icpk_get_descriptors(icpk_ctx *ctx, int32_t which, float *kp_xy, uint32_t *words, uint8_t *bin, uint8_t *valid,
                         int32_t *n);
int icpk_set_descriptors(icpk_ctx *ctx, int32_t which, const float *kp_xy, const uint32_t *words, const uint8_t *bin,
                         const uint8_t *valid, int32_t n);
int icpk_described_to_cloud(icpk_ctx *ctx, int32_t which, const uint16_t *depth, int32_t d_rows, int32_t d_cols, float fx,
                            float cx, const float R[9], const float t[3], int32_t *n_out);
int icpk_get_descriptor_cloud_map(icpk_ctx *ctx, int32_t which, int32_t *map, int32_t *n);
int icpk_match_descriptors(icpk_ctx *ctx, const icpk_brief_match_params *params, int32_t *n_out);
int icpk_get_descriptor_matches(icpk_ctx *ctx, int32_t *src_kp, int32_t *tgt_kp, int32_t *H, int32_t *H2, int32_t *n);
void icpk_brief_pattern(int8_t *out);      /* 32 x 256 x 4 bytes */
void icpk_brief_boundaries(int32_t *out);  /* 8 x (x, y) */
int icpk_brief_bin(int32_t m10, int32_t m01);
int icpk_brief_describe_host(const uint8_t *image, int32_t rows, int32_t cols, int32_t channels, const float *kp_xy,
                             int32_t n, int32_t flags, uint32_t *words, uint8_t *bin, uint8_t *valid);
int icpk_brief_match_host(const uint32_t *words_s, const uint8_t *valid_s, int32_t ns, const uint32_t *words_t,
                          const uint8_t *valid_t, int32_t nt, const icpk_brief_match_params *params, int32_t *src_kp,
                          int32_t *tgt_kp, int32_t *H, int32_t *H2, int32_t *n_out);

/* ---- DBSCAN clustering of one of the context's clouds (K33; extension: what pcl::EuclideanClusterExtraction and
 * Open3D's cluster_dbscan offer) ----
 * Says which points belong together: labels every point of the working source or the target with its cluster, and --
 * unless ICPK_CLUSTER_LABELS_ONLY -- keeps the points of the selected clusters.  A clump of stray points has neighbours,
 * so K13's filters keep it; a cluster too small to be a surface is what this call removes.
 *
 * THE CLUSTER RULE.  Input: the n points of the cloud in index order; eps > 0 (float) and min_points >= 1.
 *   distance   d(i, j) is the pair distance of icp.cpp:606-620 exactly as every NN search here evaluates it (K13's).  It
 *              is symmetric: the float differences only change sign.  `<=` is a float compare.  A point with a non-finite
 *              coordinate is nobody's neighbour and has none.
 *   count      m_i = #{ finite j : d(i, j) <= eps }, i itself and duplicates included: K12's and K13's count.  A
 *              non-finite point has m_i = 0 (and only such a point has).
 *   core       point i is a core point iff m_i >= min_points -- the point counts itself, as in Open3D and scikit-learn.
 *              min_points = 1 makes every finite point a core point: PCL's Euclidean clustering.
 *   clusters   a cluster is a connected component of the core points under d <= eps.  Its representative is the smallest
 *              index among its core points; clusters are numbered 0, 1, ... by ascending representative.
 *   border     a finite point that is not a core point but has at least one core neighbour joins the cluster of the core
 *              neighbour j that minimises (d(i, j), j) lexicographically -- the key (float bits << 32) | j.  A border
 *              point never joins two clusters together.  Libraries that give a border point to whichever cluster reaches
 *              it first depend on the order of their traversal; this rule does not, so BORDER labels may differ from
 *              Open3D's or scikit-learn's.  The partition of the core points cannot.
 *   noise      every other point, the non-finite ones included: label -1.  n_noise counts them all; the non-finite ones
 *              are exactly the points with count 0.
 *   selection  a point is kept iff its label is >= 0 and min_size <= size[label] <= max_size (max_size = 0: no upper
 *              bound; a cluster's size counts its core and border members) and, with largest_only, its cluster is the one
 *              of greatest size among all clusters, ties to the lower label.  Kept points keep their order and their
 *              floats and, on the target, their normals, exactly as K13's compaction does.
 * Everything in the record is a function of the cloud alone: the same bytes on every run, and the bytes of the numpy model
 * (tests/cluster_model.py) and of icpk_cluster_host.  The labels of the core points of a permuted cloud are the permuted
 * partition.
 *
 * icpk_cluster_dbscan   which: 0 = the working source (indexed in buffers of the call's own: the target's index is not
 *     disturbed), 1 = the target (its own index, built if it has none and then valid for the alignment that follows).
 *     Without ICPK_CLUSTER_LABELS_ONLY the kept points become the context's cloud exactly as after icpk_remove_outliers:
 *     everything derived from the old cloud is dropped, the target's normals are carried.  With it nothing of the cloud,
 *     its normals or its index changes; the record (out_index and n_out included, which then say what a replacing call
 *     would keep) is replaced either way.  n_clusters / n_noise / n_out: any may be NULL.  One host wait, for the counts.
 *     An empty cloud is ICPK_OK with no cluster.
 *     ICPK_E_ARG: another `which`, an unknown flag, NULL params, a non-finite or non-positive eps, min_points < 1, a
 *     negative min_size or max_size, max_size below min_size when not 0, largest_only other than 0 or 1 (nothing
 *     changes); ICPK_E_NOT_SET if that cloud has not been set.
 * icpk_get_clusters   the record of the last call (it stays on the device until asked for; this call waits).  Per point
 *     (n_in entries): labels; core (1 / 0); count (m_i); nearest_core (i for a core point, the chosen j for a border
 *     point, -1 for noise); out_index (the position in the selected cloud, -1 where the point was not kept).  Per cluster
 *     (n_clusters entries): sizes; first (the representative).  Any pointer may be NULL: a first call with all arrays NULL
 *     returns the two sizes.  ICPK_E_NOT_SET before the first icpk_cluster_dbscan.
 * icpk_cluster_host   host only, no context: the rule as a literal O(n^2) program over points[3][n] (x, y and z planes),
 *     with the same outputs (labels_only has no meaning here: nothing is replaced).  The per-point arrays take n entries,
 *     sizes and first n_clusters (<= n; a call with both NULL returns it).  Any output may be NULL.  ICPK_E_ARG as above,
 *     and for n < 0 or NULL points with n > 0. */
#define ICPK_CLUSTER_LABELS_ONLY 1 /* flags: compute and keep the record, leave the cloud as it is */
typedef struct icpk_cluster_params {
  float eps;            /* finite, > 0                                            */
  int32_t min_points;   /* >= 1: neighbours (itself included) that make a core    */
  int32_t min_size;     /* selection: >= 0                                        */
  int32_t max_size;     /* selection: 0 = no upper bound, else >= min_size        */
  int32_t largest_only; /* selection: 1 = only the cluster of greatest size       */
} icpk_cluster_params;
int icpk_cluster_dbscan(icpk_ctx *ctx, int32_t which, const icpk_cluster_params *params, int32_t flags,
                        int32_t *n_clusters, int32_t *n_noise, int32_t *n_out);
int icpk_get_clusters(icpk_ctx *ctx, int32_t *n_in, int32_t *n_clusters, int32_t *labels, uint8_t *core, int32_t *count,
                      int32_t *nearest_core, int32_t *out_index, int32_t *sizes, int32_t *first);
int icpk_cluster_host(const float *points, int32_t n, const icpk_cluster_params *params, int32_t *n_clusters,
                      int32_t *n_noise, int32_t *n_out, int32_t *labels, uint8_t *core, int32_t *count,
                      int32_t *nearest_core, int32_t *out_index, int32_t *sizes, int32_t *first);

/* ---- RANSAC plane segmentation of one of the context's clouds (K34; extension: what Open3D's segment_plane and PCL's
 * SACSegmentation<SACMODEL_PLANE> offer, repeated until no plane is left) ----
 * Says which points are the floor, the wall, the table top: labels every point of the working source or the target with
 * the plane it lies on and -- unless ICPK_PLANE_LABELS_ONLY -- keeps either what is left when the planes are taken out
 * (the default: "remove the planes, cluster the rest", icpk_cluster_dbscan) or the points of the planes.
 *
 * THE PLANE RULE.  Input: the n points of the cloud in index order, as floats; distance_threshold t (float, finite,
 * > 0); n_hypotheses H (1 .. ICPK_PLANE_MAX_HYPOTHESES); seed (uint64); max_planes P (1 .. ICPK_PLANE_MAX_PLANES);
 * min_inliers >= 3.  Everything below is float64 unless it says otherwise; every product, sum and difference is one
 * rounded operation in the written association, none is fused, and of libm only sqrt is used.
 *   labels     every point starts with label -1.  A point with a non-finite coordinate is never sampled and never an
 *              inlier: it keeps -1 and counts as dropped (it is in neither n_unassigned nor any plane).
 *   rounds     r = 0, 1, ... while r < P.  E is the list of the finite points with label -1 in ascending index, m = |E|.
 *              The round ends the call if m < 3 or m < min_inliers.
 *   draws      hypothesis h = 0 .. H-1 has g = r * H + h (uint64) and draws d = 0 .. 15:
 *              z = seed + (g + 1) * 0x9E3779B97F4A7C15 + d * 0xD1B54A32D192ED03 mod 2^64, then icpk_set_subsample's
 *              finaliser (z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31)
 *              and c = (uint32)(z >> 32) % m -- K16's draw.  The first three distinct c in draw order give the samples
 *              a = E[c0], b = E[c1], c = E[c2]; fewer than three distinct values make the hypothesis invalid.
 *   plane      u = b - a, v = c - a (differences of the widened floats); N0 = u1 v2 - u2 v1, N1 = u2 v0 - u0 v2,
 *              N2 = u0 v1 - u1 v0; L2 = (N0 N0 + N1 N1) + N2 N2; G = ((double)t * (double)t) * L2.  The hypothesis is valid
 *              iff L2 > 0 and G is finite.
 *   count      for every point p of E: e_k = (double)p_k - (double)a_k, s = (N0 e0 + N1 e1) + N2 e2; p is an inlier iff
 *              s * s <= G.  c_h is the number of inliers.  The winner is the valid h of greatest c_h, ties to the lowest
 *              h.  No valid hypothesis, or a winning count below 3, ends the call.
 *   refit      over the winner's inliers the nine terms e0, e1, e2, e0 e0, e0 e1, e0 e2, e1 e1, e1 e2, e2 e2 (e relative
 *              to the winner's a) are summed through the canonical tree (ICPK_RED_THREADS / ICPK_RED_MAX_BLOCKS, the tree
 *              of icpk_reduce) over all n points in index order; a point that is not an inlier adds nothing.  With
 *              k = (double)count: mu_a = S_a / k and C_ab = S_ab - (S_a * S_b) / k.  The symmetric 3 x 3 C goes through a
 *              cyclic Jacobi eigen-solve: sweeps over (p, q) = (0,1), (0,2), (1,2), at most 32 of them, ended when every
 *              off-diagonal entry is exactly 0; a rotation skips an entry that is exactly 0 and otherwise takes
 *              theta = (C_qq - C_pp) / (2 C_pq), root = sqrt(theta theta + 1), tan = theta < 0 ? -1 / (root - theta)
 *              : 1 / (root + theta), cos = 1 / sqrt(tan tan + 1), sin = tan cos; C_pp -= tan C_pq, C_qq += tan C_pq,
 *              C_pq = 0, C_rp = cos C_rp - sin C_rq and C_rq = sin C_rp + cos C_rq (old values on the right), and the same
 *              two-column update on the rows of V, which starts as the identity.  Eigenvalues l0 <= l1 <= l2: the least
 *              diagonal entry (the lowest axis on a tie) is l0, and the column of V at its axis, divided by its length
 *              sqrt((v0 v0 + v1 v1) + v2 v2), is the normal.  Sign: the component of largest magnitude is made positive,
 *              the lowest axis on a tie.  centre = (double)a + mu.  If any of these is not finite, or
 *              l1 <= 2^-20 * l2 (the inliers lie on a line), the plane falls back to the hypothesis: normal N / sqrt(L2)
 *              with the same sign convention, centre a, curvature 0.
 *   final      a point of E is a final inlier iff |(n0 (p0 - c0) + n1 (p1 - c1)) + n2 (p2 - c2)| <= (double)t (p widened,
 *              c the centre).  If there are fewer than min_inliers of them the round writes nothing and ends the call;
 *              otherwise they get label r and the next round starts.
 *   record     per plane eight doubles -- normal (3), d = -((n0 c0 + n1 c1) + n2 c2), centre (3), the curvature
 *              l0 / ((l0 + l1) + l2) -- six integers -- the winning h, the three samples' indices in the cloud, the RANSAC
 *              count, the final count -- and the nine sums.
 *   selection  default: the finite points with label -1.  ICPK_PLANE_KEEP_INLIERS: the points with label >= 0, or with
 *              select_plane = k >= 0 those with label k.  Kept points keep their order, their floats and, on the target,
 *              their normals, exactly as K13's compaction does.
 * The draws, every count, the winner, the sums' bits and -- given a plane's eight doubles -- the final mask are exact for
 * a given order of the cloud; the fit carries the rounding of the Jacobi, which is the same function on the host and on
 * the device (csrc/plane_rule.h).  So the record is a function of the cloud and the seed alone: the same bytes on every
 * run, and the bytes of the numpy model (tests/plane_model.py) and of icpk_segment_planes_host.
 *
 * icpk_default_plane_params   seed 0, t 0.01, 256 hypotheses, 4 planes, min_inliers 1000, select_plane -1.
 * icpk_segment_planes   which: 0 = the working source, 1 = the target; no index is built or read.  Without
 *     ICPK_PLANE_LABELS_ONLY the selected points become the context's cloud exactly as after icpk_remove_outliers:
 *     everything derived from the old cloud is dropped, the target's normals are carried.  With it nothing of the cloud,
 *     its normals or its index changes; the record (out_index and n_out included, which then say what a replacing call
 *     would keep) is replaced either way.  n_planes; n_unassigned: the finite points left with label -1; n_out: the
 *     selected points.  Any may be NULL.  One host wait per round that runs (at most max_planes), for the round's count
 *     block; a round the rule would end at once is not started.  An empty cloud, and a cloud with no plane, are ICPK_OK
 *     with n_planes = 0.
 *     ICPK_E_ARG (nothing changes): another `which`, an unknown flag, NULL params, t not finite or <= 0, n_hypotheses,
 *     max_planes, min_inliers or select_plane (-1 .. ICPK_PLANE_MAX_PLANES - 1) out of range, select_plane >= 0 without
 *     ICPK_PLANE_KEEP_INLIERS; ICPK_E_NOT_SET if that cloud has not been set.
 * icpk_get_planes   the record of the last call (it stays on the device until asked for; this call waits).  Per point
 *     (n_in entries): labels, out_index (the position in the selected cloud, -1 where the point was not selected).  Per
 *     plane (n_planes entries): model (8 doubles), info (6 integers), sums (9 doubles).  Any pointer may be NULL: a first
 *     call with all arrays NULL returns the two sizes.  ICPK_E_NOT_SET before the first icpk_segment_planes.
 * icpk_segment_planes_host   host only, no context: the rule as a literal O(P H n) program over points[3][n] (x, y and
 *     z planes) with the same outputs; of the flags only ICPK_PLANE_KEEP_INLIERS means anything here.  Any output may be
 *     NULL.  ICPK_E_ARG as above, and for n < 0 or NULL points with n > 0.
 * icpk_plane_fit_host   host only: the refit alone -- the nine sums, their count (>= 1), the sample a and the
 *     hypothesis' normal N (not normalised) to the plane's eight doubles. */
#define ICPK_PLANE_MAX_HYPOTHESES 65536
#define ICPK_PLANE_MAX_PLANES 16
#define ICPK_PLANE_LABELS_ONLY 1  /* flags: compute and keep the record, leave the cloud as it is */
#define ICPK_PLANE_KEEP_INLIERS 2 /* flags: the selection keeps the plane points; default keeps the rest (planes removed) */
typedef struct icpk_plane_params {
  uint64_t seed;
  float distance_threshold; /* t: finite, > 0                                        */
  int32_t n_hypotheses;     /* H: 1 .. ICPK_PLANE_MAX_HYPOTHESES, per round          */
  int32_t max_planes;       /* P: 1 .. ICPK_PLANE_MAX_PLANES                         */
  int32_t min_inliers;      /* >= 3: final inliers a plane needs                     */
  int32_t select_plane;     /* -1: all planes; k: plane k only (with KEEP_INLIERS)   */
  int32_t reserved;         /* 0                                                     */
} icpk_plane_params;
void icpk_default_plane_params(icpk_plane_params *params);
int icpk_segment_planes(icpk_ctx *ctx, int32_t which, const icpk_plane_params *params, int32_t flags, int32_t *n_planes,
                        int32_t *n_unassigned, int32_t *n_out);
int icpk_get_planes(icpk_ctx *ctx, int32_t *n_in, int32_t *n_planes, int32_t *labels, int32_t *out_index, double *model,
                    int32_t *info, double *sums);
int icpk_segment_planes_host(const float *points, int32_t n, const icpk_plane_params *params, int32_t flags,
                             int32_t *n_planes, int32_t *n_unassigned, int32_t *n_out, int32_t *labels, int32_t *out_index,
                             double *model, int32_t *info, double *sums);
int icpk_plane_fit_host(const double sums[9], int32_t count, const float a[3], const double hyp_normal[3], double model[8]);

/* ---- test hook ------------------------------------------------------------ */
/* icp.cpp:606-620 distance(color_point_t, color_point_t) evaluated on the
 * device for n pairs; a and b are host xyz-SoA arrays [3][n].  Lets the parity
 * tests check the float/double/sqrt sequence bit for bit on its own. */
int icpk_pair_distance(icpk_ctx *ctx, const float *a, const float *b, float *out, int32_t n);
/* same for icp.cpp:595-602 distance(cv::Point3f, cv::Point3f): double sqrt, narrowed on
 * return (dead in the reference: its only call site is pointcloud.cpp:246) */
int icpk_pair_distance3(icpk_ctx *ctx, const float *a, const float *b, float *out, int32_t n);

/* ---- small host helpers restated from the reference (no device work) ----- */
float icpk_distance3(const float a[3], const float b[3]);                            /* icp.cpp:595-602      */
void icpk_make_rotation_matrix(float x_deg, float y_deg, float z_deg, float out[9]); /* icp.cpp:640-653      */
void icpk_matrix_to_quaternion(const float m[9], float q_wxyz[4]);                 /* quaternion.cpp:23-79 */
void icpk_quaternion_to_euler(const float q_wxyz[4], float e_deg[3]);              /* SLAM.cpp:613-636     */
/* pointcloud.cpp:60-98: the 3-D points of a frame's key points (what findGlobalKeyPointAssociations, icp.cpp:488,
 * is fed).  kp_xy: n pixel positions (x, y) as cv::KeyPoint::pt holds them; each is rounded to a pixel as the
 * reference's Point2f -> Point2i conversion does (cvRound: to nearest, ties to even), dropped if its depth is 0
 * (:67-70) -- or if it falls outside the image, where the reference reads out of bounds -- and back-projected with
 * the formula of :86-88 (CX and FX for y too).  out_xyz: room for n points (x, y, z interleaved); kept (or NULL):
 * the index into kp_xy of every point written.  Returns the number of points (>= 0) or a negative status.  Host only. */
int icpk_backproject_keypoints(const uint16_t *depth, int32_t rows, int32_t cols, const float *kp_xy, int32_t n,
                               float fx, float cx, float *out_xyz, int32_t *kept);
/* host solve exposed for testing: reference flavour from the float moment,
 * Kabsch flavour from raw sums (n, sum a, sum b, sum a b^T) */
void icpk_solve_reference(const float M[9], float R[9]);                           /* icp.cpp:215-223      */
void icpk_solve_kabsch(int64_t n, const double sa[3], const double sb[3],
                       const double sab[9], double R[9], double t[3]);             /* rigid_transform_3D.py:9-40 */

#ifdef __cplusplus
}
#endif
#endif /* ICPK_H */
