// icpk_sweep.cpp -- host side of the nearest-neighbour sweeps (K1 in every ICPK_NN_* mode) and of the reductions
// (K2, K5, K14): device buffers, target and query preparation, the frame-batch set-up recorder, and the C ABI's icpk_nn,
// icpk_reduce, icpk_reduce_p2l and icpk_get_associations.
#include <cstring>
#include <utility>

#include "icpk_ctx.h"

using namespace icpk;

namespace icpk {

int ensure_cloud(icpk_ctx* ctx, Cloud& c, int n) {
  if (ctx && (&c == &ctx->src0 || &c == &ctx->src)) ctx->src_pristine = false;  // (about to be resized or rewritten)
  if (ctx && &c == &ctx->src) ctx->rec_pending = false;  // (whatever was to be unpacked into it is superseded)
  // (as is a copy of the committed source still owed to it; and one owed FROM a source that is being replaced is dropped:
  // every such call goes on to write the working source too, or to copy_src0_to_src)
  if (ctx && (&c == &ctx->src0 || &c == &ctx->src)) ctx->src_deferred = false;
  if (ctx && &c == &ctx->src0) ctx->have_src_normals = false;  // (they describe the uploaded source that is being replaced)
  if (ctx && &c == &ctx->src0) fpfh_dropped(ctx, 0);           // (as K16's descriptors and matches do)
  if (ctx && &c == &ctx->src0) ctx->have_src_colors = false;   // (as K17's intensities do)
  if (ctx && (&c == &ctx->src0 || &c == &ctx->tgt)) ctx->have_pix_seed = false;  // (other points than the pixel maps describe)
  if (ctx && (&c == &ctx->src0 || &c == &ctx->tgt)) ctx->have_score_assoc = false;  // (K15's kept associations speak of the clouds they were scored on)
  const int cap = round_up(n < 1 ? 1 : n, NN_TILE);
  if (cap > c.cap) {
    c.cap = 0;
    // +64 floats: the filtered NN kernel prefetches one group past its chunk
    if (int rc = c.base.reserve(ctx, (size_t)3 * cap + 64)) return rc;
    c.cap = cap;
  }
  c.n = n;
  return ICPK_OK;
}

int ensure_assoc(icpk_ctx* ctx, int nq) {
  const size_t cap = round_up(nq < 1 ? 1 : nq, NN_TILE);
  bool grown = false;
  const int rc = reserve_group(ctx, &grown, need(ctx->best, cap), need(ctx->seed, cap), need(ctx->best_m, cap),
                               need(ctx->seed_m, cap), need(ctx->idx, cap), need(ctx->dist, cap));
  if (grown) ctx->have_seed = false;
  return rc;
}

static int ensure_sort_buffers(icpk_ctx* ctx, int n) {
  const size_t cap = round_up(n < 1 ? 1 : n, NN_TILE);
  int rc = reserve_group(ctx, nullptr, need(ctx->sort_keys, 2 * cap), need(ctx->sort_vals, cap));
  ctx->sort_cap = (int)ctx->sort_vals.capacity();
  return rc ? rc : ctx->bounds.reserve(ctx, 6);
}

static int ensure_scan_buffers(icpk_ctx* ctx);

// Morton order of `c` (cells of the target's bounding box) -> perm_out[k] = index of the k-th point; the sorted keys
// land in sort_keys[sort_cap ...), the unsorted ones stay in sort_keys[0 ... n)
static int enqueue_morton_order(icpk_ctx* ctx, const Cloud& c, int* perm_out) {
  int rc = ensure_sort_buffers(ctx, c.n);
  if (rc) return rc;
  rc = ensure_scan_buffers(ctx);
  if (!rc) rc = ctx->morton_table.reserve(ctx, 1);
  if (rc) return rc;
  unsigned* ka = ctx->sort_keys;
  unsigned* kb = ctx->sort_keys + ctx->sort_cap;
  const int bits = ctx->grid_max_cells >= (1 << 21) + 1 ? 7 : 6;  // 8^bits cells + 1 bin + 1 must fit the count table
  ctx->qcount_dirty = true;
  launch_morton_order(c.x(), c.y(), c.z(), c.n, ctx->bounds, bits, ka, ctx->sort_vals, ctx->qcount, ctx->qstart, ctx->scan_bsum,
                      ctx->morton_table, kb, perm_out, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ctx->qcount_dirty = false;
  return ICPK_OK;
}

// boxes + Morton-ordered target for the pruned scan (once per target cloud)
static int prepare_pruned_target(icpk_ctx* ctx, NnBoxes& bx) {
  const int nt = ctx->tgt.n;
  const int nt_pad = round_up(nt, NN_TILE);
  const int ntiles = nt_pad / NN_TILE;
  bool grown = false;
  int rc = ICPK_OK;
  if (ntiles > ctx->boxes_tiles_cap) {
    ctx->boxes_tiles_cap = 0;
    rc = ctx->boxes.reserve(ctx, (size_t)6 * (ntiles + 16) * (1 + NN_SUBS), &grown);
    if (!rc) ctx->boxes_tiles_cap = ntiles;
  }
  if (!rc) rc = ctx->tperm.reserve(ctx, (size_t)nt_pad + 64, &grown);  // (+64: read ahead)
  if (!rc) rc = ctx->tkeys.reserve(ctx, (size_t)nt_pad + 64, &grown);
  if (grown) ctx->have_boxes = false;
  if (rc) return rc;
  bx.tbox_stride = ctx->boxes_tiles_cap + 16;
  bx.sbox_stride = (ctx->boxes_tiles_cap + 16) * NN_SUBS;
  bx.tbox = ctx->boxes;
  bx.sbox = ctx->boxes + (size_t)6 * bx.tbox_stride;
  bx.ox = ctx->tgt.x();
  bx.oy = ctx->tgt.y();
  bx.oz = ctx->tgt.z();
  bx.tperm = ctx->tperm;
  bx.qperm = ctx->qperm;
  if (ctx->have_boxes) return ICPK_OK;
  rc = ensure_cloud(ctx, ctx->sorted, nt);
  if (rc) return rc;
  rc = ensure_sort_buffers(ctx, nt);
  if (rc) return rc;
  // bounds of the cloud from boxes of the caller's order, then sort, gather, final boxes
  launch_tile_boxes(ctx->tgt.x(), ctx->tgt.y(), ctx->tgt.z(), nt, ntiles, bx, ctx->stream);
  launch_bounds(bx.tbox, bx.tbox_stride, ntiles, ctx->bounds, ctx->stream);
  rc = enqueue_morton_order(ctx, ctx->tgt, ctx->tperm);
  if (rc) return rc;
  ICPK_HIP(ctx, hipMemcpyAsync(ctx->tkeys, ctx->sort_keys + ctx->sort_cap, (size_t)nt * sizeof(unsigned),
                               hipMemcpyDeviceToDevice, ctx->stream));
  launch_gather_planes(ctx->tgt.x(), ctx->tgt.y(), ctx->tgt.z(), ctx->tperm, nt, nt_pad, __builtin_inff(),
                       ctx->sorted.x(), ctx->sorted.y(), ctx->sorted.z(), ctx->tperm, ctx->stream);
  launch_tile_boxes(ctx->sorted.x(), ctx->sorted.y(), ctx->sorted.z(), nt, ntiles, bx, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ctx->have_boxes = true;
  return ICPK_OK;
}

// counts / starts of the counting sorts by cell (targets: cell_start; queries: qstart).  The count table is
// all zero between two sorts (the scan hands it back zeroed); a sort that did not get as far as its scan --
// a failed launch -- leaves it marked dirty, and the next one clears all of it first.
static int ensure_scan_buffers(icpk_ctx* ctx) {
  const size_t cells = (size_t)ctx->grid_max_cells + 1;
  bool fresh = false;
  int rc = ctx->qcount.reserve(ctx, cells, &fresh);
  if (fresh) ctx->qcount_dirty = true;
  if (rc) return rc;
  if (ctx->qcount_dirty) {
    ICPK_HIP(ctx, hipMemsetAsync(ctx->qcount, 0, cells * sizeof(int), ctx->stream));
    ctx->qcount_dirty = false;
  }
  rc = ctx->qstart.reserve(ctx, cells);
  return rc ? rc : ctx->scan_bsum.reserve(ctx, GRID_SCAN_BLOCKS);
}

int GridIndex::reserve(icpk_ctx* ctx, int n, bool* grown) {
  int rc = info.reserve(ctx, 1);
  if (!rc) rc = bounds.reserve(ctx, (size_t)GRID_BOUNDS_PARTS * 6);
  if (!rc) rc = cell_start.reserve(ctx, (size_t)ctx->grid_max_cells + 1);
  if (rc) return rc;
  const size_t n4 = (size_t)round_up(n, NN_TILE) + 64;
  return reserve_group(ctx, grown, need(t4, n4), need(o4, n4));
}

// room for the target's index (a reallocation drops the grid)
static int reserve_target_index(icpk_ctx* ctx) {
  if (ctx->tgt.n > (1 << 28)) return fail(ctx, ICPK_E_ARG, "the grid search addresses its cell-sorted targets with 32-bit byte offsets: at most 2^28 target points");
  bool grown = false;
  const int rc = ctx->grid.reserve(ctx, ctx->tgt.n, &grown);
  if (grown) ctx->have_grid = false;
  return rc;
}

// Everything is enqueued: the grid's size stays on the device (GridInfo), the counting sort's
// zero fill and scan read it there -- no host round trip, so the frame-batch mode can build the
// next group's grids in the shadow of the running loop.
int index_cloud(icpk_ctx* ctx, const float* x, const float* y, const float* z, int n, GridIndex& g) {
  int rc = ensure_sort_buffers(ctx, n);
  if (!rc) rc = ensure_scan_buffers(ctx);
  if (rc) return rc;
  launch_grid_bounds(bounds_args(x, y, z, n, g.bounds), ctx->stream);
  launch_grid_info(info_args(g.bounds, n, ctx->tune.grid_ppc, ctx->tune.grid_xdiv, ctx->grid_max_cells, g.info), ctx->stream);
  // counting sort of the points by cell: slot within the cell by atomics (the order inside a
  // cell is irrelevant: candidates are merged lexicographically), cell starts by an exclusive
  // scan of the counts (entry ncells = n), scatter into the AoS copy
  int* cell = reinterpret_cast<int*>(ctx->sort_keys + ctx->sort_cap);
  int* slot = ctx->sort_vals;
  ctx->qcount_dirty = true;
  launch_grid_qslot(QslotArgs{x, y, z, g.info, ctx->qcount, cell, slot, n, 0}, ctx->stream);
  launch_grid_scan(ScanArgs{ctx->qcount, g.cell_start, ctx->scan_bsum, g.info, 0, 0}, ctx->stream);
  launch_grid_tscatter(TscatterArgs{x, y, z, cell, slot, g.cell_start, g.t4, g.o4, n, 0}, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ctx->qcount_dirty = false;
  return ICPK_OK;
}

// (once per target cloud)
int index_target(icpk_ctx* ctx, GridView* out) {
  int rc = reserve_target_index(ctx);
  if (!rc && !ctx->have_grid) {
    rc = index_cloud(ctx, ctx->tgt.x(), ctx->tgt.y(), ctx->tgt.z(), ctx->tgt.n, ctx->grid);
    ctx->have_grid = !rc;
  }
  if (!rc && out) *out = ctx->grid.view();
  return rc;
}

int index_aux(icpk_ctx* ctx, const Cloud& c, GridView* out) {
  if (c.n > (1 << 28)) return fail(ctx, ICPK_E_ARG, "the grid search addresses its cell-sorted points with 32-bit byte offsets: at most 2^28 points");
  int rc = ctx->aux_grid.reserve(ctx, c.n);
  if (!rc) rc = index_cloud(ctx, c.x(), c.y(), c.z(), c.n, ctx->aux_grid);
  if (!rc) *out = ctx->aux_grid.view();
  return rc;
}

// the scatter of the working source into scan order (qm4 != nullptr: with the scan-order queries and their seeds; pix: the
// seeds come from the pixel maps)
static QscatterArgs query_scatter_args(icpk_ctx* ctx, const int* qcell, const int* qslot, float4* qm4, bool pix) {
  const Cloud& q = query_cloud(ctx);
  return QscatterArgs{qcell,        qslot,        ctx->qstart,  ctx->qperm, q.x(),        q.y(),        q.z(),
                      ctx->tgt.x(), ctx->tgt.y(), ctx->tgt.z(), qm4,        ctx->sp_in,   ctx->seed_m,  ctx->src.n,
                      0,            pix ? ctx->pix_src.get() : nullptr,     pix ? ctx->pix_tidx.get() : nullptr,
                      ctx->pix_rows, ctx->pix_cols};
}

// query order for the grid scan: counting sort of the source by cell of the target's grid.
// with_points: the scatter also writes the scan-order queries and element 0 as everybody's seed
// (the first sweep of an alignment that has no seeds)
static int enqueue_cell_order(icpk_ctx* ctx, bool with_points) {
  const int nq = ctx->src.n;
  int rc = ensure_sort_buffers(ctx, nq);
  if (rc) return rc;
  rc = ensure_scan_buffers(ctx);
  if (rc) return rc;
  int* qcell = reinterpret_cast<int*>(ctx->sort_keys + ctx->sort_cap);
  int* qslot = ctx->sort_vals;
  // a source in image order with pixel maps (icpk_backproject_pair, icpk_align_frames_batch's slots): as in
  // build_grid_and_order, the queries keep the caller's order (no counting sort) and get pixel seeds
  const bool ident = ctx->have_pix_seed && ctx->tune.image_order;
  const bool pix = ctx->have_pix_seed && ctx->tune.pixel_seeds && with_points;
  if (!ident) {
    // (locality only: the coarser table, xdiv times fewer counts to scan)
    ctx->qcount_dirty = true;
    const Cloud& q = query_cloud(ctx);
    const QslotArgs qa{q.x(), q.y(), q.z(), ctx->grid.info, ctx->qcount, qcell, qslot, nq, 1};
    // (a new source pose against an indexed target: this is the alignment's first launch, and it carries the pending
    // initial LoopState as grid_begin_kernel does for a fresh pair)
    if (ctx->init_pending && launch_grid_qslot_init(qa, ctx->pending_init, ctx->stream))
      ctx->init_pending = false;
    else
      launch_grid_qslot(qa, ctx->stream);
    launch_grid_scan(ScanArgs{ctx->qcount, ctx->qstart, ctx->scan_bsum, ctx->grid.info, 1, 0}, ctx->stream);
  }
  launch_grid_qscatter(query_scatter_args(ctx, ident ? nullptr : qcell, qslot, with_points ? ctx->qm4.get() : nullptr, pix),
                       ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ctx->qcount_dirty = false;
  return ICPK_OK;
}

static int ensure_query_points(icpk_ctx* ctx, int nq);

// After a device loop of grid sweeps the caller-order views -- the moved source planes, the association keys -- exist
// only as records (ctx->rec, kernels_grid.hip); they are unpacked when something asks for them (icpk_get_source,
// icpk_get_associations, icpk_commit_source, icpk_transform_source, icpk_nn, icpk_reduce ...) and dropped when the
// working source is overwritten first (the next alignment, a new source): a tracker that only wants the pose never
// pays the launch.  ICPK_LAZY_UNPACK=0: unpack at the end of every loop.
// It is also the one place that makes a deferred copy of the committed source (src_deferred): all of it when nothing has
// moved the source since, only the padding when the unpack is about to write every point.
int ensure_unpacked(icpk_ctx* ctx) {
  if (ctx->src_deferred) {
    ctx->src_deferred = false;
    if (int rc = copy_source_planes(ctx, /*tail_only=*/ctx->rec_pending)) return rc;
  }
  if (!ctx->rec_pending) return ICPK_OK;
  ctx->rec_pending = false;
  launch_grid_unpack(ctx->qm4, ctx->rec, ctx->src.n, ctx->src.x(), ctx->src.y(), ctx->src.z(), ctx->best, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  return ICPK_OK;
}

// the deferred initial LoopState of a device loop (device_loop_begin), if no set-up launch has carried it
int flush_loop_init(icpk_ctx* ctx) {
  if (!ctx->init_pending) return ICPK_OK;
  ctx->init_pending = false;
  launch_loop_init(ctx->pending_init, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  return ICPK_OK;
}

// A FRESH pair (new target, new source, no seeds: every frame of the drop-in path): the target's grid and the
// query order in 6 launches instead of 10 -- the two counting sorts run side by side (cell slots of both clouds in one
// launch, both scans in two, both scatters in one), each with its own count table.  Same kernels' bodies as
// index_target + enqueue_cell_order: same tables, same copies.  ~5 us of launch latency per launch saved on a
// path that is a chain of tiny dependent kernels.
static int build_grid_and_order(icpk_ctx* ctx) {
  const int nt = ctx->tgt.n, nq = ctx->src.n;
  int rc = reserve_target_index(ctx);
  if (rc) return rc;
  rc = ensure_sort_buffers(ctx, nq > nt ? nq : nt);
  if (rc) return rc;
  rc = ensure_scan_buffers(ctx);
  if (rc) return rc;
  const size_t cells = (size_t)ctx->grid_max_cells + 1;
  bool fresh = false;
  rc = ctx->qcount2.reserve(ctx, cells, &fresh);
  if (fresh) ctx->qcount2_dirty = true;
  if (!rc) rc = ctx->scan_bsum2.reserve(ctx, GRID_SCAN_BLOCKS);
  if (rc) return rc;
  if (ctx->qcount2_dirty) {  // (first use, or a sort that was cut short: the scans hand the table back zeroed otherwise)
    ICPK_HIP(ctx, hipMemsetAsync(ctx->qcount2, 0, cells * sizeof(int), ctx->stream));
    ctx->qcount2_dirty = false;
  }
  if ((rc = ctx->sort_vals2.reserve(ctx, ctx->sort_cap))) return rc;
  int* tcell = reinterpret_cast<int*>(ctx->sort_keys + ctx->sort_cap);
  int* tslot = ctx->sort_vals;
  int* qcell = reinterpret_cast<int*>(ctx->sort_keys.get());
  int* qslot = ctx->sort_vals2;
  fresh = false;
  if ((rc = ctx->grid_ticket.reserve(ctx, 1, &fresh))) return rc;
  if (fresh) {  // (zero from here on: the last arrival resets it; a failed memset gives the ticket up, to be made again)
    const hipError_t e = hipMemsetAsync(ctx->grid_ticket, 0, sizeof(int), ctx->stream);
    if (e != hipSuccess) {
      (void)ctx->grid_ticket.release();
      return hip_failure(ctx, "hipMemsetAsync(grid_ticket)", e);
    }
  }
  // bounds + geometry (+ the pending initial LoopState of the alignment being enqueued) in ONE launch
  GridIndex& g = ctx->grid;
  launch_grid_begin(bounds_args(ctx->tgt.x(), ctx->tgt.y(), ctx->tgt.z(), nt, g.bounds),
                    info_args(g.bounds, nt, ctx->tune.grid_ppc, ctx->tune.grid_xdiv, ctx->grid_max_cells, g.info),
                    ctx->init_pending ? &ctx->pending_init : nullptr, ctx->grid_ticket, ctx->stream);
  ctx->init_pending = false;
  ctx->qcount_dirty = ctx->qcount2_dirty = true;
  SetupBatchOf<QslotArgs> qb{};
  qb.p[0] = QslotArgs{ctx->tgt.x(), ctx->tgt.y(), ctx->tgt.z(), g.info, ctx->qcount, tcell, tslot, nt, 0};
  const Cloud& q = query_cloud(ctx);
  qb.p[1] = QslotArgs{q.x(), q.y(), q.z(), g.info, ctx->qcount2, qcell, qslot, nq, 1};
  // A source that icpk_backproject_pair has just made is in row-major IMAGE order: eight consecutive points are a short
  // run of one image row, as close together as a grid cell's -- the queries are swept in the caller's order and their
  // counting sort is left out (-3.5 us per 92k-point pair, -14 us at 306k; ICPK_IMAGE_ORDER=0: sort them all the same).
  const bool ident = ctx->have_pix_seed && ctx->tune.image_order;
  launch_grid_qslot_batch(qb, ident ? 1 : 2, ctx->stream);
  SetupBatchOf<ScanArgs> sb{};
  sb.p[0] = ScanArgs{ctx->qcount, g.cell_start, ctx->scan_bsum, g.info, 0, 0};
  sb.p[1] = ScanArgs{ctx->qcount2, ctx->qstart, ctx->scan_bsum2, g.info, 1, 0};
  launch_grid_scan_batch(sb, ident ? 1 : 2, ctx->stream);
  const TscatterArgs ta{ctx->tgt.x(), ctx->tgt.y(), ctx->tgt.z(), tcell, tslot, g.cell_start, g.t4, g.o4, nt, 0};
  const bool pix = ctx->have_pix_seed && ctx->tune.pixel_seeds;
  launch_grid_tqscatter(ta, query_scatter_args(ctx, ident ? nullptr : qcell, qslot, ctx->qm4, pix), ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ctx->qcount_dirty = ctx->qcount2_dirty = false;
  ctx->have_grid = true;
  return ICPK_OK;
}

// scan-order copies of the queries and of their seed points (grid scan)
static int ensure_query_points(icpk_ctx* ctx, int nq) {
  const size_t n4 = (size_t)round_up(nq, NN_TILE) + 64;
  bool grown = false;
  const int rc = reserve_group(ctx, &grown, need(ctx->qm4, n4), need(ctx->sp_in, n4), need(ctx->sp_out, n4),
                               need(ctx->rec, 2 * n4));
  if (grown) ctx->grid_chain = false;
  return rc;
}

// Everything a pruned / grid sweep needs before its K1 launch: query order (once per alignment),
// seeds in scan order, buffer rotation.  Enqueues on ctx->stream only for the FIRST sweep of a
// chain; for a sweep that continues a chain of grid sweeps inside a device loop it merely
// rotates pointers.  recheck = 1: the seeds are loose (first sweep).
int prepare_sorted_sweep(icpk_ctx* ctx, int nn_mode, NnArgs& a, NnBoxes& bx, int& recheck) {
  const int nq = ctx->src.n;
  bool grown = false;
  int rc = ctx->qperm.reserve(ctx, round_up(nq, NN_TILE), &grown);
  if (grown) ctx->have_qperm = false;
  if (rc) return rc;
  bx = NnBoxes{};
  bool fresh = false;
  if (nn_mode == ICPK_NN_GRID) {
    bx.ox = ctx->tgt.x();
    bx.oy = ctx->tgt.y();
    bx.oz = ctx->tgt.z();
    // (one size for both counting sorts up front: the target's sort must not see its scratch re-allocated by
    // the queries' -- its launches may only have been recorded so far, see SetupRecorder)
    rc = ensure_sort_buffers(ctx, nq > ctx->tgt.n ? nq : ctx->tgt.n);
    // a fresh pair (no grid yet, no seeds, launches not being recorded for a lock-step group): both sorts side by side
    fresh = !rc && !ctx->have_grid && !ctx->have_seed && !setup_recorder() && ctx->tune.merged_setup && ctx->tgt.n > 0;
    if (fresh) {
      rc = ensure_query_points(ctx, nq);
      if (!rc) rc = build_grid_and_order(ctx);
    } else {
      if (!rc) rc = index_target(ctx, nullptr);
      if (!rc) rc = ensure_query_points(ctx, nq);
    }
  } else {
    rc = prepare_pruned_target(ctx, bx);
  }
  if (rc) return rc;
  bool new_order = false;
  bool points_written = false;  // qm4 / sp_in / seed_m already hold this sweep's queries and seeds
  const int want_kind = nn_mode == ICPK_NN_GRID ? 2 : 1;
  if (fresh) {  // order, scan-order queries and literal seeds were written by build_grid_and_order
    ctx->have_qperm = true;
    ctx->qperm_kind = want_kind;
    new_order = true;
    points_written = true;
  } else if (!ctx->have_qperm || !ctx->have_seed || ctx->qperm_kind != want_kind) {
    // query order (once per alignment), from the source at its current pose: Morton order
    // for the pruned scan (the unsorted Morton keys of the queries stay in sort_keys[0..nq)
    // for its first-sweep seeds), order by grid cell (a cheaper counting sort) for the grid scan
    if (nn_mode == ICPK_NN_GRID) {
      points_written = !ctx->have_seed;
      rc = enqueue_cell_order(ctx, points_written);
    } else {
      rc = enqueue_morton_order(ctx, ctx->src, ctx->qperm);
    }
    if (rc) return rc;
    ctx->have_qperm = true;
    ctx->qperm_kind = want_kind;
    new_order = true;
  }
  recheck = 0;
  if (ctx->have_seed && ctx->have_seed_m && !new_order) {
    // matches of the previous pruned sweep, already in query Morton order
    std::swap(ctx->seed_m, ctx->best_m);
    std::swap(ctx->seed, ctx->best);
  } else if (ctx->have_seed) {  // matches of a sweep by another kernel: bring them into Morton order
    launch_seed_gather(ctx->best, ctx->qperm, nq, ctx->seed_m, ctx->stream);
    std::swap(ctx->seed, ctx->best);
  } else if (nn_mode == ICPK_NN_GRID) {
    // first sweep of the grid scan: the reference's own literal seed, element 0 (icp.cpp:572);
    // the expanding search does not depend on the seed's quality
    if (!points_written) launch_fill_u64(ctx->seed_m, nq, 0ull, nullptr, ctx->stream);
    recheck = 1;
  } else {  // first sweep: the target with the nearest Morton code; loose, so re-check lazily
    launch_seed_morton(ctx->sort_keys, ctx->qperm, nq, ctx->src.x(), ctx->src.y(), ctx->src.z(), ctx->tkeys,
                       ctx->sorted.x(), ctx->sorted.y(), ctx->sorted.z(), ctx->tperm, ctx->tgt.n, ctx->seed_m,
                       ctx->stream);
    recheck = 1;
  }
  a.tx = ctx->sorted.x();
  a.ty = ctx->sorted.y();
  a.tz = ctx->sorted.z();
  a.tiles_per_chunk = a.nt_pad / NN_TILE;
  a.best = ctx->best;
  if (nn_mode == ICPK_NN_GRID) {
    // inside a device loop the grid sweeps keep qm4 / the seed points current themselves;
    // anywhere else the source may have been moved by other kernels: gather afresh
    if (!(ctx->st_active && ctx->grid_chain) && !points_written) {
      const Cloud& q = query_cloud(ctx);
      launch_grid_query_points(q.x(), q.y(), q.z(), ctx->qperm, nq, ctx->seed_m, bx.ox, bx.oy, bx.oz, ctx->qm4, ctx->sp_in,
                               ctx->stream);
    }
  }
  ICPK_HIP(ctx, hipGetLastError());
  return ICPK_OK;
}

// lanes per query of the grid scan (measured with cells 4x finer along x: 8 is best up to 217k queries, 4 from
// 307k on; a launch that fills the GPU several times over is issue-bound and prefers fewer, longer lanes)
static int grid_slices_for(const icpk_ctx* ctx, int nq) { return ctx->tune.grid_slices ? ctx->tune.grid_slices : (nq > 524288 ? 4 : 8); }

// the K1d arguments of the sweep prepare_sorted_sweep has just set up, and the bookkeeping
// that follows its launch
GridSweepArgs grid_sweep_args(icpk_ctx* ctx, const NnArgs& a, const NnBoxes& bx) {
  GridSweepArgs g{};
  g.qx = const_cast<float*>(a.qx);
  g.qy = const_cast<float*>(a.qy);
  g.qz = const_cast<float*>(a.qz);
  g.nq = a.nq;
  g.qm4 = ctx->qm4;
  g.t4 = ctx->grid.t4;
  g.cell_start = ctx->grid.cell_start;
  g.gi = ctx->grid.info;
  g.ox = bx.ox;
  g.oy = bx.oy;
  g.oz = bx.oz;
  g.sp_in = ctx->sp_in;
  g.sp_out = ctx->sp_out;
  g.best = a.best;
  g.best_m = ctx->best_m;
  g.st = ctx->st_active;
  g.rec = ctx->st_active ? ctx->rec : nullptr;  // inside a device loop K2 reads the records; planes / keys once at the end
  return g;
}
void after_grid_sweep(icpk_ctx* ctx) {
  std::swap(ctx->sp_in, ctx->sp_out);
  ctx->grid_chain = ctx->st_active != nullptr;
  ctx->have_assoc = true;
  ctx->have_seed = true;
  ctx->have_seed_m = true;
}

NnArgs base_nn_args(const icpk_ctx* ctx) {
  NnArgs a;
  a.qx = ctx->src.x();
  a.qy = ctx->src.y();
  a.qz = ctx->src.z();
  a.nq = ctx->src.n;
  a.tx = ctx->tgt.x();
  a.ty = ctx->tgt.y();
  a.tz = ctx->tgt.z();
  a.nt_pad = round_up(ctx->tgt.n, NN_TILE);
  a.tiles_per_chunk = a.nt_pad / NN_TILE;
  a.best = ctx->best;
  a.stop = ctx->stop;
  return a;
}

// enqueue one NN sweep (K1) over the working source; ev0/ev1 (optional) are recorded
// immediately before/after the K1 launch itself, so that set-up kernels of a first sweep
// (sort, seeding, fills) do not count as kernel time
int enqueue_nn(icpk_ctx* ctx, int nn_mode, hipEvent_t ev0, hipEvent_t ev1) {
  auto mark = [&](hipEvent_t e) -> int {
    if (e) ICPK_HIP(ctx, hipEventRecord(e, ctx->stream));
    return ICPK_OK;
  };
  if (nn_mode != ICPK_NN_EXACT && nn_mode != ICPK_NN_FILTERED && nn_mode != ICPK_NN_PRUNED && nn_mode != ICPK_NN_GRID &&
      nn_mode != ICPK_NN_MAP)
    return fail(ctx, ICPK_E_ARG, "unknown nn_mode");
  if (nn_mode == ICPK_NN_MAP && !icpk_map_lookup_current(ctx))
    return fail(ctx, ICPK_E_ARG, "ICPK_NN_MAP needs the map's current lookup target (icpk_map_lookup_to_target)");
  const int nq = ctx->src.n;
  int rc = ensure_assoc(ctx, nq);
  if (rc) return rc;
  if (nq == 0) {
    ctx->have_assoc = true;
    return ICPK_OK;
  }
  auto chunking = [&](int nqb, int ntiles) {
    int nchunks = (ctx->tune.target_blocks + nqb - 1) / nqb;
    if (nchunks < 1) nchunks = 1;
    if (nchunks > ntiles) nchunks = ntiles;
    return (ntiles + nchunks - 1) / nchunks;
  };
  NnArgs a = base_nn_args(ctx);
  const int ntiles = a.nt_pad / NN_TILE;
  if (nn_mode != ICPK_NN_GRID && (rc = flush_loop_init(ctx))) return rc;  // (their fills and kernels look at the state)
  if (nn_mode == ICPK_NN_MAP) {  // K9 (icpk_map.cpp): the sweep's keys index the lookup target
    if ((rc = mark(ev0))) return rc;
    if ((rc = icpk_map_nn_sweep(ctx))) return rc;
    if ((rc = mark(ev1))) return rc;
    ICPK_HIP(ctx, hipGetLastError());
    ctx->grid_chain = false;
    ctx->have_assoc = true;
    ctx->have_seed = false;  // (a lookup result is no nearest target: it must not seed a filtered sweep)
    ctx->have_seed_m = false;
    return ICPK_OK;
  }
  if (nn_mode == ICPK_NN_EXACT) {
    a.tiles_per_chunk = chunking((nq + NN_THREADS - 1) / NN_THREADS, ntiles);
    a.best = ctx->best;
    launch_fill_u64(ctx->best, nq, NN_KEY_INIT, ctx->stop, ctx->stream);
    if ((rc = mark(ev0))) return rc;
    launch_nn_exact(a, ctx->stream);
    if ((rc = mark(ev1))) return rc;
  } else if (nn_mode == ICPK_NN_PRUNED || nn_mode == ICPK_NN_GRID) {
    NnBoxes bx{};
    int recheck = 0;
    rc = prepare_sorted_sweep(ctx, nn_mode, a, bx, recheck);
    if (rc) return rc;
    if ((rc = flush_loop_init(ctx))) return rc;  // (unless the set-up's first launch has carried it)
    if ((rc = mark(ev0))) return rc;
    if (nn_mode == ICPK_NN_GRID) {
      launch_nn_grid(grid_sweep_args(ctx, a, bx), grid_slices_for(ctx, nq), recheck, ctx->stream);
      after_grid_sweep(ctx);
    } else {
      // lanes per query: as many as keep the launch at <= ~10k waves (measured best: 16 at 10k
      // queries, 4 at 92k, 2 at 217k-307k, 1 at 10^6)
      int slices = ctx->tune.slices;
      if (slices == 0) {
        slices = 16;
        while (slices > 1 && (long long)nq * slices / 64 > 10000) slices >>= 1;
      }
      launch_nn_pruned(a, ctx->seed_m, ctx->best_m, bx, slices, recheck, ctx->st_active, ctx->stream);
      ctx->grid_chain = false;
      ctx->have_assoc = true;
      ctx->have_seed = true;
      ctx->have_seed_m = true;
    }
    if ((rc = mark(ev1))) return rc;
    ICPK_HIP(ctx, hipGetLastError());
    return ICPK_OK;
  } else {
    int seed_scale = 1;
    if (ctx->have_seed) {
      // matches of the previous sweep (same clouds, source possibly moved) seed this one
      std::swap(ctx->seed, ctx->best);
    } else {
      // coarse pre-pass: exact NN against every NN_SEED_STRIDE-th target
      if (!ctx->have_dec) {
        const int nd = (ctx->tgt.n + NN_SEED_STRIDE - 1) / NN_SEED_STRIDE;
        rc = ensure_cloud(ctx, ctx->dec, nd);
        if (rc) return rc;
        launch_decimate(ctx->tgt.x(), ctx->tgt.y(), ctx->tgt.z(), ctx->tgt.n, NN_SEED_STRIDE, ctx->dec.x(),
                        ctx->dec.y(), ctx->dec.z(), round_up(nd, NN_TILE), ctx->stream);
        ctx->have_dec = true;
      }
      NnArgs c = a;
      c.tx = ctx->dec.x();
      c.ty = ctx->dec.y();
      c.tz = ctx->dec.z();
      c.nt_pad = round_up(ctx->dec.n, NN_TILE);
      c.tiles_per_chunk = chunking((nq + NN_THREADS - 1) / NN_THREADS, c.nt_pad / NN_TILE);
      c.best = ctx->seed;
      launch_fill_u64(ctx->seed, nq, NN_KEY_INIT, ctx->stop, ctx->stream);
      launch_nn_exact(c, ctx->stream);
      seed_scale = NN_SEED_STRIDE;
    }
    const int q = ctx->tune.q_per_lane > 0 ? ctx->tune.q_per_lane : (nq >= 65536 ? 2 : 1);
    a.tiles_per_chunk = chunking((nq + NN_THREADS * q - 1) / (NN_THREADS * q), ntiles);
    a.best = ctx->best;
    launch_fill_u64(ctx->best, nq, NN_KEY_INIT, ctx->stop, ctx->stream);
    if ((rc = mark(ev0))) return rc;
    launch_nn_filtered(a, ctx->seed, seed_scale, q, ctx->stream);
    if ((rc = mark(ev1))) return rc;
  }
  ICPK_HIP(ctx, hipGetLastError());
  ctx->have_assoc = true;
  ctx->have_seed = true;
  ctx->have_seed_m = false;  // exact / filtered sweeps leave their matches in the caller's order only
  return ICPK_OK;
}

// the records of the grid sweep just enqueued, if it was one of a device loop (then planes and keys are stale until
// the loop's final unpack)
const float4* loop_rec(const icpk_ctx* ctx) { return ctx->st_active && ctx->grid_chain ? ctx->rec : nullptr; }

// outside a device loop: the sums and the pair count of the reduction just enqueued into red_host (not waited for)
static int read_back_sums(icpk_ctx* ctx, int nsum) {
  ICPK_HIP(ctx, hipGetLastError());
  if (!ctx->st_active)
    ICPK_HIP(ctx, hipMemcpyAsync(ctx->red_host, ctx->red_out, (nsum + 1) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  return ICPK_OK;
}

// what every reduction takes from the context; inside a device loop nothing is unpacked and no final stage runs (the
// loop step sums the partials)
static PairArgs reduce_args(icpk_ctx* ctx, float max_dist) {
  const bool loop = ctx->st_active;
  PairArgs a{};
  a.best = ctx->best;
  a.ax = ctx->src.x(), a.ay = ctx->src.y(), a.az = ctx->src.z();
  a.tx = ctx->tgt.x(), a.ty = ctx->tgt.y(), a.tz = ctx->tgt.z();
  a.o4 = ctx->have_grid ? ctx->grid.o4.get() : nullptr;
  a.rec = loop_rec(ctx);
  a.nq = ctx->src.n;
  a.max_dist = max_dist;
  a.idx_out = loop ? nullptr : ctx->idx.get();
  a.dist_out = loop ? nullptr : ctx->dist.get();
  a.partial = ctx->partial;
  a.pcount = ctx->pcount;
  a.out = loop ? nullptr : ctx->red_out.get();
  a.st = ctx->st_active;
  return a;
}

// enqueue K2 and the 160-byte read-back; caller synchronises
int enqueue_reduce(icpk_ctx* ctx, float max_dist) {
  launch_assoc_reduce(reduce_args(ctx, max_dist), ctx->st_active ? ctx->loop_nact : NSUM, ctx->stream);
  return read_back_sums(ctx, NSUM);
}

// point-to-plane flavour of enqueue_reduce (K5)
int enqueue_reduce_p2l(icpk_ctx* ctx, float max_dist) {
  launch_p2l_reduce(reduce_args(ctx, max_dist), ctx->nrm.x(), ctx->nrm.y(), ctx->nrm.z(), ctx->stream);
  return read_back_sums(ctx, NP2L);
}

int enqueue_reduce_gicp(icpk_ctx* ctx, float max_dist, const float* R_acc) {
  GicpArgs g{};
  g.snx = ctx->snrm.x(), g.sny = ctx->snrm.y(), g.snz = ctx->snrm.z();
  g.tnx = ctx->nrm.x(), g.tny = ctx->nrm.y(), g.tnz = ctx->nrm.z();
  for (int k = 0; k < 9; ++k) g.R[k] = R_acc ? R_acc[k] : (k % 4 == 0 ? 1.f : 0.f);
  g.epsilon = ctx->gicp_epsilon;
  launch_gicp_reduce(reduce_args(ctx, max_dist), g, ctx->stream);
  return read_back_sums(ctx, NP2L);
}

int enqueue_reduce_colored(icpk_ctx* ctx, float max_dist) {
  ColoredArgs g{};
  g.tnx = ctx->nrm.x(), g.tny = ctx->nrm.y(), g.tnz = ctx->nrm.z();
  g.gx = ctx->cgrad.x(), g.gy = ctx->cgrad.y(), g.gz = ctx->cgrad.z();
  g.tcol = ctx->tcol;
  g.scol = ctx->scol;
  g.lambda_geometric = ctx->lambda_geometric;
  launch_colored_reduce(reduce_args(ctx, max_dist), g, ctx->stream);
  return read_back_sums(ctx, NP2L);
}

int ensure_robust(icpk_ctx* ctx, int nq) {
  int rc = ctx->rsel.reserve(ctx, 1);
  if (!rc) rc = ctx->rsel_host.reserve(ctx, 1);
  if (!rc) rc = ctx->rhist.reserve(ctx, 2 * SEL_BINS);
  if (!rc) rc = ctx->rdsel.reserve(ctx, round_up(nq < 1 ? 1 : nq, NN_TILE));
  if (!rc && !ctx->robust_trace_pin) {
    rc = ctx->robust_trace_pin.reserve(ctx, LOOP_MAX_ITER);
    void* d = nullptr;
    if (!rc) ICPK_HIP(ctx, hipHostGetDevicePointer(&d, ctx->robust_trace_pin.get(), 0));
    ctx->robust_trace_dev = static_cast<RobustTraceEntry*>(d);
  }
  if (rc) return rc;
  // (each scan clears what its pass filled; this makes a selection cut short by an earlier error harmless)
  ICPK_HIP(ctx, hipMemsetAsync(ctx->rhist, 0, 2 * SEL_BINS * sizeof(int), ctx->stream));
  return ICPK_OK;
}

int enqueue_reduce_robust(icpk_ctx* ctx, float max_dist, bool p2l) {
  const int nq = ctx->src.n;
  const icpk_robust& r = ctx->robust;
  const RobustCfg cfg{r.kernel, r.scale_mode, r.scale, r.trim_fraction};
  const float4* rec = loop_rec(ctx);
  launch_robust_select(ctx->best, rec, nq, max_dist, p2l ? ctx->nrm.x() : nullptr, p2l ? ctx->nrm.y() : nullptr,
                       p2l ? ctx->nrm.z() : nullptr, ctx->rdsel, ctx->rhist, ctx->rsel, cfg, ctx->st_active, ctx->stream);
  const PairArgs a = reduce_args(ctx, max_dist);
  if (p2l)
    launch_p2l_reduce(a, ctx->nrm.x(), ctx->nrm.y(), ctx->nrm.z(), ctx->stream, ctx->rsel);
  else
    launch_assoc_reduce(a, NSUM_W, ctx->stream, ctx->rsel);
  const int rc = read_back_sums(ctx, p2l ? NP2L_W : NSUM_W);
  if (rc || ctx->st_active) return rc;
  ICPK_HIP(ctx, hipMemcpyAsync(ctx->rsel_host, ctx->rsel, sizeof(RobustSel), hipMemcpyDeviceToHost, ctx->stream));
  return ICPK_OK;
}

// ---- deferred set-up launches (icpk_internal.h) ----
SetupRecorder*& setup_recorder() {
  static thread_local SetupRecorder* rec = nullptr;
  return rec;
}

// every pair of the group recorded the same steps in the same order?
static bool same_sequences(const SetupRecorder* recs, int count) {
  for (int k = 0; k < count; ++k) {
    if (recs[k].overflow || recs[k].n != recs[0].n) return false;
    for (int j = 0; j < recs[0].n; ++j)
      if (recs[k].calls[j].kind != recs[0].calls[j].kind) return false;
  }
  return true;
}

// THE table of the set-up steps: kind, the union's member, its type, the single launch, the batch launch
#define ICPK_SETUP_STEPS(X)                                                                   \
  X(SK_INGEST, ingest, IngestArgs, launch_ingest_cloud, launch_ingest_batch)                  \
  X(SK_LOOP_INIT, loop_init, LoopInitArgs, launch_loop_init, launch_loop_init_batch)          \
  X(SK_BOUNDS, bounds, BoundsArgs, launch_grid_bounds, launch_grid_bounds_batch)              \
  X(SK_INFO, info, InfoArgs, launch_grid_info, launch_grid_info_batch)                        \
  X(SK_QSLOT, qslot, QslotArgs, launch_grid_qslot, launch_grid_qslot_batch)                   \
  X(SK_SCAN, scan, ScanArgs, launch_grid_scan, launch_grid_scan_batch)                        \
  X(SK_TSCATTER, tscatter, TscatterArgs, launch_grid_tscatter, launch_grid_tscatter_batch)    \
  X(SK_QSCATTER, qscatter, QscatterArgs, launch_grid_qscatter, launch_grid_qscatter_batch)

bool flush_setup_batches(const SetupRecorder* recs, int count, hipStream_t s) {
  if (count <= 0) return true;
  if (count > BATCH_MAX || !same_sequences(recs, count)) return false;
  for (int j = 0; j < recs[0].n; ++j) {
#define ICPK_BATCH_STEP(KIND, FIELD, TYPE, LAUNCH, BATCH)            \
  case KIND: {                                                      \
    SetupBatchOf<TYPE> b;                                           \
    for (int k = 0; k < count; ++k) b.p[k] = recs[k].calls[j].FIELD; \
    BATCH(b, count, s);                                             \
    break;                                                          \
  }
    switch (recs[0].calls[j].kind) {
      ICPK_SETUP_STEPS(ICPK_BATCH_STEP)
      default: return false;
    }
#undef ICPK_BATCH_STEP
  }
  return true;
}

// one pair's recorded steps, launched one by one (the sequences of a group differed)
void replay_setup(const SetupRecorder& rec, hipStream_t s) {
  SetupRecorder* const saved = setup_recorder();
  setup_recorder() = nullptr;  // (the launchers launch)
  for (int j = 0; j < rec.n; ++j) {
    const SetupCall& c = rec.calls[j];
#define ICPK_REPLAY_STEP(KIND, FIELD, TYPE, LAUNCH, BATCH) \
  case KIND: LAUNCH(c.FIELD, s); break;
    switch (c.kind) {
      ICPK_SETUP_STEPS(ICPK_REPLAY_STEP)
      default: break;
    }
#undef ICPK_REPLAY_STEP
  }
  setup_recorder() = saved;
}
#undef ICPK_SETUP_STEPS
}  // namespace icpk

// icpk_reduce / icpk_reduce_p2l: K2 / K5 over the current associations, sums and pair count back to the host
static int reduce_to_host(icpk_ctx* ctx, float max_dist, double* sums, int64_t* count, bool p2l) {
  if (!ctx || !sums) return ICPK_E_ARG;
  if (!ctx->have_assoc) return fail(ctx, ICPK_E_NOT_SET, "no nearest-neighbour sweep has run");
  if (p2l && !ctx->have_normals) return fail(ctx, ICPK_E_NOT_SET, "no target normals");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (int ru = ensure_unpacked(ctx)) return ru;
  const int nsum = p2l ? NP2L : NSUM;
  if (ctx->src.n == 0) {
    std::memset(sums, 0, nsum * sizeof(double));
    if (count) *count = 0;
    return ICPK_OK;
  }
  int rc = p2l ? enqueue_reduce_p2l(ctx, max_dist) : enqueue_reduce(ctx, max_dist);
  if (rc) return rc;
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  std::memcpy(sums, ctx->red_host, nsum * sizeof(double));
  if (count) std::memcpy(count, ctx->red_host + nsum, sizeof(int64_t));
  return ICPK_OK;
}

extern "C" {

int icpk_get_associations(icpk_ctx* ctx, int32_t* idx_out, float* dist_out) {
  if (!ctx) return ICPK_E_ARG;
  if (!ctx->have_assoc) return fail(ctx, ICPK_E_NOT_SET, "no nearest-neighbour sweep has run");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  const int nq = ctx->src.n;
  if (int ru = ensure_unpacked(ctx)) return ru;  // (after a device loop of grid sweeps; a frame-batch slot after its lock-step loop)
  if (nq > 0) {
    // K2 unpacks (distance, index) keys into the idx/dist planes
    int rc = enqueue_reduce(ctx, __builtin_inff());
    if (rc) return rc;
    if (idx_out)
      ICPK_HIP(ctx, hipMemcpyAsync(idx_out, ctx->idx, (size_t)nq * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (dist_out)
      ICPK_HIP(ctx, hipMemcpyAsync(dist_out, ctx->dist, (size_t)nq * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  }
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_nn(icpk_ctx* ctx, int32_t nn_mode, int32_t* idx_out, float* dist_out) {
  int rc = check_ready(ctx);
  if (rc) return rc;
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (int ru = ensure_unpacked(ctx)) return ru;
  rc = enqueue_nn(ctx, nn_mode);
  if (rc) return rc;
  if (idx_out || dist_out) return icpk_get_associations(ctx, idx_out, dist_out);
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return ICPK_OK;
}

int icpk_reduce(icpk_ctx* ctx, float max_dist, double* sums, int64_t* count) {
  return reduce_to_host(ctx, max_dist, sums, count, false);
}

int icpk_reduce_p2l(icpk_ctx* ctx, float max_dist, double* sums, int64_t* count) {
  return reduce_to_host(ctx, max_dist, sums, count, true);
}

int icpk_reduce_weighted(icpk_ctx* ctx, float max_dist, int32_t solve, double* sums, int64_t* accepted, int64_t* kept,
                         float* cut, float* median, double* c) {
  if (!ctx || !sums || (solve != ICPK_SOLVE_KABSCH && solve != ICPK_SOLVE_POINT_TO_PLANE)) return ICPK_E_ARG;
  if (!ctx->robust_on) return fail(ctx, ICPK_E_NOT_SET, "robust alignment is off (icpk_set_robust)");
  if (!ctx->have_assoc) return fail(ctx, ICPK_E_NOT_SET, "no nearest-neighbour sweep has run");
  const bool p2l = solve == ICPK_SOLVE_POINT_TO_PLANE;
  if (p2l && !ctx->have_normals) return fail(ctx, ICPK_E_NOT_SET, "no target normals");
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  if (int ru = ensure_unpacked(ctx)) return ru;
  const int nsum = p2l ? NP2L_W : NSUM_W;
  RobustSel sel{};
  int64_t n = 0;
  if (ctx->src.n == 0) {
    std::memset(sums, 0, nsum * sizeof(double));
    sel.c = ctx->robust.scale_mode == ICPK_SCALE_MEDIAN ? 0.0 : (double)ctx->robust.scale;
  } else {
    int rc = ensure_robust(ctx, ctx->src.n);
    if (!rc) rc = enqueue_reduce_robust(ctx, max_dist, p2l);
    if (rc) return rc;
    ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(sums, ctx->red_host, nsum * sizeof(double));
    std::memcpy(&n, ctx->red_host + nsum, sizeof(int64_t));
    sel = *ctx->rsel_host;
  }
  if (accepted) *accepted = n;
  if (kept) *kept = (int64_t)sums[nsum - 1];
  if (cut) *cut = sel.cut;
  if (median) *median = sel.median;
  if (c) *c = sel.c;
  return ICPK_OK;
}

}  // extern "C"
