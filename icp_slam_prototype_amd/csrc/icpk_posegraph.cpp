// icpk_posegraph.cpp -- host side of pose-graph optimisation (K18; kernels_posegraph.hip): the refusals, the adjacency
// list, the Levenberg-Marquardt loop (one host wait per iteration: the cost, the gain ratio, the decision) and the
// pruning of the line process.  The rule is written out in include/icpk.h.
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "icpk_ctx.h"

using namespace icpk;

static_assert(sizeof(PgEdge) == sizeof(icpk_pg_edge) && offsetof(PgEdge, T) == offsetof(icpk_pg_edge, T) &&
                  offsetof(PgEdge, info) == offsetof(icpk_pg_edge, info) &&
                  offsetof(PgEdge, uncertain) == offsetof(icpk_pg_edge, uncertain),
              "the device reads icpk_pg_edge as it is");

namespace {

bool all_finite(const double* v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

bool tolerance_ok(double v) { return std::isfinite(v) && v >= 0.0; }

// nullptr: fine; else what is wrong
const char* check_graph(int32_t n_nodes, const double* poses, int32_t n_edges, const icpk_pg_edge* edges,
                        const icpk_pg_params* p) {
  if (!poses || !edges) return "poses and edges must not be NULL";
  if (n_nodes < 2 || n_nodes > ICPK_PG_MAX_NODES) return "n_nodes outside 2 .. ICPK_PG_MAX_NODES";
  if (n_edges < 1 || n_edges > ICPK_PG_MAX_EDGES) return "n_edges outside 1 .. ICPK_PG_MAX_EDGES";
  if (p->reference_node < 0 || p->reference_node >= n_nodes) return "reference_node out of range";
  if (p->flags & ~ICPK_PG_PRUNE) return "unknown pose-graph flag";
  if (p->max_iterations < 0 || p->max_pcg_iterations < 1) return "max_iterations < 0 or max_pcg_iterations < 1";
  if (!tolerance_ok(p->pcg_tolerance) || !tolerance_ok(p->cost_tolerance) || !tolerance_ok(p->step_tolerance) ||
      !tolerance_ok(p->gradient_tolerance) || !tolerance_ok(p->preference_loop_closure) ||
      !tolerance_ok(p->edge_prune_threshold) || !tolerance_ok(p->tau) || !(p->tau > 0.0))
    return "a tolerance, tau, preference_loop_closure or edge_prune_threshold is negative or not finite";
  if (!all_finite(poses, 16 * (size_t)n_nodes)) return "a pose is not finite";
  std::vector<int32_t> parent((size_t)n_nodes);
  std::iota(parent.begin(), parent.end(), 0);
  auto find = [&](int32_t i) {
    while (parent[i] != i) i = parent[i] = parent[parent[i]];
    return i;
  };
  for (int32_t e = 0; e < n_edges; ++e) {
    const icpk_pg_edge& ed = edges[e];
    if (ed.source < 0 || ed.source >= n_nodes || ed.target < 0 || ed.target >= n_nodes) return "an edge's node index is out of range";
    if (ed.source == ed.target) return "an edge joins a node to itself";
    if (!all_finite(ed.T, 16) || !all_finite(ed.info, 36)) return "an edge's T or information matrix is not finite";
    const int32_t a = find(ed.source), b = find(ed.target);
    if (a != b) parent[a < b ? b : a] = a < b ? a : b;
  }
  const int32_t root = find(p->reference_node);
  for (int32_t i = 0; i < n_nodes; ++i)
    if (find(i) != root) return "a node cannot be reached from the reference node";
  return nullptr;
}

// the buffers of one call, carved out of the context's
struct Work {
  PgArgs a{};
  PgLin lin[2]{};
  double* poses[2]{};
  int nbe = 0, nbn = 0;
};

int reserve(icpk_ctx* ctx, int n_nodes, int n_edges, Work& w) {
  const size_t n = (size_t)n_nodes, m = (size_t)n_edges;
  int rc = ctx->pg_edges.reserve(ctx, m);
  if (!rc) rc = ctx->pg_adj.reserve(ctx, n + 1 + 2 * m);
  if (!rc) rc = ctx->pg_edge_f64.reserve(ctx, 2 * 44 * m);
  if (!rc) rc = ctx->pg_node_f64.reserve(ctx, n * (2 * 16 + 2 * 42 + 36 + 5 * 6));
  if (!rc) rc = ctx->pg_partial.reserve(ctx, (size_t)PG_NPARTIAL * RED_MAX_BLOCKS);
  if (!rc) rc = ctx->pg_scal.reserve(ctx, 1);
  if (!rc) rc = ctx->pg_scal_host.reserve(ctx, 1);
  if (rc) return rc;
  double* f = ctx->pg_edge_f64;
  for (int k = 0; k < 2; ++k) {
    w.lin[k].A = f, f += 36 * m;
    w.lin[k].b = f, f += 6 * m;
    w.lin[k].chi2 = f, f += m;
    w.lin[k].l = f, f += m;
  }
  f = ctx->pg_node_f64;
  for (int k = 0; k < 2; ++k) w.poses[k] = f, f += 16 * n;
  for (int k = 0; k < 2; ++k) {
    w.lin[k].D = f, f += 36 * n;
    w.lin[k].g = f, f += 6 * n;
    w.lin[k].poses = w.poses[k];
  }
  w.a.L = f, f += 36 * n;
  w.a.x = f, f += 6 * n;
  w.a.r = f, f += 6 * n;
  w.a.z = f, f += 6 * n;
  w.a.p = f, f += 6 * n;
  w.a.q = f, f += 6 * n;
  w.a.n_nodes = n_nodes;
  w.a.edges = ctx->pg_edges;
  w.a.adj_start = ctx->pg_adj;
  w.a.adj = ctx->pg_adj + (n + 1);
  w.a.partial = ctx->pg_partial;
  w.a.scal = ctx->pg_scal;
  return ICPK_OK;
}

// the m edges at `list` (the caller's array as it stands, or the kept ones) and their adjacency list onto the device;
// every node's entries in ascending edge index (a counting sort over the edges in order)
int upload_edges(icpk_ctx* ctx, Work& w, const icpk_pg_edge* list, int m) {
  const int n = w.a.n_nodes;
  std::vector<int> adj((size_t)n + 1 + 2 * (size_t)m, 0);
  int* start = adj.data();
  int* ent = adj.data() + n + 1;
  for (int e = 0; e < m; ++e) start[list[e].source + 1] += 1, start[list[e].target + 1] += 1;
  for (int i = 0; i < n; ++i) start[i + 1] += start[i];
  std::vector<int> fill(start, start + n);
  for (int e = 0; e < m; ++e) {
    ent[fill[list[e].source]++] = 2 * e;
    ent[fill[list[e].target]++] = 2 * e + 1;
  }
  w.a.n_edges = m;
  ICPK_HIP(ctx, hipMemcpyAsync(ctx->pg_edges, list, (size_t)m * sizeof(icpk_pg_edge), hipMemcpyHostToDevice, ctx->stream));
  ICPK_HIP(ctx, hipMemcpyAsync(ctx->pg_adj, adj.data(), adj.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (adj goes away, and `list` may)
  return ICPK_OK;
}

// the scalars of what has been enqueued: the one host wait
int read_scalars(icpk_ctx* ctx, PgScalars& s) {
  ICPK_HIP(ctx, hipGetLastError());
  ICPK_HIP(ctx, hipMemcpyAsync(ctx->pg_scal_host, ctx->pg_scal, sizeof(PgScalars), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  s = *ctx->pg_scal_host;
  return ICPK_OK;
}

// Levenberg-Marquardt over the edges on the device, from lin[cur]'s poses; cur follows the accepted steps.
// *converged: a stopping rule other than max_iterations ended it
int run_lm(icpk_ctx* ctx, Work& w, const icpk_pg_params& p, int& cur, icpk_pg_result& res, double& cost, bool& converged) {
  PgScalars s{};
  launch_pg_linearise(w.a, w.lin[cur], true, ctx->stream);
  if (int rc = read_scalars(ctx, s)) return rc;
  cost = s.cost;
  if (res.iterations == 0 && res.n_pruned == 0) res.initial_cost = cost;  // (the first run's)
  double lambda = p.tau * s.hmax, nu = 2.0;
  res.final_lambda = lambda;
  converged = s.gmax < p.gradient_tolerance;
  for (int it = 0; it < p.max_iterations && !converged; ++it) {
    const int alt = cur ^ 1;
    launch_pg_solve(w.a, w.lin[cur], lambda, p.pcg_tolerance, p.max_pcg_iterations, w.poses[alt], ctx->stream);
    launch_pg_linearise(w.a, w.lin[alt], true, ctx->stream);
    if (int rc = read_scalars(ctx, s)) return rc;
    const double rho = s.pred > 0.0 ? (cost - s.cost) / s.pred : -1.0;
    const bool accepted = rho > 0.0;
    res.iterations += 1;
    res.pcg_iterations += s.pcg_iters;
    ctx->pg_trace_lambda.push_back(lambda);
    ctx->pg_trace_pcg.push_back(s.pcg_iters);
    ctx->pg_trace_accepted.push_back(accepted ? 1 : 0);
    if (accepted) {
      const double rel = cost > 0.0 ? (cost - s.cost) / cost : 0.0;
      res.accepted += 1;
      cur = alt;
      cost = s.cost;
      const double c = 2.0 * rho - 1.0;
      const double f = 1.0 - c * c * c;
      lambda = lambda * (f > 1.0 / 3.0 ? f : 1.0 / 3.0);
      nu = 2.0;
      converged = rel < p.cost_tolerance || s.dmax < p.step_tolerance || s.gmax < p.gradient_tolerance;
    } else {
      lambda = lambda * nu;
      nu = 2.0 * nu;
      converged = s.dmax < p.step_tolerance;
    }
    ctx->pg_trace_cost.push_back(cost);
    res.final_lambda = lambda;
  }
  return ICPK_OK;
}

}  // namespace

extern "C" {

void icpk_default_pg_params(icpk_pg_params* p) {
  if (!p) return;
  p->max_iterations = 100;
  p->max_pcg_iterations = 200;
  p->pcg_tolerance = 1e-8;
  p->tau = 1e-3;
  p->cost_tolerance = 1e-9;
  p->step_tolerance = 1e-10;
  p->gradient_tolerance = 1e-10;
  p->preference_loop_closure = 0.0;
  p->edge_prune_threshold = 0.25;
  p->reference_node = 0;
  p->flags = 0;
}

int icpk_pose_graph_check(int32_t n_nodes, const double* poses, int32_t n_edges, const icpk_pg_edge* edges,
                          const icpk_pg_params* params) {
  icpk_pg_params d;
  icpk_default_pg_params(&d);
  return check_graph(n_nodes, poses, n_edges, edges, params ? params : &d) ? ICPK_E_ARG : ICPK_OK;
}

int icpk_pose_graph_optimize(icpk_ctx* ctx, int32_t n_nodes, double* poses, int32_t n_edges, const icpk_pg_edge* edges,
                             const icpk_pg_params* params, icpk_pg_result* result, double* edge_weight_out,
                             double* edge_chi2_out, uint8_t* pruned_out) {
  if (!ctx) return ICPK_E_ARG;
  icpk_pg_params p;
  icpk_default_pg_params(&p);
  if (params) p = *params;
  if (const char* why = check_graph(n_nodes, poses, n_edges, edges, &p)) return fail(ctx, ICPK_E_ARG, why);
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  ctx->pg_trace_cost.clear(), ctx->pg_trace_lambda.clear(), ctx->pg_trace_pcg.clear(), ctx->pg_trace_accepted.clear();
  Work w;
  if (int rc = reserve(ctx, n_nodes, n_edges, w)) return rc;
  w.a.ref = p.reference_node;
  w.a.mu = p.preference_loop_closure;
  const size_t pose_bytes = 16 * (size_t)n_nodes * sizeof(double);
  ICPK_HIP(ctx, hipMemsetAsync(ctx->pg_partial, 0, (size_t)PG_NPARTIAL * RED_MAX_BLOCKS * sizeof(double), ctx->stream));
  ICPK_HIP(ctx, hipMemcpyAsync(w.poses[0], poses, pose_bytes, hipMemcpyHostToDevice, ctx->stream));
  if (int rc = upload_edges(ctx, w, edges, n_edges)) return rc;
  icpk_pg_result res{};
  int cur = 0;
  double cost = 0.0;
  bool converged = false;
  if (int rc = run_lm(ctx, w, p, cur, res, cost, converged)) return rc;
  bool all_converged = converged;
  std::vector<double> l((size_t)n_edges), chi2((size_t)n_edges);
  std::vector<uint8_t> pruned((size_t)n_edges, 0);
  if ((p.flags & ICPK_PG_PRUNE) && p.preference_loop_closure > 0.0) {
    ICPK_HIP(ctx, hipMemcpyAsync(l.data(), w.lin[cur].l, (size_t)n_edges * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int e = 0; e < n_edges; ++e) {
      pruned[e] = edges[e].uncertain && l[e] < p.edge_prune_threshold;
      res.n_pruned += pruned[e];
    }
    if (res.n_pruned > 0) {  // (the only copy of edges this call makes, and only the kept ones)
      std::vector<icpk_pg_edge> kept;
      kept.reserve((size_t)(n_edges - res.n_pruned));
      for (int e = 0; e < n_edges; ++e)
        if (!pruned[e]) kept.push_back(edges[e]);
      // The rule: when the kept edges no longer join every node to the reference node (the dropped ones were the only
      // way to some node), NOTHING is pruned: the mask is all zero, n_pruned is 0 and there is no second run
      if (check_graph(n_nodes, poses, (int32_t)kept.size(), kept.data(), &p)) {
        std::fill(pruned.begin(), pruned.end(), 0);
        res.n_pruned = 0;
      } else {
        if (int rc = upload_edges(ctx, w, kept.data(), (int)kept.size())) return rc;
        if (int rc = run_lm(ctx, w, p, cur, res, cost, converged)) return rc;
        all_converged = all_converged && converged;
        if (int rc = upload_edges(ctx, w, edges, n_edges)) return rc;
      }
    }
  }
  res.final_cost = cost;
  // l and chi2 of every edge at the final poses: one edge pass without blocks into the other linearisation's arrays
  PgLin ev = w.lin[cur ^ 1];
  ev.poses = w.poses[cur];
  ev.A = nullptr, ev.b = nullptr;
  launch_pg_linearise(w.a, ev, false, ctx->stream);
  ICPK_HIP(ctx, hipGetLastError());
  ICPK_HIP(ctx, hipMemcpyAsync(l.data(), ev.l, (size_t)n_edges * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipMemcpyAsync(chi2.data(), ev.chi2, (size_t)n_edges * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  std::vector<double> out(16 * (size_t)n_nodes);
  ICPK_HIP(ctx, hipMemcpyAsync(out.data(), w.poses[cur], pose_bytes, hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  // (the reference node's pose never left the caller's array: the device copied its bytes from step to step)
  std::memcpy(poses, out.data(), pose_bytes);
  if (edge_weight_out) std::memcpy(edge_weight_out, l.data(), l.size() * sizeof(double));
  if (edge_chi2_out) std::memcpy(edge_chi2_out, chi2.data(), chi2.size() * sizeof(double));
  if (pruned_out) std::memcpy(pruned_out, pruned.data(), pruned.size());
  if (result) *result = res;
  return all_converged ? ICPK_OK : ICPK_W_NOT_CONVERGED;
}

int icpk_pose_graph_evaluate(icpk_ctx* ctx, int32_t n_nodes, const double* poses, int32_t n_edges,
                             const icpk_pg_edge* edges, double mu, double* chi2_out, double* weight_out, double* cost_out,
                             double* gradient_out) {
  if (!ctx) return ICPK_E_ARG;
  icpk_pg_params p;
  icpk_default_pg_params(&p);
  p.preference_loop_closure = mu;
  if (const char* why = check_graph(n_nodes, poses, n_edges, edges, &p)) return fail(ctx, ICPK_E_ARG, why);
  ICPK_HIP(ctx, hipSetDevice(ctx->device));
  Work w;
  if (int rc = reserve(ctx, n_nodes, n_edges, w)) return rc;
  w.a.ref = -1;  // (no node is left out of anything here)
  w.a.mu = mu;
  ICPK_HIP(ctx, hipMemsetAsync(ctx->pg_partial, 0, (size_t)PG_NPARTIAL * RED_MAX_BLOCKS * sizeof(double), ctx->stream));
  ICPK_HIP(ctx, hipMemcpyAsync(w.poses[0], poses, 16 * (size_t)n_nodes * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  if (int rc = upload_edges(ctx, w, edges, n_edges)) return rc;
  launch_pg_linearise(w.a, w.lin[0], true, ctx->stream);
  PgScalars s{};
  if (int rc = read_scalars(ctx, s)) return rc;
  const size_t m = (size_t)n_edges;
  if (chi2_out) ICPK_HIP(ctx, hipMemcpyAsync(chi2_out, w.lin[0].chi2, m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (weight_out) ICPK_HIP(ctx, hipMemcpyAsync(weight_out, w.lin[0].l, m * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  if (gradient_out)
    ICPK_HIP(ctx, hipMemcpyAsync(gradient_out, w.lin[0].g, 6 * (size_t)n_nodes * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  ICPK_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (cost_out) *cost_out = s.cost;
  return ICPK_OK;
}

int icpk_get_pose_graph_trace(icpk_ctx* ctx, int32_t* n_iter, double* cost_out, double* lambda_out,
                              int32_t* pcg_iterations_out, int32_t* accepted_out) {
  if (!ctx || !n_iter) return ICPK_E_ARG;
  const size_t n = ctx->pg_trace_cost.size();
  *n_iter = (int32_t)n;
  if (cost_out) std::memcpy(cost_out, ctx->pg_trace_cost.data(), n * sizeof(double));
  if (lambda_out) std::memcpy(lambda_out, ctx->pg_trace_lambda.data(), n * sizeof(double));
  if (pcg_iterations_out) std::memcpy(pcg_iterations_out, ctx->pg_trace_pcg.data(), n * sizeof(int32_t));
  if (accepted_out) std::memcpy(accepted_out, ctx->pg_trace_accepted.data(), n * sizeof(int32_t));
  return ICPK_OK;
}

}  // extern "C"
