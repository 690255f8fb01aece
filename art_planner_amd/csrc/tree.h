// tree.h -- the tree planners of the reference (art_planner/src/planner.cpp:92-105: OMPL's RRTstar, InformedRRTstar and
// RRTsharp) as ONE batch per stage on the device: artp_tree_* of include/artp_c.h.
//
// One tree per handle; vertex 0 is the start, vertices are n x 7 SE3 rows.  A batch of B samples runs, every stage a
// kernel (or the existing checkMotion pipeline) on the context's stream, two host reads of survivor counts per batch:
//   1. sample      B states of the (seed, index) stream; while the goal is not a vertex, slot 0 is the goal itself
//   2. nearest     exact nearest unpruned pre-batch vertex (tree_knn_kernel, k = 1); steer to range; d == 0 drops
//   3. informed    inf_rrt_star with a solution: h(s, x) + h(x, g) >= c_best drops the sample
//   4. first motion  checkMotion(nearest, x_new) for the survivors (artp_check_motions_dev)         -> host read 1, 2
//   5. near set    exact k nearest unpruned pre-batch vertices of x_new (k = RRTstar's k_rrt_), checkMotion for each
//   6. parent      argmin (cost(u) + c(u, x_new), u) over the valid candidates; new vertices in slot order
//   7. rewire      pre-batch j -> new v when cost(v) + c(v, j) < cost(j); integer atomics on the cost bits, then the id
//   8. cost-to-come  left fold from the root along every parent chain (tree_cost_fold_kernel)
//   9. rrt_sharp   instead of 7: exact shortest paths over every valid checked motion (the RRG), parent = predecessor
//  10. pruning     inf_rrt_star: h(s, v) + h(v, g) >= c_best marks v pruned (no longer a nearest / near candidate)
// Everything is a pure function of the parameters: no float atomics, ties broken by ids -- a tree is reproducible bit
// for bit.  DESIGN.md "Tree planners" has the semantics and where they differ from OMPL's sequential loop.
#pragma once

#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

namespace artp {

constexpr int TREE_KMAX = 64;              // near-set size limit: list entry i lives in lane i of the query's wave
constexpr uint32_t TREE_NONE = 0xffffffffu;
constexpr int TREE_MAX_BATCH = 65536;      // tree_compact_kernel: one workgroup, 64 flags per lane
constexpr int TREE_NSTAGES = 10;

__device__ __forceinline__ bool tree_less(double a, uint32_t ai, double b, uint32_t bi) {
  return a < b || (a == b && ai < bi);
}

// Exact k nearest (distance, id) of every query among the unpruned vertices [0, nv), OMPL's SE3 distance, ascending by
// (distance, id); missing entries are TREE_NONE / +inf.  One wave64 per query (4 per workgroup), the vertex rows staged
// through LDS in tiles of 256 shared by the four waves.  The wave's current list is held one entry per lane; a chunk
// of 64 vertices (one per lane) offers its candidates below the k-th entry, the smallest goes in by a shift across
// lanes, repeated while candidates remain (after the first tiles a chunk rarely has one).  The R^3 part of the distance
// is a lower bound: the arc length (an acos) is only formed when it does not already exceed the k-th distance.
__global__ void __launch_bounds__(256)
tree_knn_kernel(const double* __restrict__ verts, int nv, const uint8_t* __restrict__ pruned,
                const double* __restrict__ queries, int nq, int k, uint32_t* __restrict__ out_id,
                double* __restrict__ out_d) {
  __shared__ double tile[256 * 7];
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  const bool active = q < nq;
  double x[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) x[c] = active ? queries[(size_t)q * 7 + c] : 0.0;
  double ld = INFINITY, kd = INFINITY;
  uint32_t lid = TREE_NONE, kid = TREE_NONE;
  for (int base = 0; base < nv; base += 256) {
    const int cnt = min(256, nv - base);
    __syncthreads();
    for (int i = threadIdx.x; i < cnt * 7; i += 256) tile[i] = verts[(size_t)base * 7 + i];
    __syncthreads();
    if (!active) continue;
    for (int sub = 0; sub < cnt; sub += 64) {
      const int t = sub + lane;
      double d = INFINITY;
      uint32_t id = TREE_NONE;
      if (t < cnt && !(pruned && pruned[base + t])) {
        const double* v = &tile[t * 7];
        const double dx = x[0] - v[0], dy = x[1] - v[1], dz = x[2] - v[2];
        const double dp = sqrt(dx * dx + dy * dy + dz * dz);
        if (dp <= kd) {  // se3_distance, formed the same way (same bits)
          d = dp + so3_arc_length(x + 3, v + 3);
          id = (uint32_t)(base + t);
        }
      }
      bool cand = id != TREE_NONE && tree_less(d, id, kd, kid);
      while (__ballot(cand)) {
        double md = cand ? d : INFINITY;
        uint32_t mid = cand ? id : TREE_NONE;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const double od = __shfl_xor(md, off, 64);
          const uint32_t oi = (uint32_t)__shfl_xor((int)mid, off, 64);
          if (tree_less(od, oi, md, mid)) {
            md = od;
            mid = oi;
          }
        }
        const int pos = __popcll(__ballot(lane < k && tree_less(ld, lid, md, mid)));
        const double pd = __shfl_up(ld, 1, 64);
        const uint32_t pi = (uint32_t)__shfl_up((int)lid, 1, 64);
        if (lane == pos) {
          ld = md;
          lid = mid;
        } else if (lane > pos && lane < k) {
          ld = pd;
          lid = pi;
        }
        kd = __shfl(ld, k - 1, 64);
        kid = (uint32_t)__shfl((int)lid, k - 1, 64);
        if (id == mid) cand = false;
        cand = cand && tree_less(d, id, kd, kid);
      }
    }
  }
  if (active && lane < k) {
    out_id[(size_t)q * k + lane] = lid;
    if (out_d) out_d[(size_t)q * k + lane] = ld;
  }
}

// PathLengthObjective::motionCostHeuristic (path_length_objective.cpp:58-70): |dxyz| / max_lon_vel
__device__ __forceinline__ double tree_heuristic(double max_lon_vel, const double* a, const double* b) {
  const PathLengthParams h{0, max_lon_vel, 1.0, 1.0};
  return path_length_cost(h, a, b);
}

// Stages 2 (steer) and 3 (informed rejection).  c_best = cost[goal_id] (the previous batch's) when goal_id is a vertex.
__global__ void __launch_bounds__(256)
tree_steer_kernel(const double* __restrict__ verts, const double* __restrict__ samp, const uint32_t* __restrict__ nn,
                  const double* __restrict__ nd, int B, double range, int informed, const double* __restrict__ sg,
                  const double* __restrict__ cost, uint32_t goal_id, double max_lon_vel, double* __restrict__ xnew,
                  uint8_t* __restrict__ alive, uint32_t* __restrict__ exact0) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= B) return;
  const double d = nd[s];
  bool ok = nn[s] != TREE_NONE && d > 0.0;
  double x[7];
  const double* b = samp + (size_t)s * 7;
  if (ok && d > range) {
    se3_interpolate(verts + (size_t)nn[s] * 7, b, range / d, x);
  } else {
#pragma unroll
    for (int c = 0; c < 7; ++c) x[c] = b[c];
  }
  if (ok && informed && goal_id != TREE_NONE)
    ok = tree_heuristic(max_lon_vel, sg, x) + tree_heuristic(max_lon_vel, x, sg + 7) < cost[goal_id];
#pragma unroll
  for (int c = 0; c < 7; ++c) xnew[(size_t)s * 7 + c] = x[c];
  alive[s] = ok ? 1 : 0;
  if (s == 0) *exact0 = ok && !(d > range) ? 1u : 0u;  // slot 0's x_new IS its sample (the goal, when it holds the goal)
}

// Stream compaction of n <= TREE_MAX_BATCH flags in ONE workgroup (order kept): idx[j] = the j-th flagged position,
// rank[i] = flagged positions before i (may be NULL), out[0] = count, out[1] = remap[idx[0]] (or idx[0]; TREE_NONE when
// nothing is flagged).
__global__ void __launch_bounds__(1024)
tree_compact_kernel(const uint8_t* __restrict__ flag, int n, uint32_t* __restrict__ idx, uint32_t* __restrict__ rank,
                    const uint32_t* __restrict__ remap, uint32_t* __restrict__ out) {
  __shared__ uint32_t part[1024];
  const int t = threadIdx.x;
  const int per = (n + 1023) / 1024;
  const int i0 = min(n, t * per), i1 = min(n, i0 + per);
  uint32_t cnt = 0;
  for (int i = i0; i < i1; ++i) cnt += flag[i] ? 1u : 0u;
  part[t] = cnt;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {  // inclusive scan (Hillis-Steele)
    const uint32_t add = t >= off ? part[t - off] : 0u;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  uint32_t r = part[t] - cnt;
  for (int i = i0; i < i1; ++i) {
    if (rank) rank[i] = r;
    if (flag[i]) idx[r++] = (uint32_t)i;
  }
  __syncthreads();
  if (t == 0) {
    const uint32_t total = part[1023];
    out[0] = total;
    out[1] = total ? (remap ? remap[idx[0]] : idx[0]) : TREE_NONE;
  }
}

// First-motion end points: s1 = nearest vertex, s2 = x_new, for the m survivors of the steer stage
__global__ void __launch_bounds__(256)
tree_gather_first_kernel(const double* __restrict__ verts, const double* __restrict__ xnew, const uint32_t* __restrict__ nn,
                         const uint32_t* __restrict__ idx1, int m, double* __restrict__ s1, double* __restrict__ s2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint32_t s = idx1[i];
#pragma unroll
  for (int c = 0; c < 7; ++c) {
    s1[(size_t)i * 7 + c] = verts[(size_t)nn[s] * 7 + c];
    s2[(size_t)i * 7 + c] = xnew[(size_t)s * 7 + c];
  }
}

// Log of the first motions (vertex id of x_new or TREE_NONE) and the survivors' rows for the near stage:
// xs[j] / par0[j] / c0[j] = x_new / nearest / c(nearest, x_new) of the j-th new vertex (id n_pre + j, j < m_keep).
__global__ void __launch_bounds__(256)
tree_first_log_kernel(PathLengthParams pl, const double* __restrict__ verts, const double* __restrict__ xnew,
                      const uint32_t* __restrict__ nn, const uint32_t* __restrict__ idx1, const uint8_t* __restrict__ valid1,
                      const uint32_t* __restrict__ rank2, int m1, uint32_t m_keep, uint32_t n_pre, uint32_t batch,
                      double* __restrict__ xs, uint32_t* __restrict__ par0, double* __restrict__ c0, uint32_t* __restrict__ lu,
                      uint32_t* __restrict__ lv, uint8_t* __restrict__ lvalid, uint32_t* __restrict__ lbatch,
                      double* __restrict__ lcuv, double* __restrict__ lcvu) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m1) return;
  const uint32_t s = idx1[i], u = nn[s];
  const double* a = verts + (size_t)u * 7;
  const double* x = xnew + (size_t)s * 7;
  const bool keep = valid1[i] && rank2[i] < m_keep;
  lu[i] = u;
  lv[i] = keep ? n_pre + rank2[i] : TREE_NONE;
  lvalid[i] = valid1[i] ? 1 : 0;
  lbatch[i] = batch;
  const double w = path_length_cost(pl, a, x);
  lcuv[i] = w;
  lcvu[i] = path_length_cost(pl, x, a);
  if (keep) {
    const uint32_t j = rank2[i];
    c0[j] = w;
#pragma unroll
    for (int c = 0; c < 7; ++c) xs[(size_t)j * 7 + c] = x[c];
    par0[j] = u;
  }
}

// Near motions: (u, x_new) for every near entry that is a vertex other than the nearest (whose verdict is known);
// the other slots get the zero-length motion (x_new, x_new) and are not logged as motions.
__global__ void __launch_bounds__(256)
tree_near_pairs_kernel(const double* __restrict__ verts, const double* __restrict__ xs, const uint32_t* __restrict__ par0,
                       const uint32_t* __restrict__ near_id, int m2, int k, double* __restrict__ s1,
                       double* __restrict__ s2) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)m2 * k) return;
  const size_t j = e / k;
  const uint32_t u = near_id[e];
  const bool real = u != TREE_NONE && u != par0[j];
  const double* a = real ? verts + (size_t)u * 7 : xs + j * 7;
#pragma unroll
  for (int c = 0; c < 7; ++c) {
    s1[e * 7 + c] = a[c];
    s2[e * 7 + c] = xs[j * 7 + c];
  }
}

// Stage 6: parent of new vertex n_pre + j = argmin (cost(u) + c(u, x), u) over the nearest and the valid near motions
// (pre-batch costs); the near motions go to the log (valid = 0xff: no motion in that slot).
__global__ void __launch_bounds__(256)
tree_parent_kernel(PathLengthParams pl, double* __restrict__ verts, double* __restrict__ cost, uint32_t* __restrict__ parent,
                   double* __restrict__ ecost, uint32_t* __restrict__ born, uint8_t* __restrict__ pruned,
                   const double* __restrict__ xs, const uint32_t* __restrict__ par0, const double* __restrict__ c0,
                   const uint32_t* __restrict__ near_id, const uint8_t* __restrict__ near_valid, int m2, int k,
                   uint32_t n_pre, uint32_t batch, uint32_t* __restrict__ lu, uint32_t* __restrict__ lv,
                   uint8_t* __restrict__ lvalid, uint32_t* __restrict__ lbatch, double* __restrict__ lcuv,
                   double* __restrict__ lcvu, unsigned long long* __restrict__ n_checked) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m2) return;
  double x[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) x[c] = xs[(size_t)j * 7 + c];
  const uint32_t v = n_pre + (uint32_t)j;
  uint32_t best_u = par0[j];
  double best_w = c0[j];
  double best = cost[best_u] + best_w;
  unsigned real_n = 0;
  for (int q = 0; q < k; ++q) {
    const size_t e = (size_t)j * k + q;
    const uint32_t u = near_id[e];
    const bool real = u != TREE_NONE && u != par0[j];
    lu[e] = u;
    lv[e] = v;
    lbatch[e] = batch;
    if (!real) {
      lvalid[e] = 0xff;
      lcuv[e] = lcvu[e] = 0.0;
      continue;
    }
    ++real_n;
    const double* a = verts + (size_t)u * 7;
    const double w = path_length_cost(pl, a, x);
    lvalid[e] = near_valid[e] ? 1 : 0;
    lcuv[e] = w;
    lcvu[e] = path_length_cost(pl, x, a);
    if (!near_valid[e]) continue;
    const double cand = cost[u] + w;
    if (tree_less(cand, u, best, best_u)) {
      best = cand;
      best_u = u;
      best_w = w;
    }
  }
#pragma unroll
  for (int c = 0; c < 7; ++c) verts[(size_t)v * 7 + c] = x[c];
  parent[v] = best_u;
  ecost[v] = best_w;
  cost[v] = best;
  born[v] = batch;
  pruned[v] = 0;
  if (real_n) atomicAdd(n_checked, (unsigned long long)real_n);
}

// Stage 7, rewiring, over the batch's logged motions (u pre-batch, v new, valid): cand = cost(v) + c(v, u) with the
// costs of stage 6.  Phase 0: smallest candidate bits per u (non-negative doubles order like their bit patterns),
// phase 1: smallest v among the candidates with those bits, phase 2: the winner becomes u's parent.
__global__ void __launch_bounds__(256)
tree_rewire_kernel(int phase, const uint32_t* __restrict__ lu, const uint32_t* __restrict__ lv,
                   const uint8_t* __restrict__ lvalid, const double* __restrict__ lcvu, size_t ne, uint32_t n_pre,
                   const double* __restrict__ cost, unsigned long long* __restrict__ best_bits,
                   uint32_t* __restrict__ best_id, uint32_t* __restrict__ parent, double* __restrict__ ecost,
                   unsigned long long* __restrict__ n_rewired) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ne || lvalid[e] != 1) return;
  const uint32_t u = lu[e], v = lv[e];
  if (v == TREE_NONE || v < n_pre || u >= n_pre) return;
  const double cand = cost[v] + lcvu[e];
  if (!(cand < cost[u])) return;
  const unsigned long long bits = (unsigned long long)__double_as_longlong(cand);
  if (phase == 0) {
    atomicMin(&best_bits[u], bits);
  } else if (phase == 1) {
    if (bits == best_bits[u]) atomicMin(&best_id[u], v);
  } else if (bits == best_bits[u] && v == best_id[u]) {
    parent[u] = v;
    ecost[u] = lcvu[e];
    atomicAdd(n_rewired, 1ull);
  }
}

// Stage 8: cost(v) = the left fold ((0 + w1) + w2) + ... of the edge costs from the root down to v.  One lane per vertex
// walks its parent chain: once for the depth D, then in chunks of 32 edges from the root side (a chunk's edges are
// collected walking up from its deepest vertex and folded in root order).  A chain longer than the vertex count is a
// cycle: *err = 1 (the tests' debug assert; a correct tree never sets it).
__global__ void __launch_bounds__(256)
tree_cost_fold_kernel(const uint32_t* __restrict__ parent, const double* __restrict__ ecost, uint32_t n,
                      double* __restrict__ cost, int* __restrict__ err) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  uint32_t D = 0;
  for (uint32_t u = v; u != 0; u = parent[u]) {
    if (u >= n || ++D > n) {
      *err = 1;
      return;
    }
  }
  double acc = 0.0, buf[32];
  uint32_t done = 0;
  while (done < D) {
    const uint32_t chunk = min(32u, D - done);
    uint32_t u = v;
    for (uint32_t s = 0; s < D - done - chunk; ++s) u = parent[u];
    for (uint32_t i = chunk; i-- > 0;) {  // buf[i] = the edge at root position done + i
      buf[i] = ecost[u];
      u = parent[u];
    }
    for (uint32_t i = 0; i < chunk; ++i) acc = acc + buf[i];
    done += chunk;
  }
  cost[v] = acc;
}

// Stage 9 (rrt_sharp): label-correcting shortest paths from the root over every valid logged motion, both directions
// with their directed costs, in ONE workgroup until a sweep changes nothing (no host round trip).  dist starts from the
// current costs (each is the cost of a path in the graph; the graph only grows), so it converges to the exact least fixed
// point: dist[v] = min over paths of the left-fold sum, the same whatever the order of the relaxations.
__global__ void __launch_bounds__(1024)
tree_sssp_kernel(const uint32_t* __restrict__ lu, const uint32_t* __restrict__ lv, const uint8_t* __restrict__ lvalid,
                 const double* __restrict__ lcuv, const double* __restrict__ lcvu, size_t ne,
                 unsigned long long* __restrict__ dist, uint32_t max_sweeps, int* __restrict__ err) {
  __shared__ int changed;
  for (uint32_t sweep = 0;; ++sweep) {
    if (threadIdx.x == 0) changed = 0;
    __syncthreads();
    int local = 0;
    for (size_t e = threadIdx.x; e < ne; e += 1024) {
      if (lvalid[e] != 1 || lv[e] == TREE_NONE) continue;
      const uint32_t u = lu[e], v = lv[e];
      const double du = __longlong_as_double((long long)__hip_atomic_load(&dist[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      const double dv = __longlong_as_double((long long)__hip_atomic_load(&dist[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      if (du + lcuv[e] < dv) {
        const unsigned long long nd = (unsigned long long)__double_as_longlong(du + lcuv[e]);
        if (atomicMin(&dist[v], nd) > nd) local = 1;
      }
      if (dv + lcvu[e] < du) {
        const unsigned long long nd = (unsigned long long)__double_as_longlong(dv + lcvu[e]);
        if (atomicMin(&dist[u], nd) > nd) local = 1;
      }
    }
    if (local) atomicOr(&changed, 1);
    __syncthreads();
    const int again = changed;
    __syncthreads();
    if (!again) return;
    if (sweep >= max_sweeps) {
      if (threadIdx.x == 0) *err = 2;
      return;
    }
  }
}

// A tight motion u -> v at the fixed point: dist[u] + w == dist[v] bit for bit
__device__ __forceinline__ bool tree_tight(const unsigned long long* dist, uint32_t u, uint32_t v, double w) {
  const double du = __longlong_as_double((long long)dist[u]), dv = __longlong_as_double((long long)dist[v]);
  return v != 0 && du < INFINITY && du + w == dv;
}

// hops[v] = the fewest tight motions from the root to v (one workgroup, sweeps until nothing changes).  Motions of cost 0
// exist (the sampler repeats cell positions: states that differ in yaw only), so "tight" alone admits cycles of equal
// dist; a predecessor one hop closer to the root cannot close one.
__global__ void __launch_bounds__(1024)
tree_hops_kernel(const uint32_t* __restrict__ lu, const uint32_t* __restrict__ lv, const uint8_t* __restrict__ lvalid,
                 const double* __restrict__ lcuv, const double* __restrict__ lcvu, size_t ne,
                 const unsigned long long* __restrict__ dist, uint32_t* __restrict__ hops, uint32_t max_sweeps,
                 int* __restrict__ err) {
  __shared__ int changed;
  for (uint32_t sweep = 0;; ++sweep) {
    if (threadIdx.x == 0) changed = 0;
    __syncthreads();
    int local = 0;
    for (size_t e = threadIdx.x; e < ne; e += 1024) {
      if (lvalid[e] != 1 || lv[e] == TREE_NONE) continue;
      const uint32_t u = lu[e], v = lv[e];
      const uint32_t hu = __hip_atomic_load(&hops[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const uint32_t hv = __hip_atomic_load(&hops[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (hu != TREE_NONE && hu + 1 < hv && tree_tight(dist, u, v, lcuv[e]) && atomicMin(&hops[v], hu + 1) > hu + 1)
        local = 1;
      if (hv != TREE_NONE && hv + 1 < hu && tree_tight(dist, v, u, lcvu[e]) && atomicMin(&hops[u], hv + 1) > hv + 1)
        local = 1;
    }
    if (local) atomicOr(&changed, 1);
    __syncthreads();
    const int again = changed;
    __syncthreads();
    if (!again) return;
    if (sweep >= max_sweeps) {
      if (threadIdx.x == 0) *err = 2;
      return;
    }
  }
}

// pred[v] = the smallest u with a tight valid motion u -> v and hops[u] + 1 == hops[v] (phase 0); its cost becomes the
// edge cost (phase 1)
__global__ void __launch_bounds__(256)
tree_pred_kernel(int phase, const uint32_t* __restrict__ lu, const uint32_t* __restrict__ lv,
                 const uint8_t* __restrict__ lvalid, const double* __restrict__ lcuv, const double* __restrict__ lcvu,
                 size_t ne, const unsigned long long* __restrict__ dist, const uint32_t* __restrict__ hops,
                 uint32_t* __restrict__ pred, double* __restrict__ pred_w) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ne || lvalid[e] != 1 || lv[e] == TREE_NONE) return;
  const uint32_t u = lu[e], v = lv[e];
  if (hops[u] != TREE_NONE && hops[u] + 1 == hops[v] && tree_tight(dist, u, v, lcuv[e])) {
    if (phase == 0) atomicMin(&pred[v], u);
    else if (pred[v] == u) pred_w[v] = lcuv[e];
  }
  if (hops[v] != TREE_NONE && hops[v] + 1 == hops[u] && tree_tight(dist, v, u, lcvu[e])) {
    if (phase == 0) atomicMin(&pred[u], v);
    else if (pred[u] == v) pred_w[u] = lcvu[e];
  }
}

// The predecessors become the parents (every vertex but the root has one: it is reached by its tree edge)
__global__ void __launch_bounds__(256)
tree_apply_pred_kernel(const uint32_t* __restrict__ pred, const double* __restrict__ pred_w, uint32_t n, uint32_t n_pre,
                       uint32_t* __restrict__ parent, double* __restrict__ ecost, unsigned long long* __restrict__ n_rewired) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v == 0 || v >= n || pred[v] == TREE_NONE) return;
  if (v < n_pre && parent[v] != pred[v]) atomicAdd(n_rewired, 1ull);
  parent[v] = pred[v];
  ecost[v] = pred_w[v];
}

// Stage 10 (inf_rrt_star): h(s, v) + h(v, g) >= c_best prunes v (never the root or the goal vertex)
__global__ void __launch_bounds__(256)
tree_prune_kernel(const double* __restrict__ verts, uint32_t n, const double* __restrict__ sg, const double* __restrict__ cost,
                  uint32_t goal_id, double max_lon_vel, uint8_t* __restrict__ pruned) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v == 0 || v >= n || v == goal_id || pruned[v]) return;
  const double* x = verts + (size_t)v * 7;
  if (tree_heuristic(max_lon_vel, sg, x) + tree_heuristic(max_lon_vel, x, sg + 7) >= cost[goal_id]) pruned[v] = 1;
}

}  // namespace artp

struct artp_tree {
  artp_ctx* ctx = nullptr;
  artp_tree_params params{};
  double sg[14];                 // start, goal
  double range = 0.0;
  int kmax = 1;                  // near-set size at max_vertices
  uint32_t cap = 0, n = 1;       // vertex capacity, vertices
  uint64_t batches = 0;
  uint32_t goal_id = artp::TREE_NONE;
  uint64_t first_solution_batch = ~0ull;
  // the tree (cap rows)
  double *d_verts = nullptr, *d_cost = nullptr, *d_ecost = nullptr;
  uint32_t *d_parent = nullptr, *d_born = nullptr;
  uint8_t* d_pruned = nullptr;
  double* d_sg = nullptr;
  // per-batch scratch (B rows, B x kmax near slots)
  double *d_samp = nullptr, *d_xnew = nullptr, *d_nd = nullptr, *d_xs = nullptr, *d_c0 = nullptr;
  double *d_s1 = nullptr, *d_s2 = nullptr;
  uint32_t *d_nn = nullptr, *d_idx1 = nullptr, *d_idx2 = nullptr, *d_rank = nullptr, *d_par0 = nullptr, *d_near = nullptr;
  uint8_t *d_alive = nullptr, *d_valid1 = nullptr, *d_validk = nullptr;
  uint32_t* d_cnt = nullptr;     // 4 words: compaction results
  PinnedBuffer<uint32_t> h_cnt;  // pinned twin
  unsigned long long* d_counters = nullptr;  // [0] near motions checked, [1] rewires
  int* d_err = nullptr;
  unsigned long long* d_best_bits = nullptr;  // rewire: cap; rrt_sharp: dist
  uint32_t* d_best_id = nullptr;              // rewire: cap; rrt_sharp: pred
  double* d_pred_w = nullptr;
  uint32_t* d_hops = nullptr;                 // rrt_sharp
  // every motion checked since creation (valid 0xff = an unused near slot, skipped by the exports)
  uint32_t *d_lu = nullptr, *d_lv = nullptr, *d_lbatch = nullptr;
  uint8_t* d_lvalid = nullptr;
  double *d_lcuv = nullptr, *d_lcvu = nullptr;
  size_t log_n = 0, log_cap = 0;
  uint64_t first_checked = 0;    // first motions checked (host count; the near ones are counted on the device)
  double stage_us[artp::TREE_NSTAGES] = {};
  hipEvent_t ev[artp::TREE_NSTAGES + 1] = {};
  DeviceScratch mem;             // owns every d_ pointer above
};

namespace {

// RRTstar's k_rrt_ rule (OMPL RRTstar::calculateRewiringLowerBounds): ceil(rewire_factor (e + e / dim) ln (n + 1)), dim 6
inline int tree_k(double rewire_factor, size_t n) {
  return (int)std::ceil(rewire_factor * (2.718281828459045 + 2.718281828459045 / 6.0) * std::log((double)n + 1.0));
}

// what the tree's members do not own themselves: the events
void tree_free(artp_tree* t) {
  for (hipEvent_t& e : t->ev)
    if (e) (void)hipEventDestroy(e);
}

// make room for `need` log entries (doubling; the old entries are copied)
int tree_log_reserve(artp_tree* t, size_t need) {
  artp_ctx* c = t->ctx;
  if (need <= t->log_cap) return ARTP_OK;
  size_t cap = t->log_cap ? t->log_cap : (1u << 16);
  while (cap < need) cap *= 2;
  uint32_t *lu = nullptr, *lv = nullptr, *lb = nullptr;
  uint8_t* lval = nullptr;
  double *cuv = nullptr, *cvu = nullptr;
  DeviceScratch S;  // the new six until the copy is through
  HIP_TRY(c, S.alloc(&lu, cap));
  HIP_TRY(c, S.alloc(&lv, cap));
  HIP_TRY(c, S.alloc(&lb, cap));
  HIP_TRY(c, S.alloc(&lval, cap));
  HIP_TRY(c, S.alloc(&cuv, cap));
  HIP_TRY(c, S.alloc(&cvu, cap));
  if (t->log_n) {
    const size_t m = t->log_n;
    HIP_TRY(c, hipMemcpyAsync(lu, t->d_lu, m * 4, hipMemcpyDeviceToDevice, c->lane->stream));
    HIP_TRY(c, hipMemcpyAsync(lv, t->d_lv, m * 4, hipMemcpyDeviceToDevice, c->lane->stream));
    HIP_TRY(c, hipMemcpyAsync(lb, t->d_lbatch, m * 4, hipMemcpyDeviceToDevice, c->lane->stream));
    HIP_TRY(c, hipMemcpyAsync(lval, t->d_lvalid, m, hipMemcpyDeviceToDevice, c->lane->stream));
    HIP_TRY(c, hipMemcpyAsync(cuv, t->d_lcuv, m * 8, hipMemcpyDeviceToDevice, c->lane->stream));
    HIP_TRY(c, hipMemcpyAsync(cvu, t->d_lcvu, m * 8, hipMemcpyDeviceToDevice, c->lane->stream));
    HIP_TRY(c, hipStreamSynchronize(c->lane->stream));
  }
  for (void* p : {(void*)t->d_lu, (void*)t->d_lv, (void*)t->d_lbatch, (void*)t->d_lvalid, (void*)t->d_lcuv, (void*)t->d_lcvu})
    t->mem.release(p);
  t->d_lu = t->mem.adopt(S.take(lu));
  t->d_lv = t->mem.adopt(S.take(lv));
  t->d_lbatch = t->mem.adopt(S.take(lb));
  t->d_lvalid = t->mem.adopt(S.take(lval));
  t->d_lcuv = t->mem.adopt(S.take(cuv));
  t->d_lcvu = t->mem.adopt(S.take(cvu));
  t->log_cap = cap;
  return ARTP_OK;
}

// blocks of bs threads over n items, at least one (also what roadmap_many.h launches with)
inline unsigned tree_blocks(size_t n, unsigned bs = 256) { return (unsigned)std::max<size_t>((n + bs - 1) / bs, 1); }

// One batch (stages 1-10).  *stop = true when the tree cannot take another vertex.
int tree_batch(artp_tree* t, bool* stop) {
  using namespace artp;
  artp_ctx* c = t->ctx;
  hipStream_t st = c->lane->stream;
  const artp_tree_params& p = t->params;
  const int B = (int)p.batch;
  const uint32_t n_pre = t->n;
  const uint32_t batch = (uint32_t)t->batches;
  const PathLengthParams pl{p.objective == 1, p.max_lon_vel, p.max_lat_vel, p.max_ang_vel};
  const bool prof = p.profile != 0;
  auto mark = [&](int i) -> int {
    if (prof) HIP_TRY(c, hipEventRecord(t->ev[i], st));
    return ARTP_OK;
  };
  // 1. sample (slot i = stream index first_index + batch * B + i); the goal takes slot 0 while it is not a vertex
  //    (with B == 1: every 20th batch, OMPL's 5 % goal bias)
  ARTP_TRY(mark(0));
  ARTP_TRY(artp_sample_states_dev(c, p.seed, p.first_index + (uint64_t)batch * B, (size_t)B, t->d_samp));
  const bool goal_slot = t->goal_id == TREE_NONE && (B > 1 || batch % 20 == 0);
  if (goal_slot)
    HIP_TRY(c, hipMemcpyAsync(t->d_samp, t->d_sg + 7, 7 * sizeof(double), hipMemcpyDeviceToDevice, st));
  // 2. nearest unpruned pre-batch vertex
  ARTP_TRY(mark(1));
  hipLaunchKernelGGL(tree_knn_kernel, dim3(tree_blocks(B, 4)), dim3(256), 0, st, t->d_verts, (int)n_pre,
                     (const uint8_t*)t->d_pruned, (const double*)t->d_samp, B, 1, t->d_nn, t->d_nd);
  // 2b / 3. steer, informed rejection, compaction of the survivors (host read 1)
  ARTP_TRY(mark(2));
  hipLaunchKernelGGL(tree_steer_kernel, dim3(tree_blocks(B)), dim3(256), 0, st, (const double*)t->d_verts,
                     (const double*)t->d_samp, (const uint32_t*)t->d_nn, (const double*)t->d_nd, B, t->range,
                     p.variant == 1 ? 1 : 0, (const double*)t->d_sg, (const double*)t->d_cost, t->goal_id, p.max_lon_vel,
                     t->d_xnew, t->d_alive, t->d_cnt + 2);
  hipLaunchKernelGGL(tree_compact_kernel, dim3(1), dim3(1024), 0, st, (const uint8_t*)t->d_alive, B, t->d_idx1,
                     (uint32_t*)nullptr, (const uint32_t*)nullptr, t->d_cnt);
  HIP_TRY(c, hipMemcpyAsync(t->h_cnt.host(), t->d_cnt, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  const int m1 = (int)t->h_cnt.host()[0];
  // 4. first motion checkMotion(nearest, x_new) (host read 2: survivors, and whether slot 0 -- the goal -- is one)
  ARTP_TRY(mark(3));
  int m2 = 0;
  uint32_t first_slot = TREE_NONE;
  if (m1) {
    hipLaunchKernelGGL(tree_gather_first_kernel, dim3(tree_blocks(m1)), dim3(256), 0, st, (const double*)t->d_verts,
                       (const double*)t->d_xnew, (const uint32_t*)t->d_nn, (const uint32_t*)t->d_idx1, m1, t->d_s1, t->d_s2);
    ARTP_TRY(artp_check_motions_dev(c, t->d_s1, t->d_s2, (size_t)m1, t->d_valid1));
    hipLaunchKernelGGL(tree_compact_kernel, dim3(1), dim3(1024), 0, st, (const uint8_t*)t->d_valid1, m1, t->d_idx2,
                       t->d_rank, (const uint32_t*)t->d_idx1, t->d_cnt);
    HIP_TRY(c, hipMemcpyAsync(t->h_cnt.host(), t->d_cnt, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    m2 = (int)std::min<uint32_t>(t->h_cnt.host()[0], t->cap - n_pre);
    first_slot = t->h_cnt.host()[2] ? t->h_cnt.host()[1] : TREE_NONE;  // a goal steered short of the goal is not the goal
  }
  t->first_checked += (uint64_t)m1;
  const int k = std::max(1, std::min(tree_k(p.rewire_factor, n_pre), t->kmax));
  const size_t log0 = t->log_n, n_log = (size_t)m1 + (size_t)m2 * k;
  ARTP_TRY(tree_log_reserve(t, log0 + n_log));
  if (m1)
    hipLaunchKernelGGL(tree_first_log_kernel, dim3(tree_blocks(m1)), dim3(256), 0, st, pl, (const double*)t->d_verts,
                       (const double*)t->d_xnew, (const uint32_t*)t->d_nn, (const uint32_t*)t->d_idx1,
                       (const uint8_t*)t->d_valid1, (const uint32_t*)t->d_rank, m1, (uint32_t)m2, n_pre, batch, t->d_xs,
                       t->d_par0, t->d_c0, t->d_lu + log0, t->d_lv + log0, t->d_lvalid + log0, t->d_lbatch + log0,
                       t->d_lcuv + log0, t->d_lcvu + log0);
  if (m2) {
    // 5. near set of every survivor and its motions
    ARTP_TRY(mark(4));
    hipLaunchKernelGGL(tree_knn_kernel, dim3(tree_blocks(m2, 4)), dim3(256), 0, st, t->d_verts, (int)n_pre,
                       (const uint8_t*)t->d_pruned, (const double*)t->d_xs, m2, k, t->d_near, (double*)nullptr);
    ARTP_TRY(mark(5));
    hipLaunchKernelGGL(tree_near_pairs_kernel, dim3(tree_blocks((size_t)m2 * k)), dim3(256), 0, st,
                       (const double*)t->d_verts, (const double*)t->d_xs, (const uint32_t*)t->d_par0,
                       (const uint32_t*)t->d_near, m2, k, t->d_s1, t->d_s2);
    ARTP_TRY(artp_check_motions_dev(c, t->d_s1, t->d_s2, (size_t)m2 * k, t->d_validk));
    // 6. parent choice, new vertices n_pre .. n_pre + m2 - 1
    ARTP_TRY(mark(6));
    const size_t ln = log0 + (size_t)m1;
    hipLaunchKernelGGL(tree_parent_kernel, dim3(tree_blocks(m2)), dim3(256), 0, st, pl, t->d_verts, t->d_cost,
                       t->d_parent, t->d_ecost, t->d_born, t->d_pruned, (const double*)t->d_xs,
                       (const uint32_t*)t->d_par0, (const double*)t->d_c0, (const uint32_t*)t->d_near,
                       (const uint8_t*)t->d_validk, m2, k, n_pre, batch, t->d_lu + ln, t->d_lv + ln,
                       t->d_lvalid + ln, t->d_lbatch + ln, t->d_lcuv + ln, t->d_lcvu + ln, t->d_counters);
  } else {
    for (int i = 4; i < 7; ++i) ARTP_TRY(mark(i));
  }
  t->log_n = log0 + n_log;
  const uint32_t n_now = n_pre + (uint32_t)m2;
  // 7. rewiring (rrt_star, inf_rrt_star) over this batch's motions
  ARTP_TRY(mark(7));
  if (p.variant != 2 && m2) {
    HIP_TRY(c, hipMemsetAsync(t->d_best_bits, 0xff, (size_t)n_pre * 8, st));
    HIP_TRY(c, hipMemsetAsync(t->d_best_id, 0xff, (size_t)n_pre * 4, st));
    for (int phase = 0; phase < 3; ++phase)
      hipLaunchKernelGGL(tree_rewire_kernel, dim3(tree_blocks(n_log)), dim3(256), 0, st, phase,
                         (const uint32_t*)t->d_lu + log0, (const uint32_t*)t->d_lv + log0,
                         (const uint8_t*)t->d_lvalid + log0, (const double*)t->d_lcvu + log0, n_log, n_pre,
                         (const double*)t->d_cost, t->d_best_bits, t->d_best_id, t->d_parent, t->d_ecost,
                         t->d_counters + 1);
  }
  // 9. rrt_sharp: shortest paths over the whole graph of valid checked motions
  ARTP_TRY(mark(8));
  if (p.variant == 2 && m2) {
    HIP_TRY(c, hipMemcpyAsync(t->d_best_bits, t->d_cost, (size_t)n_now * 8, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(tree_sssp_kernel, dim3(1), dim3(1024), 0, st, (const uint32_t*)t->d_lu, (const uint32_t*)t->d_lv,
                       (const uint8_t*)t->d_lvalid, (const double*)t->d_lcuv, (const double*)t->d_lcvu, t->log_n,
                       t->d_best_bits, n_now + 2u, t->d_err);
    HIP_TRY(c, hipMemsetAsync(t->d_best_id, 0xff, (size_t)n_now * 4, st));
    HIP_TRY(c, hipMemsetAsync(t->d_hops, 0xff, (size_t)n_now * 4, st));
    HIP_TRY(c, hipMemsetAsync(t->d_hops, 0, 4, st));
    hipLaunchKernelGGL(tree_hops_kernel, dim3(1), dim3(1024), 0, st, (const uint32_t*)t->d_lu, (const uint32_t*)t->d_lv,
                       (const uint8_t*)t->d_lvalid, (const double*)t->d_lcuv, (const double*)t->d_lcvu, t->log_n,
                       (const unsigned long long*)t->d_best_bits, t->d_hops, n_now + 2u, t->d_err);
    for (int phase = 0; phase < 2; ++phase)
      hipLaunchKernelGGL(tree_pred_kernel, dim3(tree_blocks(t->log_n)), dim3(256), 0, st, phase,
                         (const uint32_t*)t->d_lu, (const uint32_t*)t->d_lv, (const uint8_t*)t->d_lvalid,
                         (const double*)t->d_lcuv, (const double*)t->d_lcvu, t->log_n,
                         (const unsigned long long*)t->d_best_bits, (const uint32_t*)t->d_hops, t->d_best_id,
                         t->d_pred_w);
    hipLaunchKernelGGL(tree_apply_pred_kernel, dim3(tree_blocks(n_now)), dim3(256), 0, st, (const uint32_t*)t->d_best_id,
                       (const double*)t->d_pred_w, n_now, n_pre, t->d_parent, t->d_ecost, t->d_counters + 1);
  }
  // 8. cost-to-come: the left fold along every parent chain
  ARTP_TRY(mark(9));
  if (m2)
    hipLaunchKernelGGL(tree_cost_fold_kernel, dim3(tree_blocks(n_now)), dim3(256), 0, st, (const uint32_t*)t->d_parent,
                       (const double*)t->d_ecost, n_now, t->d_cost, t->d_err);
  HIP_TRY(c, hipGetLastError());
  t->n = n_now;
  ++t->batches;
  if (goal_slot && first_slot == 0 && m2 > 0) {
    t->goal_id = n_pre;  // slot 0 survived: the goal is the batch's first new vertex
    t->first_solution_batch = batch;
  }
  // 10. pruning by the (possibly lower) c_best
  if (p.variant == 1 && t->goal_id != TREE_NONE)
    hipLaunchKernelGGL(tree_prune_kernel, dim3(tree_blocks(n_now)), dim3(256), 0, st, (const double*)t->d_verts, n_now,
                       (const double*)t->d_sg, (const double*)t->d_cost, t->goal_id, p.max_lon_vel, t->d_pruned);
  ARTP_TRY(mark(TREE_NSTAGES));
  if (prof) {
    HIP_TRY(c, hipEventSynchronize(t->ev[TREE_NSTAGES]));
    for (int i = 0; i < TREE_NSTAGES; ++i) {
      float ms = 0.0f;
      HIP_TRY(c, hipEventElapsedTime(&ms, t->ev[i], t->ev[i + 1]));
      t->stage_us[i] += 1000.0 * ms;
    }
  }
  *stop = t->n >= t->cap;
  return ARTP_OK;
}

int tree_check_err(artp_tree* t) {
  artp_ctx* c = t->ctx;
  int err = 0;
  HIP_TRY(c, hipMemcpyAsync(&err, t->d_err, sizeof(int), hipMemcpyDeviceToHost, c->lane->stream));
  HIP_TRY(c, hipStreamSynchronize(c->lane->stream));
  if (err) {
    c->last_error = err == 1 ? "tree: a parent chain does not reach the root" : "tree: shortest-path sweeps did not settle";
    return ARTP_ERR_INVALID_ARG;
  }
  return ARTP_OK;
}

}  // namespace

extern "C" {

void artp_tree_params_defaults(artp_tree_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->seed = 42;
  p->first_index = 0;
  p->variant = 0;            // rrt_star
  p->objective = 0;          // PathLengthObjective, use_directional_cost{false} (params.h:70)
  p->max_lon_vel = 0.5;      // params.h:71-73
  p->max_lat_vel = 0.1;
  p->max_ang_vel = 0.5;
  p->batch = 1024;
  p->max_vertices = 100000;
  p->max_batches = 0;        // no limit
  p->plan_time = 0.0;        // no time budget
  p->range = 0.0;            // OMPL's 0.2 x maxExtent
  p->rewire_factor = 1.1;    // RRTstar's rewireFactor_
  p->profile = 0;
}

void artp_tree_destroy(artp_tree* t) {
  if (!t) return;
  tree_free(t);
  delete t;
}

int artp_tree_create(artp_ctx* c, const artp_tree_params* prm, const double* start7, const double* goal7, artp_tree** out) {
  if (!c || !prm || !start7 || !goal7 || !out) return ARTP_ERR_INVALID_ARG;
  *out = nullptr;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  if (prm->variant < 0 || prm->variant > 2 || prm->objective < 0 || prm->objective > 1 || prm->batch < 1 ||
      prm->batch > (uint32_t)artp::TREE_MAX_BATCH || prm->max_vertices < 2 || !(prm->max_lon_vel > 0.0) ||
      !(prm->max_lat_vel > 0.0) || !(prm->max_ang_vel > 0.0) || !(prm->range >= 0.0) || !(prm->plan_time >= 0.0) ||
      !(prm->rewire_factor > 0.0) || tree_k(prm->rewire_factor, prm->max_vertices) > artp::TREE_KMAX) {
    c->last_error = prm->objective == 2 ? "tree planners take objectives 0 and 1 only (PathLengthObjective)"
                                        : "tree parameters out of range";
    return ARTP_ERR_INVALID_ARG;
  }
  if (!c->have_field[0] || !c->have_field[1] || !c->have_sampler || !c->have_z) return ARTP_ERR_NO_MAP;
  std::unique_ptr<artp_tree, void (*)(artp_tree*)> owner(new artp_tree(), artp_tree_destroy);
  artp_tree* t = owner.get();
  t->ctx = c;
  t->params = *prm;
  std::memcpy(t->sg, start7, 7 * sizeof(double));
  std::memcpy(t->sg + 7, goal7, 7 * sizeof(double));
  HIP_TRY(c, hipSetDevice(c->device));
  {  // start and goal must be valid states (OMPL: INVALID_START / INVALID_GOAL)
    uint8_t ok[2] = {0, 0};
    ARTP_TRY(artp_validate_states(c, t->sg, 2, ok, nullptr));
    if (!ok[0] || !ok[1]) {
      c->last_error = !ok[0] ? "start state is not valid" : "goal state is not valid";
      return ARTP_ERR_INVALID_ARG;
    }
  }
  // OMPL's default range: 0.2 x the space's maximum extent -- |hi - lo| of the R^3 bounds (planner.cpp:146-156: map centre
  // -+ the full length, the context's z bounds; or the fixed extent of artp_set_r3_extent) plus SO3's pi / 2
  const double ex = 2.0 * c->geom.len_x, ey = 2.0 * c->geom.len_y, ez = c->z_high - c->z_low;
  const double r3 = c->r3_extent_override > 0.0 ? c->r3_extent_override : std::sqrt(ex * ex + ey * ey + ez * ez);
  t->range = prm->range > 0.0 ? prm->range : 0.2 * (r3 + 0.5 * 3.14159265358979323846);
  t->cap = prm->max_vertices;
  t->kmax = std::max(1, tree_k(prm->rewire_factor, t->cap));
  const size_t cap = t->cap, B = prm->batch, BK = B * (size_t)t->kmax;
  HIP_TRY(c, t->mem.alloc(&t->d_verts, cap * 7));
  HIP_TRY(c, t->mem.alloc(&t->d_cost, cap));
  HIP_TRY(c, t->mem.alloc(&t->d_ecost, cap));
  HIP_TRY(c, t->mem.alloc(&t->d_parent, cap));
  HIP_TRY(c, t->mem.alloc(&t->d_born, cap));
  HIP_TRY(c, t->mem.alloc(&t->d_pruned, cap));
  HIP_TRY(c, t->mem.alloc(&t->d_best_bits, cap));
  HIP_TRY(c, t->mem.alloc(&t->d_best_id, cap));
  HIP_TRY(c, t->mem.alloc(&t->d_pred_w, cap));
  HIP_TRY(c, t->mem.alloc(&t->d_hops, cap));
  HIP_TRY(c, t->mem.alloc(&t->d_sg, 14));
  HIP_TRY(c, t->mem.alloc(&t->d_samp, B * 7));
  HIP_TRY(c, t->mem.alloc(&t->d_xnew, B * 7));
  HIP_TRY(c, t->mem.alloc(&t->d_xs, B * 7));
  HIP_TRY(c, t->mem.alloc(&t->d_nd, B));
  HIP_TRY(c, t->mem.alloc(&t->d_c0, B));
  HIP_TRY(c, t->mem.alloc(&t->d_s1, BK * 7));
  HIP_TRY(c, t->mem.alloc(&t->d_s2, BK * 7));
  HIP_TRY(c, t->mem.alloc(&t->d_nn, B));
  HIP_TRY(c, t->mem.alloc(&t->d_idx1, B));
  HIP_TRY(c, t->mem.alloc(&t->d_idx2, B));
  HIP_TRY(c, t->mem.alloc(&t->d_rank, B));
  HIP_TRY(c, t->mem.alloc(&t->d_par0, B));
  HIP_TRY(c, t->mem.alloc(&t->d_near, BK));
  HIP_TRY(c, t->mem.alloc(&t->d_alive, B));
  HIP_TRY(c, t->mem.alloc(&t->d_valid1, B));
  HIP_TRY(c, t->mem.alloc(&t->d_validk, BK));
  HIP_TRY(c, t->mem.alloc(&t->d_cnt, 4));
  HIP_TRY(c, t->h_cnt.reserve(4 * 4, hipHostMallocDefault));
  HIP_TRY(c, t->mem.alloc(&t->d_counters, 2));
  HIP_TRY(c, t->mem.alloc(&t->d_err, 1));
  if (prm->profile)
    for (hipEvent_t& e : t->ev) HIP_TRY(c, hipEventCreate(&e));
  hipStream_t st = c->lane->stream;
  HIP_TRY(c, hipMemcpyAsync(t->d_sg, t->sg, 14 * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(t->d_verts, t->sg, 7 * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemsetAsync(t->d_cost, 0, 8, st));
  HIP_TRY(c, hipMemsetAsync(t->d_ecost, 0, 8, st));
  HIP_TRY(c, hipMemsetAsync(t->d_parent, 0xff, 4, st));
  HIP_TRY(c, hipMemsetAsync(t->d_born, 0, 4, st));
  HIP_TRY(c, hipMemsetAsync(t->d_pruned, 0, cap, st));
  HIP_TRY(c, hipMemsetAsync(t->d_counters, 0, 2 * 8, st));
  HIP_TRY(c, hipMemsetAsync(t->d_err, 0, sizeof(int), st));
  HIP_TRY(c, hipStreamSynchronize(st));
  *out = owner.release();
  return ARTP_OK;
}

int artp_tree_grow(artp_tree* t, uint64_t n_batches, uint64_t out[2]) {
  if (!t) return ARTP_ERR_INVALID_ARG;
  artp_ctx* c = t->ctx;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  const artp_tree_params& p = t->params;
  if (!n_batches && !p.max_batches && !(p.plan_time > 0.0)) {
    c->last_error = "artp_tree_grow needs a budget: n_batches, max_batches or plan_time";
    return ARTP_ERR_INVALID_ARG;
  }
  const auto t0 = std::chrono::steady_clock::now();
  uint64_t ran = 0;
  bool stop = t->n >= t->cap;
  while (!stop) {
    if (n_batches && ran >= n_batches) break;
    if (p.max_batches && t->batches >= p.max_batches) break;
    if (p.plan_time > 0.0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() >= p.plan_time)
      break;
    ARTP_TRY(tree_batch(t, &stop));
    ++ran;
  }
  ARTP_TRY(tree_check_err(t));
  if (out) {
    out[0] = ran;
    out[1] = t->n;
  }
  return ARTP_OK;
}

int artp_tree_stats(const artp_tree* t, uint64_t out[8]) {
  if (!t || !out) return ARTP_ERR_INVALID_ARG;
  artp_ctx* c = t->ctx;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  unsigned long long cnt[2] = {0, 0};
  std::vector<uint8_t> pr(t->n);
  HIP_TRY(c, hipMemcpyAsync(cnt, t->d_counters, sizeof(cnt), hipMemcpyDeviceToHost, c->lane->stream));
  HIP_TRY(c, hipMemcpyAsync(pr.data(), t->d_pruned, t->n, hipMemcpyDeviceToHost, c->lane->stream));
  HIP_TRY(c, hipStreamSynchronize(c->lane->stream));
  uint64_t np = 0;
  for (uint8_t b : pr) np += b ? 1 : 0;
  out[0] = t->n;
  out[1] = t->batches;
  out[2] = t->batches * (uint64_t)t->params.batch;
  out[3] = t->first_checked + cnt[0];
  out[4] = cnt[1];
  out[5] = np;
  out[6] = t->goal_id == artp::TREE_NONE ? ~0ull : (uint64_t)t->goal_id;
  out[7] = t->first_solution_batch;
  return ARTP_OK;
}

int artp_tree_export(const artp_tree* t, double* verts, uint32_t* parent, double* cost, double* edge_cost,
                     uint32_t* born_batch, uint8_t* pruned) {
  if (!t) return ARTP_ERR_INVALID_ARG;
  artp_ctx* c = t->ctx;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  const size_t n = t->n;
  hipStream_t st = c->lane->stream;
  if (verts) HIP_TRY(c, hipMemcpyAsync(verts, t->d_verts, n * 7 * 8, hipMemcpyDeviceToHost, st));
  if (parent) HIP_TRY(c, hipMemcpyAsync(parent, t->d_parent, n * 4, hipMemcpyDeviceToHost, st));
  if (cost) HIP_TRY(c, hipMemcpyAsync(cost, t->d_cost, n * 8, hipMemcpyDeviceToHost, st));
  if (edge_cost) HIP_TRY(c, hipMemcpyAsync(edge_cost, t->d_ecost, n * 8, hipMemcpyDeviceToHost, st));
  if (born_batch) HIP_TRY(c, hipMemcpyAsync(born_batch, t->d_born, n * 4, hipMemcpyDeviceToHost, st));
  if (pruned) HIP_TRY(c, hipMemcpyAsync(pruned, t->d_pruned, n, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return ARTP_OK;
}

int artp_tree_export_checked(const artp_tree* t, uint32_t* u, uint32_t* v, uint8_t* valid, uint32_t* batch, size_t cap,
                             size_t* n_out) {
  if (!t || !n_out) return ARTP_ERR_INVALID_ARG;
  artp_ctx* c = t->ctx;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  const size_t m = t->log_n;
  std::vector<uint32_t> lu(m), lv(m), lb(m);
  std::vector<uint8_t> lval(m);
  hipStream_t st = c->lane->stream;
  if (m) {
    HIP_TRY(c, hipMemcpyAsync(lu.data(), t->d_lu, m * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(lv.data(), t->d_lv, m * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(lb.data(), t->d_lbatch, m * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(lval.data(), t->d_lvalid, m, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
  }
  size_t k = 0;
  for (size_t e = 0; e < m; ++e) {
    if (lval[e] == 0xff) continue;
    if (k < cap) {
      if (u) u[k] = lu[e];
      if (v) v[k] = lv[e];
      if (valid) valid[k] = lval[e];
      if (batch) batch[k] = lb[e];
    }
    ++k;
  }
  *n_out = k;
  if (k > cap && (u || v || valid || batch)) {
    c->last_error = "checked-motion buffers too small";
    return ARTP_ERR_CAPACITY;
  }
  return ARTP_OK;
}

int artp_tree_solve(const artp_tree* t, double* path_se3, size_t cap_states, size_t* n_path, double* cost) {
  if (!t || !n_path) return ARTP_ERR_INVALID_ARG;
  artp_ctx* c = t->ctx;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  *n_path = 0;
  if (cost) *cost = INFINITY;
  if (t->goal_id == artp::TREE_NONE) return ARTP_OK;
  const size_t n = t->n;
  std::vector<uint32_t> parent(n);
  std::vector<double> verts(n * 7), costs(n);
  HIP_TRY(c, hipMemcpyAsync(parent.data(), t->d_parent, n * 4, hipMemcpyDeviceToHost, c->lane->stream));
  HIP_TRY(c, hipMemcpyAsync(verts.data(), t->d_verts, n * 7 * 8, hipMemcpyDeviceToHost, c->lane->stream));
  HIP_TRY(c, hipMemcpyAsync(costs.data(), t->d_cost, n * 8, hipMemcpyDeviceToHost, c->lane->stream));
  HIP_TRY(c, hipStreamSynchronize(c->lane->stream));
  std::vector<uint32_t> chain;
  for (uint32_t v = t->goal_id;; v = parent[v]) {
    chain.push_back(v);
    if (v == 0) break;
    if (chain.size() > n || parent[v] >= n) {
      c->last_error = "tree: the goal's parent chain does not reach the root";
      return ARTP_ERR_INVALID_ARG;
    }
  }
  const size_t np = chain.size();
  if (path_se3) {
    if (cap_states < np) {
      c->last_error = "path buffer too small";
      *n_path = np;
      return ARTP_ERR_CAPACITY;
    }
    for (size_t i = 0; i < np; ++i)
      std::memcpy(path_se3 + i * 7, &verts[(size_t)chain[np - 1 - i] * 7], 7 * sizeof(double));
  }
  *n_path = np;
  if (cost) *cost = costs[t->goal_id];
  return ARTP_OK;
}

int artp_tree_simplify_path(artp_tree* t, const double* path_se3, size_t n, double* out_se3, size_t* n_out, double* cost) {
  if (!t) return ARTP_ERR_INVALID_ARG;
  artp_roadmap_params prm;
  artp_roadmap_params_defaults(&prm);
  prm.objective = t->params.objective;
  prm.max_lon_vel = t->params.max_lon_vel;
  prm.max_lat_vel = t->params.max_lat_vel;
  prm.max_ang_vel = t->params.max_ang_vel;
  return roadmap_simplify_path_impl(t->ctx, &prm, path_se3, n, out_se3, n_out, cost);
}

int artp_tree_stage_times(const artp_tree* t, double us[10]) {
  if (!t || !us) return ARTP_ERR_INVALID_ARG;
  for (int i = 0; i < artp::TREE_NSTAGES; ++i) us[i] = t->stage_us[i];
  return ARTP_OK;
}

}  // extern "C"
