// roadmap_many.h -- artp_roadmap_solve_many: one start, many goals, one lazy search on the kept roadmap.
//
// For every goal the answer is what artp_roadmap_set_query(start, goal) + artp_roadmap_solve would give on the same
// roadmap, but the goals share the work:
//   * the start is attached once (its k nearest vertices, exactly set_query's list for vertex 0);
//   * every goal is attached to its own k nearest vertices (tree_knn_kernel shortlists k + a few, the host re-ranks
//     the shortlist with set_query's own formula: the neighbour sets are set_query's bit for bit);
//   * all attachment edges (start and goals) are evaluated in ONE roadmap_eval_edges_dev batch;
//   * each lazy round is one single-source search from the start over the roadmap edges (sssp_relax_kernel), one
//     predecessor tree (ties broken by hop count: no cycle through zero-weight edges), each unresolved goal's best
//     attachment, every unresolved path written out, the (edge, direction) pairs without a verdict collected once
//     however many paths share them, ONE batched motion check, and the invalid edges removed on the device.  A goal
//     whose whole path passed is frozen: removals only delete invalid edges, so its path stays a shortest valid one.
// The host reads counts only inside a round.  Goals whose query would change the start's own neighbour list ("near"
// goals: the goal enters the start's k-list or the start enters the goal's) go through set_query + solve themselves,
// with the query prefix of the roadmap restored byte for byte afterwards.  DESIGN.md "Many goals from one start" has
// the semantics, including why the equality with the sequential answers needs direction-symmetric verdicts.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace artp {

constexpr uint32_t MANY_NONE = 0xffffffffu;
constexpr int32_t MANY_PENDING = -1;  // device-side status of a goal still being planned

// per round: dist = +inf except the start, sweep stamps, hop counts, predecessor keys
__global__ void __launch_bounds__(256)
roadmap_many_init_kernel(int nv, unsigned long long* __restrict__ dist, unsigned* __restrict__ stamp,
                         uint32_t* __restrict__ hops, unsigned* __restrict__ hstamp, unsigned long long* __restrict__ pkey) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nv) return;
  dist[i] = i == 0 ? 0ull : 0x7ff0000000000000ull;
  stamp[i] = i == 0 ? 0u : 0xfefefefeu;  // the start "moved" in sweep 0 (0xfefefefe + 1 is never a sweep number)
  hops[i] = i == 0 ? 0u : MANY_NONE;
  hstamp[i] = i == 0 ? 0u : 0xfefefefeu;
  pkey[i] = ~0ull;
}

__device__ __forceinline__ bool many_tight(const unsigned long long* dist, uint32_t u, uint32_t v, double w) {
  const double du = __longlong_as_double((long long)dist[u]), dv = __longlong_as_double((long long)dist[v]);
  return v != 0 && du < INFINITY && du + w == dv;
}

// hops[v] = the fewest tight edges (dist[u] + w == dist[v] bit for bit) from the start to v, at the fixed point of
// sssp_relax_kernel.  Zero-weight edges make "tight" hold both ways, so tight edges alone can close a cycle; a
// predecessor one hop closer cannot.  Label-correcting sweeps with the same stamp rule as sssp_relax_kernel: an edge only
// has work when one of its ends moved in the previous sweep.
__global__ void __launch_bounds__(256)
roadmap_many_hops_kernel(const uint32_t* __restrict__ eu, const uint32_t* __restrict__ ev, const double* __restrict__ w,
                         size_t ne, const unsigned long long* __restrict__ dist, uint32_t* __restrict__ hops,
                         unsigned* __restrict__ hstamp, unsigned sweep, unsigned* __restrict__ changed) {
  unsigned local = 0;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (size_t)gridDim.x * blockDim.x) {
    const uint32_t u = eu[e], v = ev[e];
    if (hstamp[u] + 1u != sweep && hstamp[v] + 1u != sweep) continue;
    const double we = w[e];
    if (!(we < INFINITY)) continue;
    const uint32_t hu = __hip_atomic_load(&hops[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t hv = __hip_atomic_load(&hops[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (hu != MANY_NONE && hu + 1u < hv && many_tight(dist, u, v, we)) {
      if (atomicMin(&hops[v], hu + 1u) > hu + 1u) {
        hstamp[v] = sweep;
        local = 1;
      }
    } else if (hv != MANY_NONE && hv + 1u < hu && many_tight(dist, v, u, we)) {
      if (atomicMin(&hops[u], hv + 1u) > hv + 1u) {
        hstamp[u] = sweep;
        local = 1;
      }
    }
  }
  if (__any(local) && (threadIdx.x & 63) == 0) atomicAdd(changed, 1u);
}

// pkey[v] = (u << 32 | edge) of the smallest u with a tight edge u -> v and hops[u] + 1 == hops[v] (the rule of
// rrt_sharp's predecessors in tree.h): deterministic, and every chain reaches the start in hops[v] steps
__global__ void __launch_bounds__(256)
roadmap_many_pred_kernel(const uint32_t* __restrict__ eu, const uint32_t* __restrict__ ev, const double* __restrict__ w,
                         size_t ne, const unsigned long long* __restrict__ dist, const uint32_t* __restrict__ hops,
                         unsigned long long* __restrict__ pkey) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (size_t)gridDim.x * blockDim.x) {
    const double we = w[e];
    if (!(we < INFINITY)) continue;
    const uint32_t u = eu[e], v = ev[e];
    const uint32_t hu = hops[u], hv = hops[v];
    if (hu != MANY_NONE && hu + 1u == hv && many_tight(dist, u, v, we))
      atomicMin(&pkey[v], ((unsigned long long)u << 32) | (unsigned long long)e);
    if (hv != MANY_NONE && hv + 1u == hu && many_tight(dist, v, u, we))
      atomicMin(&pkey[u], ((unsigned long long)v << 32) | (unsigned long long)e);
  }
}

// One lane per goal: argmin over the goal's k attachment edges of dist[n] + w (ties: the smaller n), skipping
// unusable / dropped ones (w = +inf).  Writes the path length in states (start .. n, goal) for the scan; a pending goal
// with no reachable attachment is unreachable for good (the graph only loses edges).
__global__ void __launch_bounds__(256)
roadmap_many_attach_kernel(int ng, int k, const uint32_t* __restrict__ an, const double* __restrict__ aw,
                           const unsigned long long* __restrict__ dist, const uint32_t* __restrict__ hops,
                           int32_t* __restrict__ status, double* __restrict__ cost, uint32_t* __restrict__ best_a,
                           uint32_t* __restrict__ len, unsigned* __restrict__ err) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g > ng) return;
  if (g == ng) {  // the scan's last slot: the round's total
    len[g] = 0;
    return;
  }
  len[g] = 0;
  best_a[g] = MANY_NONE;
  if (status[g] != MANY_PENDING) return;
  double best = INFINITY;
  uint32_t ba = MANY_NONE, bn = MANY_NONE;
  for (int a = 0; a < k; ++a) {
    const size_t s = (size_t)g * k + a;
    const uint32_t n = an[s];
    if (n == MANY_NONE) continue;
    const double wa = aw[s];
    if (!(wa < INFINITY)) continue;
    const double dn = __longlong_as_double((long long)dist[n]);
    if (!(dn < INFINITY)) continue;
    const double val = dn + wa;  // the sequential search's last relaxation: g[n] + w
    if (val < best || (val == best && n < bn)) {
      best = val;
      ba = (uint32_t)a;
      bn = n;
    }
  }
  if (ba == MANY_NONE) {
    status[g] = 2;  // ARTP_GOAL_UNREACHABLE
    cost[g] = INFINITY;
    return;
  }
  if (hops[bn] == MANY_NONE) {  // cannot happen: every reached vertex has a tight chain from the start
    atomicOr(err, 1u);
    status[g] = 2;
    cost[g] = INFINITY;
    return;
  }
  best_a[g] = ba;
  cost[g] = best;
  len[g] = hops[bn] + 2u;
}

// One lane per goal with a path: the states (vertex ids; goal g is id nv + g) and, per state after the first, the
// item of the edge that reaches it -- 2 e + d for graph edge e travelled eu -> ev (d = 0) or ev -> eu (d = 1),
// 2 ne + slot for the goal's attachment.  pos_goal[p] = the goal a path position belongs to.
__global__ void __launch_bounds__(256)
roadmap_many_path_kernel(int ng, int k, int nv, size_t ne, const uint32_t* __restrict__ eu, const uint32_t* __restrict__ an,
                         const uint32_t* __restrict__ best_a, const uint32_t* __restrict__ len,
                         const uint32_t* __restrict__ off, const unsigned long long* __restrict__ pkey,
                         uint32_t* __restrict__ pv, uint32_t* __restrict__ pitem, uint32_t* __restrict__ pgoal,
                         unsigned* __restrict__ err) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ng || best_a[g] == MANY_NONE) return;
  const uint32_t base = off[g], L = len[g];
  const uint32_t slot = (uint32_t)g * (uint32_t)k + best_a[g];
  pv[base + L - 1] = (uint32_t)nv + (uint32_t)g;
  pitem[base + L - 1] = (uint32_t)(2 * ne) + slot;
  pgoal[base + L - 1] = (uint32_t)g;
  uint32_t v = an[slot];
  for (uint32_t pos = base + L - 2;; --pos) {
    pv[pos] = v;
    pgoal[pos] = (uint32_t)g;
    if (v == 0) {
      pitem[pos] = MANY_NONE;
      if (pos != base) atomicOr(err, 1u);  // cannot happen: the chain takes exactly hops[n] steps
      return;
    }
    const unsigned long long key = pkey[v];
    if (key == ~0ull || pos == base) {  // cannot happen at the fixed point
      atomicOr(err, 1u);
      return;
    }
    const uint32_t u = (uint32_t)(key >> 32), e = (uint32_t)(key & 0xffffffffu);
    pitem[pos] = 2u * e + (u == eu[e] ? 0u : 1u);
    v = u;
  }
}

// Items of this round's paths without a verdict, each (edge, direction) once however many paths share it: the
// verdict word goes 0 -> 3 (pending) for the lane that claims it.
__global__ void __launch_bounds__(256)
roadmap_many_collect_kernel(uint32_t total, size_t ne, const uint32_t* __restrict__ pv, const uint32_t* __restrict__ pitem,
                            uint32_t* __restrict__ verdict, uint32_t* __restrict__ averdict, uint32_t* __restrict__ items,
                            uint32_t* __restrict__ isrc, uint32_t* __restrict__ idst, unsigned* __restrict__ count) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= total) return;
  const uint32_t code = pitem[p];
  if (code == MANY_NONE) return;
  bool mine;
  if (code < 2 * ne) {
    mine = verdict[code] == 0u && atomicCAS(&verdict[code], 0u, 3u) == 0u;
  } else {  // an attachment lies on its own goal's path only
    mine = averdict[code - 2 * ne] == 0u;
    if (mine) averdict[code - 2 * ne] = 3u;
  }
  if (!mine) return;
  const unsigned i = atomicAdd(count, 1u);
  items[i] = code;
  isrc[i] = pv[p - 1];  // code != NONE only after a path's first state
  idst[i] = pv[p];
}

__global__ void __launch_bounds__(256)
roadmap_many_scatter_kernel(unsigned m, size_t ne, const uint32_t* __restrict__ items, const uint8_t* __restrict__ ok,
                            uint32_t* __restrict__ verdict, uint32_t* __restrict__ averdict) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint32_t code = items[i];
  const uint32_t val = ok[i] ? 1u : 2u;
  if (code < 2 * ne) verdict[code] = val;
  else averdict[code - 2 * ne] = val;
}

// Every invalid item on a path: the lazy check's removal -- the whole undirected edge (weight +inf, removed flag), or
// the goal's attachment -- and one removal more for the goal whose path it lies on
__global__ void __launch_bounds__(256)
roadmap_many_remove_kernel(uint32_t total, size_t ne, const uint32_t* __restrict__ pitem, const uint32_t* __restrict__ pgoal,
                           const uint32_t* __restrict__ verdict, const uint32_t* __restrict__ averdict,
                           double* __restrict__ w, uint8_t* __restrict__ removed, double* __restrict__ aw,
                           uint32_t* __restrict__ nbad) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= total) return;
  const uint32_t code = pitem[p];
  if (code == MANY_NONE) return;
  if (code < 2 * ne) {
    if (verdict[code] != 2u) return;
    w[code >> 1] = INFINITY;
    removed[code >> 1] = 1;
  } else {
    if (averdict[code - 2 * ne] != 2u) return;
    aw[code - 2 * ne] = INFINITY;
  }
  atomicAdd(&nbad[pgoal[p]], 1u);
}

// One lane per goal with a path this round: all valid -> solved and frozen at (round, offset, length); else its
// removals are counted (more than max_replans: ARTP_GOAL_TOO_MANY_REMOVALS) and it plans again next round.
__global__ void __launch_bounds__(256)
roadmap_many_resolve_kernel(int ng, uint32_t round, uint32_t max_replans, const uint32_t* __restrict__ best_a,
                            const uint32_t* __restrict__ len, const uint32_t* __restrict__ off, uint32_t* __restrict__ nbad,
                            uint32_t* __restrict__ removals, int32_t* __restrict__ status, double* __restrict__ cost,
                            uint32_t* __restrict__ fround, uint32_t* __restrict__ foff, uint32_t* __restrict__ flen,
                            unsigned* __restrict__ n_bad_goals) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ng || best_a[g] == MANY_NONE) return;
  const uint32_t b = nbad[g];
  if (b == 0) {
    status[g] = 0;  // ARTP_GOAL_SOLVED
    fround[g] = round;
    foff[g] = off[g];
    flen[g] = len[g];
    return;
  }
  nbad[g] = 0;
  removals[g] += b;
  if (removals[g] > max_replans) {
    status[g] = 3;  // ARTP_GOAL_TOO_MANY_REMOVALS
    cost[g] = INFINITY;
    return;
  }
  atomicAdd(n_bad_goals, 1u);
}

}  // namespace artp

namespace {

// set_query's distance (artp_roadmap_set_query): |dp| + the host acos of the quaternion dot product
inline double many_host_distance(const double* a, const double* b) {
  const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  const double dq = std::fabs(a[3] * b[3] + a[4] * b[4] + a[5] * b[5] + a[6] * b[6]);
  return std::sqrt(dx * dx + dy * dy + dz * dz) + (dq > 1.0 - 1e-9 ? 0.0 : std::acos(dq));
}

// set_query's neighbour list of a query state over the vertices j >= 2 not in vinvalid, ascending (distance, id)
void many_host_knn(const artp_roadmap* rm, const double* q, int k, std::vector<std::pair<double, uint32_t>>* out) {
  const size_t nv = rm->nv();
  std::vector<std::pair<double, uint32_t>> cand;
  cand.reserve(nv);
  for (uint32_t j = 2; j < nv; ++j) {
    if (j < rm->vinvalid.size() && rm->vinvalid[j]) continue;
    cand.push_back({many_host_distance(q, &rm->verts[(size_t)j * 7]), j});
  }
  const size_t kk = std::min<size_t>((size_t)k, cand.size());
  std::partial_sort(cand.begin(), cand.begin() + kk, cand.end());
  out->assign(cand.begin(), cand.begin() + kk);
}

// The query prefix of the roadmap (vertices 0 and 1, their knn rows, the edges touching them, the verdict cache) as it
// was before the exact fallback ran set_query + solve on it; restore() puts it back byte for byte.  Removals the fallback
// found on roadmap edges stay, like solve's.
struct QuerySnapshot {
  double sg[14];
  std::vector<uint32_t> knn, eu, ev, einterp;
  std::vector<double> knn_dist, ecost;
  std::vector<uint8_t> evalid, eremoved, eflip, emotion;
  uint64_t emotion_map_version = 0;
  bool emotion_dirty = true;
  size_t prefix = 0;
  void take(const artp_roadmap* rm, size_t first_keep) {
    const size_t k2 = 2 * (size_t)rm->k;
    std::memcpy(sg, rm->verts.data(), sizeof(sg));
    knn.assign(rm->knn.begin(), rm->knn.begin() + k2);
    knn_dist.assign(rm->knn_dist.begin(), rm->knn_dist.begin() + k2);
    prefix = first_keep;
    eu.assign(rm->eu.begin(), rm->eu.begin() + prefix);
    ev.assign(rm->ev.begin(), rm->ev.begin() + prefix);
    evalid.assign(rm->evalid.begin(), rm->evalid.begin() + prefix);
    einterp.assign(rm->einterp.begin(), rm->einterp.begin() + prefix);
    ecost.assign(rm->ecost.begin(), rm->ecost.begin() + prefix);
    eremoved.assign(rm->eremoved.begin(), rm->eremoved.begin() + prefix);
    if (!rm->eflip.empty()) eflip.assign(rm->eflip.begin(), rm->eflip.begin() + prefix);
    emotion = rm->emotion;
    emotion_map_version = rm->emotion_map_version;
    emotion_dirty = rm->emotion_dirty;
  }
  void restore(artp_roadmap* rm) const {
    size_t cur = 0;
    while (cur < rm->eu.size() && rm->eu[cur] < 2) ++cur;
    auto put = [&](auto& vec, const auto& head) {
      vec.erase(vec.begin(), vec.begin() + cur);
      vec.insert(vec.begin(), head.begin(), head.end());
    };
    std::memcpy(rm->verts.data(), sg, sizeof(sg));
    std::copy(knn.begin(), knn.end(), rm->knn.begin());
    std::copy(knn_dist.begin(), knn_dist.end(), rm->knn_dist.begin());
    put(rm->eu, eu);
    put(rm->ev, ev);
    put(rm->evalid, evalid);
    put(rm->einterp, einterp);
    put(rm->ecost, ecost);
    put(rm->eremoved, eremoved);
    if (!rm->eflip.empty()) put(rm->eflip, eflip);
    roadmap_edges_changed(rm);  // derived state: rebuilt from the restored arrays when next needed ...
    rm->emotion = emotion;      // ... but for the verdict cache, which comes back with the list it was taken for
    rm->emotion_map_version = emotion_map_version;
    rm->emotion_dirty = emotion_dirty;
  }
};

// the device part: goals gi[0 .. ng) (indices into goals), attached to an[ng x k] with weights aw; the start's
// attachment list is snb.  Fills status / cost of those goals and their paths as vertex-id lists (vertex nv + i =
// goals row gi[i]).
int many_device_solve(artp_roadmap* rm, const double* start7, const double* goals, const std::vector<uint32_t>& gi,
                      const std::vector<uint32_t>& an, const std::vector<double>& aw, const std::vector<uint32_t>& snb,
                      const std::vector<double>& sw, int32_t* status, double* cost,
                      std::vector<std::vector<uint32_t>>* paths, uint64_t stats[4]) {
  artp_ctx* c = rm->ctx;
  hipStream_t st = c->lane->stream;
  const int k = rm->k;
  const size_t nv = rm->nv(), ng = gi.size();
  size_t first_keep = 0;
  while (first_keep < rm->eu.size() && rm->eu[first_keep] < 2) ++first_keep;
  const size_t nr = rm->eu.size() - first_keep, ns = snb.size(), ne = nr + ns;
  // graph: the roadmap edges with both ends >= 2 (what roadmap_sssp_dev counts as usable), then the start's
  std::vector<uint32_t> heu(ne), hev(ne);
  std::vector<double> hw(ne);
  for (size_t e = 0; e < nr; ++e) {
    const size_t r = first_keep + e;
    heu[e] = rm->eu[r];
    hev[e] = rm->ev[r];
    hw[e] = roadmap_edge_weight(rm, r);
  }
  for (size_t t = 0; t < ns; ++t) {
    heu[nr + t] = 0;
    hev[nr + t] = snb[t];
    hw[nr + t] = sw[t];
  }
  // verdicts known for this map (rm->emotion, the solve loop's cache) are used, not recomputed
  const uint64_t mv = artp_map_version(c);
  const bool cache_ok = !rm->emotion_dirty && rm->emotion.size() == 2 * rm->eu.size() && rm->emotion_map_version == mv;
  std::vector<uint32_t> hverdict(2 * ne, 0u);
  if (cache_ok)
    for (size_t s = 0; s < 2 * nr; ++s) hverdict[s] = rm->emotion[2 * first_keep + s];
  // vertex states: the roadmap's, row 0 = the new start, then the goals
  std::vector<double> hV((nv + ng) * 7);
  std::memcpy(hV.data(), rm->verts.data(), nv * 7 * sizeof(double));
  std::memcpy(hV.data(), start7, 7 * sizeof(double));
  for (size_t i = 0; i < ng; ++i) std::memcpy(&hV[(nv + i) * 7], goals + (size_t)gi[i] * 7, 7 * sizeof(double));

  DeviceScratch B;
  const size_t nvv = nv + ng, nga = ng * (size_t)k;
  double *d_V, *d_w, *d_aw, *d_cost, *d_s = nullptr;
  uint32_t *d_euv, *d_verdict, *d_an, *d_averdict, *d_hops, *d_best, *d_len, *d_off, *d_nbad, *d_remv, *d_fround,
      *d_foff, *d_flen, *d_pitem = nullptr, *d_pgoal = nullptr, *d_items = nullptr, *d_isrc = nullptr;
  int32_t* d_status;
  unsigned long long *d_dist, *d_pkey;
  unsigned *d_stamp, *d_hstamp, *d_cnt;
  uint8_t* d_removed;
  uint8_t* d_ok = nullptr;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, B.alloc(&d_V, nvv * 7));
  HIP_TRY(c, B.alloc(&d_euv, 2 * ne));
  HIP_TRY(c, B.alloc(&d_w, ne));
  HIP_TRY(c, B.alloc(&d_removed, ne));
  HIP_TRY(c, B.alloc(&d_verdict, 2 * ne));
  HIP_TRY(c, B.alloc(&d_an, nga));
  HIP_TRY(c, B.alloc(&d_aw, nga));
  HIP_TRY(c, B.alloc(&d_averdict, nga));
  HIP_TRY(c, B.alloc(&d_dist, nv));
  HIP_TRY(c, B.alloc(&d_pkey, nv));
  HIP_TRY(c, B.alloc(&d_stamp, nv));
  HIP_TRY(c, B.alloc(&d_hstamp, nv));
  HIP_TRY(c, B.alloc(&d_hops, nv));
  HIP_TRY(c, B.alloc(&d_status, ng));
  HIP_TRY(c, B.alloc(&d_cost, ng));
  HIP_TRY(c, B.alloc(&d_best, ng));
  HIP_TRY(c, B.alloc(&d_len, ng + 1));
  HIP_TRY(c, B.alloc(&d_off, ng + 1));
  HIP_TRY(c, B.alloc(&d_nbad, ng));
  HIP_TRY(c, B.alloc(&d_remv, ng));
  HIP_TRY(c, B.alloc(&d_fround, ng));
  HIP_TRY(c, B.alloc(&d_foff, ng));
  HIP_TRY(c, B.alloc(&d_flen, ng));
  HIP_TRY(c, B.alloc(&d_cnt, 8));  // [0] sssp changed, [1] hops changed, [2] items, [3] goals with a bad path, [4] error
  HIP_TRY(c, hipMemcpyAsync(d_V, hV.data(), nvv * 7 * sizeof(double), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_euv, heu.data(), ne * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_euv + ne, hev.data(), ne * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_w, hw.data(), ne * sizeof(double), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemsetAsync(d_removed, 0, ne, st));
  HIP_TRY(c, hipMemcpyAsync(d_verdict, hverdict.data(), 2 * ne * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_an, an.data(), nga * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_aw, aw.data(), nga * sizeof(double), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemsetAsync(d_averdict, 0, nga * 4, st));
  {
    const std::vector<int32_t> pending(ng, artp::MANY_PENDING);
    HIP_TRY(c, hipMemcpyAsync(d_status, pending.data(), ng * 4, hipMemcpyHostToDevice, st));
  }
  HIP_TRY(c, hipMemsetAsync(d_cost, 0, ng * sizeof(double), st));
  HIP_TRY(c, hipMemsetAsync(d_nbad, 0, ng * 4, st));
  HIP_TRY(c, hipMemsetAsync(d_remv, 0, ng * 4, st));
  HIP_TRY(c, hipMemsetAsync(d_cnt, 0, 8 * 4, st));
  const uint32_t* d_eu = d_euv;
  const uint32_t* d_ev = d_euv + ne;
  size_t blocks = (ne + 255) / 256;
  if (blocks > (size_t)c->n_cus * 8) blocks = (size_t)c->n_cus * 8;
  if (blocks == 0) blocks = 1;
  void* d_scan = nullptr;
  size_t scan_bytes = 0;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, d_len, d_off, (int)(ng + 1), st));
  HIP_TRY(c, B.alloc(reinterpret_cast<uint8_t**>(&d_scan), scan_bytes + 256));
  scan_bytes += 256;
  std::vector<uint32_t*> round_pv;  // every round's path states: frozen goals point into them
  std::vector<uint32_t> round_total;
  size_t cap_items = 0;
  uint64_t rounds = 0, motions = 0;
  for (;;) {
    // 1. shortest paths from the start (sssp_relax_kernel as roadmap_sssp_dev runs it)
    hipLaunchKernelGGL(artp::roadmap_many_init_kernel, dim3(tree_blocks(nv)), dim3(256), 0, st, (int)nv, d_dist, d_stamp,
                       d_hops, d_hstamp, d_pkey);
    unsigned cnt[8];
    // sweep groups of 16, 32, 64, 64, ... between host reads (the sparse construction-1 graphs take hundreds of sweeps)
    ARTP_TRY(roadmap_sweep_to_fixed_point(c, d_cnt, 16, 64, [&](unsigned sweep) {
      hipLaunchKernelGGL(artp::sssp_relax_kernel, dim3((unsigned)blocks), dim3(256), 0, st, d_eu, d_ev, (const double*)d_w,
                         ne, d_dist, d_stamp, sweep, d_cnt);
    }));
    // 2. hop counts over the tight edges, predecessors one hop closer
    ARTP_TRY(roadmap_sweep_to_fixed_point(c, d_cnt + 1, 16, 64, [&](unsigned sweep) {
      hipLaunchKernelGGL(artp::roadmap_many_hops_kernel, dim3((unsigned)blocks), dim3(256), 0, st, d_eu, d_ev,
                         (const double*)d_w, ne, (const unsigned long long*)d_dist, d_hops, d_hstamp, sweep, d_cnt + 1);
    }));
    hipLaunchKernelGGL(artp::roadmap_many_pred_kernel, dim3((unsigned)blocks), dim3(256), 0, st, d_eu, d_ev,
                       (const double*)d_w, ne, (const unsigned long long*)d_dist, (const uint32_t*)d_hops, d_pkey);
    // 3. best attachment per pending goal, 4. path lengths -> offsets
    hipLaunchKernelGGL(artp::roadmap_many_attach_kernel, dim3(tree_blocks(ng + 1)), dim3(256), 0, st, (int)ng, k,
                       (const uint32_t*)d_an, (const double*)d_aw, (const unsigned long long*)d_dist,
                       (const uint32_t*)d_hops, d_status, d_cost, d_best, d_len, d_cnt + 4);
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(d_scan, scan_bytes, d_len, d_off, (int)(ng + 1), st));
    uint32_t total = 0;
    HIP_TRY(c, hipMemcpyAsync(&total, d_off + ng, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (total == 0) break;  // no pending goal has a path left
    ++rounds;
    uint32_t* d_pv;
    HIP_TRY(c, B.alloc(&d_pv, total));
    round_pv.push_back(d_pv);
    round_total.push_back(total);
    if (total > cap_items) {  // per-round scratch sized by the largest round
      cap_items = std::max<size_t>(total, 2 * cap_items);
      HIP_TRY(c, B.alloc(&d_pitem, cap_items));
      HIP_TRY(c, B.alloc(&d_pgoal, cap_items));
      HIP_TRY(c, B.alloc(&d_items, cap_items));
      HIP_TRY(c, B.alloc(&d_isrc, 2 * cap_items));
      HIP_TRY(c, B.alloc(&d_s, 2 * cap_items * 7));
      HIP_TRY(c, B.alloc(&d_ok, cap_items));
    }
    hipLaunchKernelGGL(artp::roadmap_many_path_kernel, dim3(tree_blocks(ng)), dim3(256), 0, st, (int)ng, k, (int)nv, ne,
                       d_eu, (const uint32_t*)d_an, (const uint32_t*)d_best, (const uint32_t*)d_len,
                       (const uint32_t*)d_off, (const unsigned long long*)d_pkey, d_pv, d_pitem, d_pgoal, d_cnt + 4);
    // 5. unchecked (edge, direction) items of all paths, once each
    HIP_TRY(c, hipMemsetAsync(d_cnt + 2, 0, 8, st));
    hipLaunchKernelGGL(artp::roadmap_many_collect_kernel, dim3(tree_blocks(total)), dim3(256), 0, st, total, ne,
                       (const uint32_t*)d_pv, (const uint32_t*)d_pitem, d_verdict, d_averdict, d_items, d_isrc,
                       d_isrc + cap_items, d_cnt + 2);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(cnt + 2, d_cnt + 2, 12, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (cnt[4]) {
      c->last_error = "artp_roadmap_solve_many: broken predecessor chain";
      return ARTP_ERR_HIP;
    }
    const unsigned m = cnt[2];
    // 6. one motion check for all of them (chunks of 2^18 motions, as roadmap_check_motion_items), verdicts scattered
    if (m) {
      hipLaunchKernelGGL(artp::gather_edge_states_uv_kernel, dim3(tree_blocks(m)), dim3(256), 0, st, (const double*)d_V,
                         (const uint32_t*)d_isrc, (const uint32_t*)(d_isrc + cap_items), (size_t)m, d_s,
                         d_s + (size_t)m * 7);
      HIP_TRY(c, hipGetLastError());
      for (size_t at = 0; at < m; at += (size_t)1 << 18) {
        const size_t mm = std::min<size_t>(m - at, (size_t)1 << 18);
        ARTP_TRY(artp_check_motions_dev(c, d_s + at * 7, d_s + ((size_t)m + at) * 7, mm, d_ok + at));
      }
      hipLaunchKernelGGL(artp::roadmap_many_scatter_kernel, dim3(tree_blocks(m)), dim3(256), 0, st, m, ne,
                         (const uint32_t*)d_items, (const uint8_t*)d_ok, d_verdict, d_averdict);
      motions += m;
    }
    // 7. removals, then freeze the goals whose whole path passed
    hipLaunchKernelGGL(artp::roadmap_many_remove_kernel, dim3(tree_blocks(total)), dim3(256), 0, st, total, ne,
                       (const uint32_t*)d_pitem, (const uint32_t*)d_pgoal, (const uint32_t*)d_verdict,
                       (const uint32_t*)d_averdict, d_w, d_removed, d_aw, d_nbad);
    hipLaunchKernelGGL(artp::roadmap_many_resolve_kernel, dim3(tree_blocks(ng)), dim3(256), 0, st, (int)ng,
                       (uint32_t)(round_pv.size() - 1), (uint32_t)rm->params.max_replans, (const uint32_t*)d_best,
                       (const uint32_t*)d_len, (const uint32_t*)d_off, d_nbad, d_remv, d_status, d_cost, d_fround,
                       d_foff, d_flen, d_cnt + 3);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(cnt + 3, d_cnt + 3, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    ARTP_TRY(check_error_flag(c));
    if (cnt[3] == 0) break;  // no pending goal's path had an invalid edge
  }
  // results: statuses, costs, frozen paths; removals and verdicts back into the roadmap
  std::vector<int32_t> hst(ng);
  std::vector<double> hcost(ng);
  std::vector<uint32_t> fr(ng), fo(ng), fl(ng), hav(nga);
  std::vector<uint8_t> hrem(ne);
  HIP_TRY(c, hipMemcpyAsync(hst.data(), d_status, ng * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(hcost.data(), d_cost, ng * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(fr.data(), d_fround, ng * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(fo.data(), d_foff, ng * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(fl.data(), d_flen, ng * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(hav.data(), d_averdict, nga * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(hrem.data(), d_removed, ne, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(hverdict.data(), d_verdict, 2 * ne * 4, hipMemcpyDeviceToHost, st));
  std::vector<std::vector<uint32_t>> rpv(round_pv.size());
  for (size_t r = 0; r < round_pv.size(); ++r) {
    rpv[r].resize(round_total[r]);
    HIP_TRY(c, hipMemcpyAsync(rpv[r].data(), round_pv[r], (size_t)round_total[r] * 4, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(c, hipStreamSynchronize(st));
  uint64_t n_removed = 0;
  for (size_t i = 0; i < ng; ++i) {
    const uint32_t g = gi[i];
    status[g] = hst[i] == artp::MANY_PENDING ? 2 : hst[i];  // pending with no path left cannot happen; unreachable
    cost[g] = status[g] == 0 ? hcost[i] : INFINITY;
    if (status[g] == 0) (*paths)[g].assign(rpv[fr[i]].begin() + fo[i], rpv[fr[i]].begin() + fo[i] + fl[i]);
    for (int a = 0; a < k; ++a) n_removed += hav[i * k + a] == 2u;
  }
  for (size_t e = 0; e < ne; ++e) {
    n_removed += hrem[e];
    if (e < nr && hrem[e]) roadmap_remove_edge(rm, first_keep + e);
  }
  if (!cache_ok) {  // the solve loop's rule: a stale table is cleared for this map and edge list first
    rm->emotion.assign(2 * rm->eu.size(), 0);
    rm->emotion_map_version = mv;
    rm->emotion_dirty = false;
  }
  for (size_t s = 0; s < 2 * nr; ++s)
    if (hverdict[s] == 1u || hverdict[s] == 2u) rm->emotion[2 * first_keep + s] = (uint8_t)hverdict[s];
  stats[0] += rounds;
  stats[1] += n_removed;
  stats[2] += motions;
  return ARTP_OK;
}

}  // namespace

extern "C" {

int artp_roadmap_solve_many(artp_roadmap* rm, const double* start_se3, const double* goals_se3, size_t n_goals,
                            int32_t* status, double* cost, uint64_t* path_offsets, double* path_se3, size_t cap_states,
                            uint64_t stats_out[4]) {
  if (!rm || !start_se3 || (n_goals > 0 && (!goals_se3 || !status || !cost))) return ARTP_ERR_INVALID_ARG;
  artp_ctx* c = rm->ctx;
  const size_t ng = n_goals, nv = rm->nv();
  const int k = rm->k;
  uint64_t stats[4] = {0, 0, 0, 0};
  // 1. validity: the start first (invalid: nothing changes), then the goals set_query would refuse
  std::vector<double> sg((ng + 1) * 7);
  std::memcpy(sg.data(), start_se3, 7 * sizeof(double));
  if (ng) std::memcpy(sg.data() + 7, goals_se3, ng * 7 * sizeof(double));
  std::vector<uint8_t> ok(ng + 1, 0);
  ARTP_TRY(artp_validate_states(c, sg.data(), ng + 1, ok.data(), nullptr));
  ARTP_TRY(roadmap_require_valid_query(c, ok[0], true));  // an invalid goal is that goal's status, not an error
  if (path_offsets) path_offsets[0] = 0;
  if (ng == 0) {
    if (stats_out) std::memset(stats_out, 0, 4 * sizeof(uint64_t));
    return ARTP_OK;
  }
  const double* goals = goals_se3;
  std::vector<std::vector<uint32_t>> paths(ng);      // device-answered goals: vertex ids (nv + i = goal gi[i])
  std::vector<std::vector<double>> near_paths(ng);   // fallback goals: states
  std::vector<uint8_t> is_near(ng, 0);
  // 2. the start's neighbour list over the vertices >= 2 (set_query's list for vertex 0 when the goal is not in it)
  std::vector<std::pair<double, uint32_t>> ls;
  many_host_knn(rm, start_se3, k, &ls);
  // 3. the goals' lists: shortlist k + margin on the device (tree_knn_kernel), exact re-rank on the host
  std::vector<uint32_t> pend;  // valid goals
  for (size_t g = 0; g < ng; ++g) {
    status[g] = ok[g + 1] ? 0 : 1;  // ARTP_GOAL_INVALID
    cost[g] = INFINITY;
    if (ok[g + 1]) pend.push_back((uint32_t)g);
  }
  std::vector<std::vector<std::pair<double, uint32_t>>> lg(pend.size());
  const int kk = std::min(k + 8, artp::TREE_KMAX);
  if (!pend.empty()) {
    std::vector<uint32_t> sid;
    std::vector<double> sd;
    if (kk > k) {
      DeviceScratch B;
      double *d_v, *d_q, *d_d;
      uint32_t* d_id;
      uint8_t* d_pr;
      const size_t nq = pend.size();
      std::vector<double> q(nq * 7);
      for (size_t i = 0; i < nq; ++i) std::memcpy(&q[i * 7], goals + (size_t)pend[i] * 7, 7 * sizeof(double));
      std::vector<uint8_t> pr(nv, 0);
      for (size_t j = 0; j < nv; ++j) pr[j] = j < 2 || (j < rm->vinvalid.size() && rm->vinvalid[j]);
      HIP_TRY(c, hipSetDevice(c->device));
      HIP_TRY(c, B.alloc(&d_v, nv * 7));
      HIP_TRY(c, B.alloc(&d_q, nq * 7));
      HIP_TRY(c, B.alloc(&d_d, nq * kk));
      HIP_TRY(c, B.alloc(&d_id, nq * kk));
      HIP_TRY(c, B.alloc(&d_pr, nv));
      HIP_TRY(c, hipMemcpyAsync(d_v, rm->verts.data(), nv * 7 * sizeof(double), hipMemcpyHostToDevice, c->lane->stream));
      HIP_TRY(c, hipMemcpyAsync(d_q, q.data(), nq * 7 * sizeof(double), hipMemcpyHostToDevice, c->lane->stream));
      HIP_TRY(c, hipMemcpyAsync(d_pr, pr.data(), nv, hipMemcpyHostToDevice, c->lane->stream));
      hipLaunchKernelGGL(artp::tree_knn_kernel, dim3(tree_blocks(nq, 4)), dim3(256), 0, c->lane->stream, (const double*)d_v,
                         (int)nv, (const uint8_t*)d_pr, (const double*)d_q, (int)nq, kk, d_id, d_d);
      HIP_TRY(c, hipGetLastError());
      sid.resize(nq * kk);
      sd.resize(nq * kk);
      HIP_TRY(c, hipMemcpyAsync(sid.data(), d_id, nq * kk * 4, hipMemcpyDeviceToHost, c->lane->stream));
      HIP_TRY(c, hipMemcpyAsync(sd.data(), d_d, nq * kk * sizeof(double), hipMemcpyDeviceToHost, c->lane->stream));
      HIP_TRY(c, hipStreamSynchronize(c->lane->stream));
    }
    for (size_t i = 0; i < pend.size(); ++i) {
      const double* q = goals + (size_t)pend[i] * 7;
      bool exact = false;
      if (kk > k) {
        std::vector<std::pair<double, uint32_t>> cand;
        for (int t = 0; t < kk; ++t) {
          const uint32_t j = sid[i * kk + t];
          if (j != artp::MANY_NONE) cand.push_back({many_host_distance(q, &rm->verts[(size_t)j * 7]), j});
        }
        std::sort(cand.begin(), cand.end());
        const size_t have = cand.size();
        if (have > (size_t)k) cand.resize(k);
        // the shortlist holds every candidate, or everything outside it is (device distance >= its last entry's, the
        // two formulas within 1e-9 of each other) farther than the k-th entry: the host order is set_query's
        exact = have < (size_t)kk || (!cand.empty() && sd[i * kk + kk - 1] - 1e-9 > cand.back().first);
        if (exact) lg[i].swap(cand);
      }
      if (!exact) many_host_knn(rm, q, k, &lg[i]);
    }
  }
  // 4. near goals: the goal would enter the start's list (id 1 beats any id >= 2 at equal distance), or the start would
  // enter the goal's (id 0)
  std::vector<uint32_t> far_goals;
  std::vector<size_t> far_row;
  for (size_t i = 0; i < pend.size(); ++i) {
    const uint32_t g = pend[i];
    const double* q = goals + (size_t)g * 7;
    const bool in_s = ls.size() < (size_t)k || many_host_distance(start_se3, q) <= ls.back().first;
    const bool in_g = lg[i].size() < (size_t)k || many_host_distance(q, start_se3) <= lg[i].back().first;
    if (in_s || in_g) {
      is_near[g] = 1;
    } else {
      far_goals.push_back(g);
      far_row.push_back(i);
    }
  }
  // 5. the exact fallback for near goals: set_query + solve on the roadmap itself, the query prefix restored after
  size_t first_keep = 0;
  while (first_keep < rm->eu.size() && rm->eu[first_keep] < 2) ++first_keep;
  {
    bool any = false;
    for (size_t g = 0; g < ng; ++g) any = any || is_near[g];
    if (any) {
      QuerySnapshot snap;
      snap.take(rm, first_keep);
      std::vector<double> buf(nv * 7 + 7);
      int rc = ARTP_OK;
      for (size_t g = 0; g < ng && rc == ARTP_OK; ++g) {
        if (!is_near[g]) continue;
        ++stats[3];
        rc = artp_roadmap_set_query(rm, start_se3, goals + g * 7);
        if (rc != ARTP_OK) break;
        size_t n = 0;
        double cst = INFINITY;
        int rep = 0;
        rc = artp_roadmap_solve(rm, buf.data(), nv + 1, &n, &cst, &rep);
        if (rc == ARTP_ERR_CAPACITY) {  // a path never has more states than the roadmap has vertices: too many removals
          status[g] = 3;
          rc = ARTP_OK;
        } else if (rc == ARTP_OK) {
          status[g] = n ? 0 : 2;
          cost[g] = n ? cst : INFINITY;
          if (n) near_paths[g].assign(buf.begin(), buf.begin() + n * 7);
        }
      }
      snap.restore(rm);
      if (rc != ARTP_OK) return rc;
    }
  }
  // 6. attachments of the start and the far goals: one edge evaluation batch (start -> neighbour, goal -> neighbour:
  // the directions set_query evaluates them in)
  if (!far_goals.empty()) {
    const size_t ns = ls.size(), nfg = far_goals.size(), na = ns + nfg * (size_t)k;
    std::vector<double> s12(2 * na * 7);
    std::vector<uint32_t> an(nfg * (size_t)k, artp::MANY_NONE);
    std::vector<double> aw(nfg * (size_t)k, INFINITY);
    std::vector<uint32_t> snb(ns);
    std::vector<double> sw(ns);
    size_t at = 0;
    auto put = [&](const double* a, uint32_t j) {
      std::memcpy(&s12[at * 7], a, 7 * sizeof(double));
      std::memcpy(&s12[(na + at) * 7], &rm->verts[(size_t)j * 7], 7 * sizeof(double));
      ++at;
    };
    for (size_t t = 0; t < ns; ++t) put(start_se3, snb[t] = ls[t].second);
    std::vector<size_t> arow;  // eval row of attachment slot i * k + t
    for (size_t i = 0; i < nfg; ++i) {
      const auto& L = lg[far_row[i]];
      for (size_t t = 0; t < L.size(); ++t) {
        an[i * k + t] = L[t].second;
        arow.push_back(at);
        put(goals + (size_t)far_goals[i] * 7, L[t].second);
      }
    }
    std::vector<uint8_t> evalid(at);
    std::vector<uint32_t> einterp(at);
    std::vector<double> ecost(at);
    {
      DeviceScratch B;
      double* d_s12;
      HIP_TRY(c, hipSetDevice(c->device));
      HIP_TRY(c, B.alloc(&d_s12, 2 * na * 7));
      HIP_TRY(c, hipMemcpy(d_s12, s12.data(), 2 * na * 7 * sizeof(double), hipMemcpyHostToDevice));
      ARTP_TRY(roadmap_eval_edges_dev(c, &rm->params, d_s12, d_s12 + na * 7, at, evalid.data(), einterp.data(),
                                      ecost.data(), rm->params.construction == 2));
    }
    auto usable = [&](size_t r) {
      return (evalid[r] && std::isfinite(ecost[r]) && ecost[r] >= 0.0) ? ecost[r] : INFINITY;
    };
    for (size_t t = 0; t < ns; ++t) sw[t] = usable(t);
    size_t ai = 0;
    for (size_t i = 0; i < nfg; ++i)
      for (size_t t = 0; t < lg[far_row[i]].size(); ++t) aw[i * k + t] = usable(arow[ai++]);
    // 7. the lazy rounds on the device
    ARTP_TRY(many_device_solve(rm, start_se3, goals, far_goals, an, aw, snb, sw, status, cost, &paths, stats));
  }
  // 8. offsets and states
  std::vector<uint64_t> off(ng + 1, 0);
  for (size_t g = 0; g < ng; ++g) {
    const size_t len = status[g] != 0 ? 0 : (is_near[g] ? near_paths[g].size() / 7 : paths[g].size());
    off[g + 1] = off[g] + len;
  }
  if (path_offsets) std::memcpy(path_offsets, off.data(), (ng + 1) * sizeof(uint64_t));
  if (stats_out) std::memcpy(stats_out, stats, sizeof(stats));
  if (path_se3) {
    if (cap_states < off[ng]) {
      c->last_error = "path buffer too small";
      return ARTP_ERR_CAPACITY;
    }
    for (size_t g = 0; g < ng; ++g) {
      if (status[g] != 0) continue;
      double* out = path_se3 + off[g] * 7;
      if (is_near[g]) {
        std::memcpy(out, near_paths[g].data(), near_paths[g].size() * sizeof(double));
        continue;
      }
      for (size_t i = 0; i < paths[g].size(); ++i) {
        const uint32_t v = paths[g][i];
        const double* src = v == 0 ? start_se3 : (v < nv ? &rm->verts[(size_t)v * 7] : goals + (size_t)g * 7);
        std::memcpy(out + i * 7, src, 7 * sizeof(double));
      }
    }
  }
  return ARTP_OK;
}

}  // extern "C"
