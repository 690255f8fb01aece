// field_simplify.h -- windowed shortcut simplification of many paths on a cost-to-go field's context (include/artp_c.h
// artp_field_simplify_paths).
//
// roadmap_simplify_path_impl (roadmap.h) tries every pair (i, j) of ONE path's states as a shortcut, lists the pairs on the
// host and runs the DAG search there.  Here the pairs are limited to a window (j - i <= window), all paths of a call share
// the batches, and nothing but the result comes back to the host:
//   field_simplify_pairs_kernel    one lane per candidate of a batch: (path, i, j) from the per-path prefix counts, the
//                                  two states written as the (s1, s2) the checks and the cost kernel read
//   roadmap_eval_edges_into        the 0.5 m interpolation rule and edge_chain_cost_kernel on its interior-state counts
//   run_edges_dev, mode 0          checkMotion
//   field_simplify_weight_kernel   w[candidate] = its cost where both verdicts pass and the cost is finite, else +inf
//   field_simplify_search_kernel   one wave per path, once per call: the forward DAG search of the host routine (i in
//                                  sequence, the lanes relax i's successors), the backtrack, kept indices, count and cost
//   field_simplify_gather_kernel   the kept states and indices of all paths into one compact buffer
// Candidate order: path by path, inside a path by i, inside i by j -- the host routine's order when the window covers the
// path.  Row i of a path of n states (m = n - 1 moves, w = min(window, m)) holds min(w, m - i) candidates: rows
// 0 .. m - w are full and start at i w, the tail rows shrink by one each.
#pragma once

namespace artp {

struct FieldSimplifyRec {  // the search's answer for one path
  int32_t status;          // 0 simplified, 1 the input chain does not pass, 2 empty
  uint32_t kept;           // states kept
  double cost;             // best[n - 1]
};

constexpr uint32_t FIELD_SIMPLIFY_LDS_STATES = 4096;  // best (f64) + from (u32) of a path this long: 48 KB of LDS

// candidates of a path of n states under window w0 (0 = all pairs)
__host__ __device__ inline unsigned long long field_simplify_count(unsigned long long n, unsigned long long w0) {
  if (n < 2) return 0;
  const unsigned long long m = n - 1, w = (w0 == 0 || w0 > m) ? m : w0;
  return w * (m - w + 1) + w * (w - 1) / 2;
}

// first candidate of row i (i < m)
__device__ __forceinline__ unsigned long long field_simplify_row(unsigned long long m, unsigned long long w, unsigned long long i) {
  if (i <= m - w) return i * w;
  const unsigned long long t = i - (m - w + 1);  // tail rows in front of row i: lengths w - 1, w - 2, ...
  return w * (m - w + 1) + t * (w - 1) - t * (t - 1) / 2;
}

// the path of item g: the last q with off[q] <= g (off ascends, off[0] = 0, g < off[n_paths]; empty paths are skipped)
__device__ __forceinline__ uint32_t field_simplify_path_of(const unsigned long long* __restrict__ off, uint32_t n_paths,
                                                           unsigned long long g) {
  uint32_t lo = 0, hi = n_paths;  // off[lo] <= g < off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// One lane per candidate g0 + e of the batch: s1[e] = state i, s2[e] = state j of its path.
__global__ void __launch_bounds__(256)
field_simplify_pairs_kernel(const double* __restrict__ se3, const unsigned long long* __restrict__ poff,
                            const unsigned long long* __restrict__ coff, uint32_t n_paths, unsigned long long window,
                            unsigned long long g0, size_t ne, double* __restrict__ s1, double* __restrict__ s2) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= ne) return;
  const unsigned long long g = g0 + e;
  const uint32_t q = field_simplify_path_of(coff, n_paths, g);
  const unsigned long long c = g - coff[q], base = poff[q], m = poff[q + 1] - base - 1;
  const unsigned long long w = (window == 0 || window > m) ? m : window;
  const unsigned long long full = w * (m - w + 1);
  unsigned long long i, j;
  if (c < full) {
    i = c / w;
    j = i + 1 + (c - i * w);
  } else {
    // the tail rows counted from the END have lengths 1, 2, 3, ...: r lies in row u with u (u + 1) / 2 <= r
    const unsigned long long r = full + w * (w - 1) / 2 - 1 - c;
    unsigned long long u = (unsigned long long)((sqrt(8.0 * (double)r + 1.0) - 1.0) * 0.5);
    while (u * (u + 1) / 2 > r) --u;
    while ((u + 1) * (u + 2) / 2 <= r) ++u;
    i = m - 1 - u;
    j = i + 1 + (u - (r - u * (u + 1) / 2));
  }
  const double* a = se3 + 7 * (base + i);
  const double* b = se3 + 7 * (base + j);
#pragma unroll
  for (int k = 0; k < 7; ++k) {
    s1[e * 7 + k] = a[k];
    s2[e * 7 + k] = b[k];
  }
}

// w[e] = the candidate's cost where it is usable, +inf where not; cnt[0] += usable candidates
__global__ void __launch_bounds__(256)
field_simplify_weight_kernel(const uint8_t* __restrict__ ok_interp, const uint8_t* __restrict__ ok_motion,
                             const double* __restrict__ cost, size_t ne, double* __restrict__ w,
                             unsigned long long* __restrict__ cnt) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool usable = false;
  if (e < ne) {
    const double c = cost[e];
    usable = ok_interp[e] && ok_motion[e] && isfinite(c);
    w[e] = usable ? c : INFINITY;
  }
  const unsigned long long votes = __ballot(usable);
  if ((threadIdx.x & 63) == 0 && votes) atomicAdd(&cnt[0], (unsigned long long)__popcll(votes));
}

// The search of one path on one wave.  best / from: n entries in LDS or in global memory.  Row i is relaxed by the lanes,
// 64 successors a step; the weights of the step after the current one are already on their way (they depend on nothing).
// best[j] is read and written by the one lane that owns j in a row, rows run in sequence, and a row only replaces on
// strictly smaller: the host routine's left fold and its "smallest i wins a tie".
template <class BestPtr, class FromPtr>
__device__ __forceinline__ void field_simplify_search(BestPtr best, FromPtr from, const double* __restrict__ wq, uint32_t n,
                                                      uint32_t w) {
  const uint32_t lane = threadIdx.x, m = n - 1;
  for (uint32_t v = lane; v < n; v += 64) {
    best[v] = v == 0 ? 0.0 : INFINITY;
    from[v] = 0xffffffffu;
  }
  __syncthreads();
  uint32_t ni = 0, nk = 0;  // the step whose weight is in `ahead`: row ni, successors ni + 1 + nk + lane
  double ahead = lane < (m < w ? m : w) ? wq[lane] : INFINITY;
  while (ni < m) {
    const uint32_t i = ni, k = nk;
    const double wv = ahead;
    const uint32_t len = m - i < w ? m - i : w;
    if (k + 64 < len) {
      nk = k + 64;
    } else {
      ni = i + 1;
      nk = 0;
    }
    if (ni < m) {
      const uint32_t nlen = m - ni < w ? m - ni : w;
      ahead = nk + lane < nlen ? wq[field_simplify_row(m, w, ni) + nk + lane] : INFINITY;
    }
    const double bi = best[i];
    if (bi < INFINITY && k + lane < len) {
      const uint32_t j = i + 1 + k + lane;
      const double cand = bi + wv;
      if (cand < best[j]) {
        best[j] = cand;
        from[j] = i;
      }
    }
    if (ni != i) __syncthreads();  // best[i + 1] is final once row i is done
  }
  __syncthreads();
}

// lane 0: the chain n - 1 -> 0 through from[], written forwards; the input itself when best[n - 1] is not finite
template <class BestPtr, class FromPtr>
__device__ __forceinline__ void field_simplify_backtrack(BestPtr best, FromPtr from, uint32_t n, uint32_t* __restrict__ kept,
                                                         FieldSimplifyRec* __restrict__ rec) {
  if (threadIdx.x != 0) return;
  const double cost = best[n - 1];
  if (!(cost < INFINITY)) {
    for (uint32_t v = 0; v < n; ++v) kept[v] = v;
    *rec = FieldSimplifyRec{1, n, INFINITY};
    return;
  }
  uint32_t len = 0;
  for (uint32_t v = n - 1; v != 0xffffffffu; v = from[v]) ++len;
  uint32_t at = len;
  for (uint32_t v = n - 1; v != 0xffffffffu; v = from[v]) kept[--at] = v;
  *rec = FieldSimplifyRec{0, len, cost};
}

// One wave per path.  kept: n entries per path at poff[q] (the first rec.kept are the answer).  gbest / gfrom: n entries
// per path at poff[q], read only by paths longer than FIELD_SIMPLIFY_LDS_STATES (may be nullptr when there is none).
__global__ void __launch_bounds__(64)
field_simplify_search_kernel(const unsigned long long* __restrict__ poff, const unsigned long long* __restrict__ coff,
                             unsigned long long window, const double* __restrict__ wts, double* __restrict__ gbest,
                             uint32_t* __restrict__ gfrom, uint32_t* __restrict__ kept, FieldSimplifyRec* __restrict__ recs) {
  __shared__ double s_best[FIELD_SIMPLIFY_LDS_STATES];
  __shared__ uint32_t s_from[FIELD_SIMPLIFY_LDS_STATES];
  const uint32_t q = blockIdx.x;
  const unsigned long long base = poff[q];
  const uint32_t n = (uint32_t)(poff[q + 1] - base);
  FieldSimplifyRec* rec = recs + q;
  if (n == 0) {
    if (threadIdx.x == 0) *rec = FieldSimplifyRec{2, 0, INFINITY};
    return;
  }
  const uint32_t m = n - 1;
  const uint32_t w = (window == 0 || window > m) ? m : (uint32_t)window;
  const double* wq = wts + coff[q];
  uint32_t* kq = kept + base;
  if (n <= FIELD_SIMPLIFY_LDS_STATES) {
    field_simplify_search(s_best, s_from, wq, n, w);
    field_simplify_backtrack(s_best, s_from, n, kq, rec);
  } else {
    field_simplify_search(gbest + base, gfrom + base, wq, n, w);
    field_simplify_backtrack(gbest + base, gfrom + base, n, kq, rec);
  }
}

// One lane per input state slot: slot t of path q carries kept state t of that path, if there is one.
__global__ void __launch_bounds__(256)
field_simplify_gather_kernel(const double* __restrict__ se3, const unsigned long long* __restrict__ poff, uint32_t n_paths,
                             const uint32_t* __restrict__ kept, const FieldSimplifyRec* __restrict__ recs,
                             const unsigned long long* __restrict__ ooff, size_t n_states, uint32_t* __restrict__ kept_out,
                             double* __restrict__ se3_out) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_states) return;
  const uint32_t q = field_simplify_path_of(poff, n_paths, g);
  const unsigned long long base = poff[q], t = g - base;
  if (t >= recs[q].kept) return;
  const uint32_t v = kept[g];
  const unsigned long long o = ooff[q] + t;
  kept_out[o] = v;
  const double* s = se3 + 7 * (base + v);
#pragma unroll
  for (int k = 0; k < 7; ++k) se3_out[7 * o + k] = s[k];
}

// kept counts of the paths as the scan's input (n_paths + 1 entries, the last 0)
__global__ void __launch_bounds__(256)
field_simplify_counts_kernel(const FieldSimplifyRec* __restrict__ recs, uint32_t n_paths, unsigned long long* __restrict__ cnt) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q <= n_paths) cnt[q] = q < n_paths ? recs[q].kept : 0ull;
}

}  // namespace artp

namespace {

// Layout of d_simplify for `paths` paths, `states` input states, `cands` candidates in all and `batch` a batch:
struct FieldSimplifyBuf {
  unsigned long long *poff, *coff, *kcnt, *ooff, *usable;  // path offsets, candidate offsets, kept counts, their scan
  artp::FieldSimplifyRec* recs;
  double *se3, *wts, *out_se3;     // the input states, one weight per candidate, the compact kept states
  uint32_t *kept, *out_kept;       // kept indices per path at its own offset; compact
  double* gbest;                   // the search's tables of paths too long for LDS (long_states entries, else none)
  uint32_t* gfrom;
  double *s1, *s2, *cost;          // a batch
  uint32_t* ninterp;
  uint8_t *ok_interp, *ok_motion;
};

size_t field_simplify_layout(char* base, size_t paths, size_t states, size_t cands, size_t batch, size_t long_states,
                             FieldSimplifyBuf* b) {
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* p = base + o;
    o += (bytes + 15) & ~(size_t)15;
    return p;
  };
  b->poff = reinterpret_cast<unsigned long long*>(take((paths + 1) * 8));
  b->coff = reinterpret_cast<unsigned long long*>(take((paths + 1) * 8));
  b->kcnt = reinterpret_cast<unsigned long long*>(take((paths + 1) * 8));
  b->ooff = reinterpret_cast<unsigned long long*>(take((paths + 1) * 8));
  b->usable = reinterpret_cast<unsigned long long*>(take(8));
  b->recs = reinterpret_cast<artp::FieldSimplifyRec*>(take(paths * sizeof(artp::FieldSimplifyRec)));
  b->se3 = reinterpret_cast<double*>(take(7 * states * 8));
  b->wts = reinterpret_cast<double*>(take(cands * 8));
  b->out_se3 = reinterpret_cast<double*>(take(7 * states * 8));
  b->kept = reinterpret_cast<uint32_t*>(take(states * 4));
  b->out_kept = reinterpret_cast<uint32_t*>(take(states * 4));
  b->gbest = reinterpret_cast<double*>(take(long_states * 8));
  b->gfrom = reinterpret_cast<uint32_t*>(take(long_states * 4));
  b->s1 = reinterpret_cast<double*>(take(7 * batch * 8));
  b->s2 = reinterpret_cast<double*>(take(7 * batch * 8));
  b->cost = reinterpret_cast<double*>(take(batch * 8));
  b->ninterp = reinterpret_cast<uint32_t*>(take(batch * 4));
  b->ok_interp = reinterpret_cast<uint8_t*>(take(batch));
  b->ok_motion = reinterpret_cast<uint8_t*>(take(batch));
  return o;
}

constexpr uint64_t FIELD_SIMPLIFY_BATCH = 1ull << 20;      // candidates a batch by default
constexpr uint64_t FIELD_SIMPLIFY_BATCH_MAX = 1ull << 30;  // run_edges_dev scans 32-bit counts

}  // namespace

extern "C" {

int artp_field_simplify_paths(artp_field* f, const artp_field_simplify_params* p, const double* se3_in, const uint64_t* offsets,
                              size_t n_paths, int32_t* statuses, double* costs, uint64_t* out_offsets, uint32_t* kept_out,
                              double* se3_out, size_t cap_states) {
  if (!f || !p || !offsets || !n_paths || !statuses || !costs || n_paths > (size_t)1 << 24) return ARTP_ERR_INVALID_ARG;
  artp_ctx* c = f->ctx;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  const auto h0 = std::chrono::steady_clock::now();
  for (size_t q = 0; q < n_paths; ++q)
    if (offsets[q + 1] < offsets[q]) {
      c->last_error = "artp_field_simplify_paths: offsets[" + std::to_string(q + 1) + "] lies below its predecessor (nothing is written)";
      return ARTP_ERR_INVALID_ARG;
    }
  const uint64_t first = offsets[0];
  const size_t n_states = (size_t)(offsets[n_paths] - first);
  if ((n_states && !se3_in) || n_states >= (size_t)0xffffffffu) {
    c->last_error = "artp_field_simplify_paths: no states, or 2^32 - 1 of them and more in one call";
    return ARTP_ERR_INVALID_ARG;
  }
  if (f->grid.objective == 2) {
    c->last_error = "artp_field_simplify_paths: a learned field is refused (segments are priced by objectives 0 and 1 only)";
    return ARTP_ERR_INVALID_ARG;
  }
  if (f->map_version != c->map_version.load()) {
    c->last_error = "artp_field_simplify_paths: the map changed since the field was computed";
    return ARTP_ERR_INVALID_ARG;
  }
  if (!c->have_field[0] || !c->have_field[1] || !c->have_z) {
    c->last_error = "artp_field_simplify_paths: checkMotion needs both validity layers and artp_set_z_bounds";
    return ARTP_ERR_NO_MAP;
  }
  // the pricing: the field's objective (a clearance-weighted field: its base objective, unweighted) and velocities
  artp_roadmap_params prm;
  artp_roadmap_params_defaults(&prm);
  prm.objective = f->params.objective;
  prm.max_lon_vel = f->params.max_lon_vel;
  prm.max_lat_vel = f->params.max_lat_vel;
  prm.max_ang_vel = f->params.max_ang_vel;

  std::vector<unsigned long long> poff(n_paths + 1), coff(n_paths + 1);
  size_t long_states = 0;
  unsigned long long n_cands = 0;
  for (size_t q = 0; q <= n_paths; ++q) {
    poff[q] = offsets[q] - first;
    coff[q] = n_cands;
    if (q < n_paths) {
      const unsigned long long n = offsets[q + 1] - offsets[q];
      n_cands += artp::field_simplify_count(n, p->window);
      if (n > artp::FIELD_SIMPLIFY_LDS_STATES) long_states = n_states;  // indexed like the states
    }
  }
  uint64_t batch = p->max_batch_pairs ? p->max_batch_pairs : FIELD_SIMPLIFY_BATCH;
  if (batch > FIELD_SIMPLIFY_BATCH_MAX) batch = FIELD_SIMPLIFY_BATCH_MAX;
  if (batch > n_cands) batch = n_cands;

  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->lane->stream;
  FieldSimplifyBuf B;
  const size_t need = field_simplify_layout(nullptr, n_paths, n_states, (size_t)n_cands, (size_t)batch, long_states, &B);
  if (f->simplify_cap < need) HIP_TRY(c, hipStreamSynchronize(st));
  ARTP_TRY(field_grow(f, &f->d_simplify, &f->simplify_cap, need));
  field_simplify_layout(f->d_simplify, n_paths, n_states, (size_t)n_cands, (size_t)batch, long_states, &B);

  artp_field_simplify_stats_t ss{};
  ss.paths = n_paths;
  ss.states_in = n_states;
  ss.candidates = n_cands;
  HIP_TRY(c, hipMemcpyAsync(B.poff, poff.data(), (n_paths + 1) * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(B.coff, coff.data(), (n_paths + 1) * 8, hipMemcpyHostToDevice, st));
  if (n_states) HIP_TRY(c, hipMemcpyAsync(B.se3, se3_in + 7 * first, 7 * n_states * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemsetAsync(B.usable, 0, 8, st));
  StreamTimer<3> tm(st);
  tm.mark(0);
  // 1. the candidates, a batch at a time: enumeration, the two checks, the cost, the weight
  DeviceScratch S;  // (the learned objective's temporaries of roadmap_eval_edges_into: none here)
  for (unsigned long long g0 = 0; g0 < n_cands; g0 += batch) {
    const size_t ne = (size_t)std::min<unsigned long long>(batch, n_cands - g0);
    const unsigned blocks = (unsigned)((ne + 255) / 256);
    hipLaunchKernelGGL(artp::field_simplify_pairs_kernel, dim3(blocks), dim3(256), 0, st, (const double*)B.se3,
                       (const unsigned long long*)B.poff, (const unsigned long long*)B.coff, (uint32_t)n_paths,
                       (unsigned long long)p->window, g0, ne, B.s1, B.s2);
    HIP_TRY(c, hipGetLastError());
    ARTP_TRY(roadmap_eval_edges_into(c, &prm, B.s1, B.s2, ne, B.ok_interp, B.ninterp, B.cost, &S));
    ARTP_TRY(run_edges_dev(c, 0, B.s1, B.s2, ne, B.ok_motion, nullptr));
    hipLaunchKernelGGL(artp::field_simplify_weight_kernel, dim3(blocks), dim3(256), 0, st, (const uint8_t*)B.ok_interp,
                       (const uint8_t*)B.ok_motion, (const double*)B.cost, ne, B.wts + g0, B.usable);
    HIP_TRY(c, hipGetLastError());
    ++ss.batches;
  }
  tm.mark(1);
  // 2. the search of every path, the scan of the kept counts, the compact output
  hipLaunchKernelGGL(artp::field_simplify_search_kernel, dim3((unsigned)n_paths), dim3(64), 0, st,
                     (const unsigned long long*)B.poff, (const unsigned long long*)B.coff, (unsigned long long)p->window,
                     (const double*)B.wts, long_states ? B.gbest : (double*)nullptr, long_states ? B.gfrom : (uint32_t*)nullptr,
                     B.kept, B.recs);
  HIP_TRY(c, hipGetLastError());
  hipLaunchKernelGGL(artp::field_simplify_counts_kernel, dim3((unsigned)((n_paths + 256) / 256)), dim3(256), 0, st,
                     (const artp::FieldSimplifyRec*)B.recs, (uint32_t)n_paths, B.kcnt);
  HIP_TRY(c, hipGetLastError());
  size_t cub = 0;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, cub, B.kcnt, B.ooff, (int)(n_paths + 1), st));
  ARTP_TRY(ensure_cub_tmp(c, cub));
  size_t cub_cap = c->lane->cub_tmp.capacity();
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(c->lane->cub_tmp.get(), cub_cap, B.kcnt, B.ooff, (int)(n_paths + 1), st));
  if (n_states) {
    hipLaunchKernelGGL(artp::field_simplify_gather_kernel, dim3((unsigned)((n_states + 255) / 256)), dim3(256), 0, st,
                       (const double*)B.se3, (const unsigned long long*)B.poff, (uint32_t)n_paths, (const uint32_t*)B.kept,
                       (const artp::FieldSimplifyRec*)B.recs, (const unsigned long long*)B.ooff, n_states, B.out_kept, B.out_se3);
    HIP_TRY(c, hipGetLastError());
  }
  tm.mark(2);
  // 3. the first read: statuses, costs and counts
  std::vector<artp::FieldSimplifyRec> recs(n_paths);
  unsigned long long usable = 0;
  HIP_TRY(c, hipMemcpyAsync(recs.data(), B.recs, n_paths * sizeof(artp::FieldSimplifyRec), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(&usable, B.usable, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  ARTP_TRY(check_error_flag(c));
  uint64_t total = 0;
  for (size_t q = 0; q < n_paths; ++q) {
    statuses[q] = recs[q].status;
    costs[q] = recs[q].cost;
    if (out_offsets) out_offsets[q] = total;
    total += recs[q].kept;
  }
  if (out_offsets) out_offsets[n_paths] = total;
  ss.states_kept = total;
  ss.usable_candidates = usable;
  ss.eval_ms = tm.ms(0, 1, true);
  ss.search_ms = tm.ms(1, 2, true);
  int rc = ARTP_OK;
  if (out_offsets && (kept_out || se3_out)) {
    if (total > cap_states) {
      c->last_error = "artp_field_simplify_paths: cap_states is smaller than out_offsets[n_paths]";
      rc = ARTP_ERR_CAPACITY;
    } else if (total) {
      // 4. the second read: the kept indices and states
      if (kept_out) HIP_TRY(c, hipMemcpyAsync(kept_out, B.out_kept, total * 4, hipMemcpyDeviceToHost, st));
      if (se3_out) HIP_TRY(c, hipMemcpyAsync(se3_out, B.out_se3, 7 * total * 8, hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
    }
  }
  ss.host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0).count();
  f->sstats = ss;
  return rc;
}

int artp_field_simplify_stats(artp_field* f, artp_field_simplify_stats_t* out) {
  if (!f || !out) return ARTP_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(f->ctx->mu);
  *out = f->sstats;
  return ARTP_OK;
}

}  // extern "C"
