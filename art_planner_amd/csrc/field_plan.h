// field_plan.h -- lazily checked paths on cost-to-go fields (include/artp_c.h artp_field_block_moves, _unblock, _blocked,
// _plan).
//
// A field may carry a BLOCKED-MOVE SET: one 16-bit word per node, bit j set = pull slot (v, j) is an absent edge (forward
// field: the edge u -> v with u the neighbour of v by offset j; reverse field: v -> u).  field.h's four readers of a pull
// cost skip a blocked slot through field_blocked_word.  Slot (v, j) is read by the rule of node v and by nobody else, and
// that rule runs in the tile that owns v: setting or clearing a bit flags that one tile in d_acc, and field_update_passes
// (unsupport, relax, hop reset, unsupport, relax) brings the field to the fixed point of the new edge set.
//   field_block_kernel     one lane per move a -> b: atomic OR of the bit into the owner's word, the owner's tile flagged,
//                          the bits that were clear counted
//   field_unblock_kernel   one lane per node of a sub-rectangle: the word cleared, its bits counted, its tile flagged
// artp_field_plan is the lazy loop on top of it (LazyPRM*'s: check what a path uses, remove what fails, repair, repeat).
// Per round: field_paths_kernel (one wave per pending target, field_path_kernel's descent) -> one read of the totals ->
// field_poses_kernel over all path nodes -> field_plan_pairs_kernel (the moves as (s1, s2) in travel order) -> checkMotion
// through run_edges_dev -> field_block_kernel over the failures -> one read of the verdict per target and the number of
// newly set bits -> field_update_passes when there was one.
#pragma once

namespace artp {

// slot of the move a -> b by move m from a: the owner node's index and the bit
__device__ __forceinline__ void field_move_slot(const FieldGrid& G, const int* a, const int* b, int m, size_t* owner, int* j) {
  const int* o = G.reverse ? a : b;
  *owner = ((size_t)o[0] + (size_t)o[1] * G.nrows) * G.n_yaw + o[2];
  *j = G.reverse ? m : field_back_move(m);
}

// Move i: a -> b with a = na + 3 q, b = nb + 3 q, q = idx ? idx[i] : i (artp_field_plan: nb = na + 3 and idx = the move's
// first state among the path nodes).  skip (may be nullptr): a move whose byte is non-zero passed its check and stays.
// Both ends inside the rectangle and one of the ten moves apart: checked by the host, or true by construction.
// cnt[7] += moves that were not blocked before; fail (may be nullptr): fail[tgt[i]] = 1 for every move that is blocked here.
__global__ void __launch_bounds__(256)
field_block_kernel(FieldGrid G, const int* __restrict__ na, const int* __restrict__ nb, const uint32_t* __restrict__ idx,
                   const uint8_t* __restrict__ skip, size_t n, uint32_t* __restrict__ blk32, unsigned* __restrict__ acc,
                   unsigned long long* __restrict__ cnt, const uint32_t* __restrict__ tgt, unsigned* __restrict__ fail) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || (skip && skip[i])) return;
  const size_t q = idx ? (size_t)idx[i] : i;
  const int* a = na + 3 * q;
  const int* b = nb + 3 * q;
  for (int m = 0; m < 10; ++m) {
    int nr, nc, nk;
    if (!field_neighbour(G, a[0], a[1], a[2], m, &nr, &nc, &nk) || nr != b[0] || nc != b[1] || nk != b[2]) continue;
    size_t owner;
    int j;
    field_move_slot(G, a, b, m, &owner, &j);
    const uint32_t bit = field_slot_bits(G, j) << ((owner & 1) * 16);  // both rotation slots at two headings: one move
    const uint32_t old = atomicOr(&blk32[owner >> 1], bit);
    if ((old & bit) != bit) atomicAdd(&cnt[7], 1ull);
    const int* o = G.reverse ? a : b;
    acc[o[0] / FIELD_T + (o[1] / FIELD_T) * G.tiles_r] = 1u;
    break;
  }
  if (fail) fail[tgt[i]] = 1u;
}

// one lane per node of sub; cnt[7] += moves unblocked (the twin rotation slots of two headings count once)
__global__ void __launch_bounds__(256)
field_unblock_kernel(FieldGrid G, FieldSub sub, uint16_t* __restrict__ blk, unsigned* __restrict__ acc,
                     unsigned long long* __restrict__ cnt) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)sub.nrows * sub.ncols * G.n_yaw) return;
  const size_t ci = i / (size_t)G.n_yaw;
  const int k = (int)(i - ci * G.n_yaw);
  const int r = sub.row0 + (int)(ci % (size_t)sub.nrows), c = sub.col0 + (int)(ci / (size_t)sub.nrows);
  const size_t node = ((size_t)r + (size_t)c * G.nrows) * G.n_yaw + k;
  const uint32_t w = blk[node];
  if (!w) return;
  blk[node] = 0;
  atomicAdd(&cnt[7], (unsigned long long)(G.n_yaw == 2 ? __popc(w & 0xffu) + ((w & 0x300u) ? 1 : 0) : __popc(w)));
  acc[r / FIELD_T + (c / FIELD_T) * G.tiles_r] = 1u;
}

// artp_field_plan's record of one target
struct FieldPlanRec {
  long long n;      // states of its path this round (0 = unreachable, -1 = no tight predecessor)
  long long off;    // its first state among the round's path nodes (valid when the round's total fits)
  long long moff;   // its first move among the round's moves
  double cost;      // dist[target]
};

// One wave per pending target (pend[blockIdx.x] = its index among the call's targets): field_path_kernel's head, room for
// the path taken from tot[0] (states) and tot[1] (moves) by one atomic each, then field_descend when the states fit into
// cap.  move_src[q] = the first state of move q, move_tgt[q] = the target it belongs to.
__global__ void __launch_bounds__(64)
field_paths_kernel(FieldGrid G, const uint32_t* __restrict__ mask, const float* __restrict__ h, const double* __restrict__ tab,
                   const uint16_t* __restrict__ blk, const double* __restrict__ dist, const uint32_t* __restrict__ hops,
                   const int* __restrict__ targets, const uint32_t* __restrict__ pend, long long cap, int* __restrict__ nodes,
                   uint32_t* __restrict__ move_src, uint32_t* __restrict__ move_tgt, FieldPlanRec* __restrict__ recs,
                   unsigned long long* __restrict__ tot) {
  const int lane = threadIdx.x;
  const uint32_t t = pend[blockIdx.x];
  const int r = targets[3 * t], c = targets[3 * t + 1], k = targets[3 * t + 2];
  const size_t node = ((size_t)r + (size_t)c * G.nrows) * G.n_yaw + k;
  const uint32_t hv = hops[node];
  const double dv = dist[node];
  if (hv == FIELD_NONE) {
    if (lane == 0) recs[t] = FieldPlanRec{0, 0, 0, dv};
    return;
  }
  const long long n = (long long)hv + 1;
  unsigned long long off = 0, moff = 0;
  if (lane == 0) {
    off = atomicAdd(&tot[0], (unsigned long long)n);
    moff = atomicAdd(&tot[1], (unsigned long long)(n - 1));
  }
  off = __shfl(off, 0);
  moff = __shfl(moff, 0);
  if (lane == 0) recs[t] = FieldPlanRec{n, (long long)off, (long long)moff, dv};
  // (the two atomics of different waves interleave: a wave's moves may lie further out than its states)
  if ((long long)off + n > cap || (long long)moff + n - 1 > cap) return;  // the host reads tot[0], grows the scratch, runs the round again
  for (long long q = lane; q < n - 1; q += 64) {
    move_src[moff + q] = (uint32_t)(off + q);
    move_tgt[moff + q] = t;
  }
  if (!field_descend(G, mask, h, tab, blk, dist, hops, r, c, k, hv, dv, nodes + 3 * off) && lane == 0) recs[t].n = -1;
}

// the moves as checkMotion's (s1, s2): the poses of state move_src[q] and of the one behind it
__global__ void __launch_bounds__(256)
field_plan_pairs_kernel(const double* __restrict__ se3, const uint32_t* __restrict__ move_src, size_t n_moves,
                        double* __restrict__ s1, double* __restrict__ s2) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_moves * 7) return;
  const size_t q = i / 7, j = i - q * 7;
  const size_t s = move_src[q];
  s1[i] = se3[7 * s + j];
  s2[i] = se3[7 * (s + 1) + j];
}

}  // namespace artp

namespace {

// the blocked words, zeroed, on the first block
int field_blocked_alloc(artp_field* f) {
  if (f->d_blk) return ARTP_OK;
  artp_ctx* c = f->ctx;
  const size_t words = (f->n_nodes + 1) / 2 * 2;  // whole 32-bit words
  HIP_TRY(c, f->mem.alloc(&f->d_blk, words));
  HIP_TRY(c, hipMemsetAsync(f->d_blk, 0, words * sizeof(uint16_t), c->lane->stream));
  return ARTP_OK;
}

// what artp_field_update's passes need, on a field of either kind
int field_plan_passes(artp_field* f, artp_field_update_stats_t* ps) {
  const int rc = field_update_passes(f, ps);
  if (rc) {
    (void)hipStreamSynchronize(f->ctx->lane->stream);
    return rc;
  }
  f->stats.reached_nodes = ps->reached_nodes;
  return ARTP_OK;
}

// Layout of d_plan for `targets` targets and `states` path states a round:
//   recs | totals[2] | fail flags | targets (3 ints) | pending list | nodes (3 ints a state) | move_src | move_tgt |
//   verdicts (1 byte a move, padded) | se3 (7 doubles a state) | s1 | s2 (7 doubles a move each)
struct FieldPlanBuf {
  artp::FieldPlanRec* recs;
  unsigned long long* tot;
  unsigned* fail;
  int* targets;
  uint32_t* pend;
  int* nodes;
  uint32_t *move_src, *move_tgt;
  uint8_t* valid;
  double *se3, *s1, *s2;
};

size_t field_plan_layout(char* base, size_t targets, size_t states, FieldPlanBuf* b) {
  size_t o = 0;
  auto take = [&](size_t bytes) {
    char* p = base + o;
    o += (bytes + 15) & ~(size_t)15;
    return p;
  };
  b->recs = reinterpret_cast<artp::FieldPlanRec*>(take(targets * sizeof(artp::FieldPlanRec)));
  b->tot = reinterpret_cast<unsigned long long*>(take(2 * sizeof(unsigned long long)));
  b->fail = reinterpret_cast<unsigned*>(take(targets * sizeof(unsigned)));
  b->targets = reinterpret_cast<int*>(take(3 * targets * sizeof(int)));
  b->pend = reinterpret_cast<uint32_t*>(take(targets * sizeof(uint32_t)));
  b->nodes = reinterpret_cast<int*>(take(3 * states * sizeof(int)));
  b->move_src = reinterpret_cast<uint32_t*>(take(states * sizeof(uint32_t)));
  b->move_tgt = reinterpret_cast<uint32_t*>(take(states * sizeof(uint32_t)));
  b->valid = reinterpret_cast<uint8_t*>(take(states));
  b->se3 = reinterpret_cast<double*>(take(7 * states * sizeof(double)));
  b->s1 = reinterpret_cast<double*>(take(7 * states * sizeof(double)));
  b->s2 = reinterpret_cast<double*>(take(7 * states * sizeof(double)));
  return o;
}

int field_plan_scratch(artp_field* f, size_t targets, size_t states, FieldPlanBuf* b) {
  artp_ctx* c = f->ctx;
  if (f->plan_targets < targets || f->plan_states < states) {
    if (targets < f->plan_targets) targets = f->plan_targets;
    if (states < f->plan_states) states = f->plan_states;
    HIP_TRY(c, hipStreamSynchronize(c->lane->stream));
    f->mem.release(f->d_plan);
    f->d_plan = nullptr;
    f->plan_targets = f->plan_states = 0;
    FieldPlanBuf tmp;
    HIP_TRY(c, f->mem.alloc(&f->d_plan, field_plan_layout(nullptr, targets, states, &tmp)));
    f->plan_targets = targets;
    f->plan_states = states;
  }
  field_plan_layout(static_cast<char*>(f->d_plan), f->plan_targets, f->plan_states, b);
  return ARTP_OK;
}

}  // namespace

extern "C" {

int artp_field_block_moves(artp_field* f, const int* a, const int* b, size_t n, uint64_t* newly_blocked) {
  if (newly_blocked) *newly_blocked = 0;
  if (!f || (n && (!a || !b))) return ARTP_ERR_INVALID_ARG;
  if (!n) return ARTP_OK;
  artp_ctx* c = f->ctx;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  const artp::FieldGrid& G = f->grid;
  for (size_t i = 0; i < n; ++i) {  // nothing is written before every pair has passed
    const int *p = a + 3 * i, *q = b + 3 * i;
    bool ok = p[0] >= 0 && p[0] < G.nrows && p[1] >= 0 && p[1] < G.ncols && p[2] >= 0 && p[2] < G.n_yaw && q[0] >= 0 &&
              q[0] < G.nrows && q[1] >= 0 && q[1] < G.ncols && q[2] >= 0 && q[2] < G.n_yaw;
    if (ok) {
      const int dr = q[0] - p[0], dc = q[1] - p[1], dk = ((q[2] - p[2]) % G.n_yaw + G.n_yaw) % G.n_yaw;
      const bool trans = dk == 0 && (dr || dc) && dr >= -1 && dr <= 1 && dc >= -1 && dc <= 1;
      const bool rot = dr == 0 && dc == 0 && G.n_yaw > 1 && (dk == 1 || dk == G.n_yaw - 1);
      ok = trans || rot;
    }
    if (!ok) {
      c->last_error = "artp_field_block_moves: pair " + std::to_string(i) +
                      " is not one of the ten moves between two nodes of the rectangle (the field is unchanged)";
      return ARTP_ERR_INVALID_ARG;
    }
  }
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->lane->stream;
  int rc = field_update_scratch(f, false);
  if (rc) return rc;
  rc = field_blocked_alloc(f);
  if (rc) return rc;
  rc = field_ensure_scratch(f, 6 * n, 8);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(f->d_nodes, a, 3 * n * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(f->d_nodes + 3 * n, b, 3 * n * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemsetAsync(f->d_acc, 0, f->n_tiles * sizeof(unsigned), st));
  HIP_TRY(c, hipMemsetAsync(f->d_ucnt, 0, 8 * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(artp::field_block_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, G, (const int*)f->d_nodes,
                     (const int*)(f->d_nodes + 3 * n), (const uint32_t*)nullptr, (const uint8_t*)nullptr, n,
                     reinterpret_cast<uint32_t*>(f->d_blk), f->d_acc, f->d_ucnt, (const uint32_t*)nullptr, (unsigned*)nullptr);
  HIP_TRY(c, hipGetLastError());
  unsigned long long newly = 0;
  HIP_TRY(c, hipMemcpyAsync(&newly, f->d_ucnt + 7, sizeof(newly), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));  // the host copies of a and b are free from here
  f->n_blocked += newly;
  if (newly_blocked) *newly_blocked = newly;
  if (!newly) return ARTP_OK;
  artp_field_update_stats_t ps{};
  return field_plan_passes(f, &ps);
}

int artp_field_unblock(artp_field* f, const int* sub_rect, uint64_t* unblocked) {
  if (unblocked) *unblocked = 0;
  if (!f) return ARTP_ERR_INVALID_ARG;
  artp_ctx* c = f->ctx;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  const artp::FieldGrid& G = f->grid;
  artp::FieldSub sub;
  ARTP_TRY(field_sub_rect(f, "artp_field_unblock", sub_rect, &sub));
  if (!f->d_blk || !f->n_blocked) return ARTP_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->lane->stream;
  int rc = field_update_scratch(f, false);
  if (rc) return rc;
  HIP_TRY(c, hipMemsetAsync(f->d_acc, 0, f->n_tiles * sizeof(unsigned), st));
  HIP_TRY(c, hipMemsetAsync(f->d_ucnt, 0, 8 * sizeof(unsigned long long), st));
  const size_t n = (size_t)sub.nrows * sub.ncols * G.n_yaw;
  hipLaunchKernelGGL(artp::field_unblock_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, G, sub, f->d_blk, f->d_acc,
                     f->d_ucnt);
  HIP_TRY(c, hipGetLastError());
  unsigned long long cleared = 0;
  HIP_TRY(c, hipMemcpyAsync(&cleared, f->d_ucnt + 7, sizeof(cleared), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  f->n_blocked -= cleared;
  if (unblocked) *unblocked = cleared;
  if (!cleared) return ARTP_OK;
  artp_field_update_stats_t ps{};
  return field_plan_passes(f, &ps);
}

int artp_field_blocked_count(artp_field* f, uint64_t* n) {
  if (!f || !n) return ARTP_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(f->ctx->mu);
  *n = f->n_blocked;
  return ARTP_OK;
}

int artp_field_blocked(artp_field* f, uint16_t* words_out) {
  if (!f || !words_out) return ARTP_ERR_INVALID_ARG;
  artp_ctx* c = f->ctx;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  if (!f->d_blk) {
    std::memset(words_out, 0, f->n_nodes * sizeof(uint16_t));
    return ARTP_OK;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(words_out, f->d_blk, f->n_nodes * sizeof(uint16_t), hipMemcpyDeviceToHost, c->lane->stream));
  HIP_TRY(c, hipStreamSynchronize(c->lane->stream));
  return ARTP_OK;
}

int artp_field_plan(artp_field* f, const int* targets, size_t n_targets, int max_rounds, int32_t* statuses, double* costs,
                    uint64_t* path_offsets, int* nodes_out, double* se3_out, size_t cap_states) {
  if (!f || !targets || !n_targets || !statuses || !costs || max_rounds < 1 || n_targets > (size_t)1 << 24)
    return ARTP_ERR_INVALID_ARG;
  artp_ctx* c = f->ctx;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  const artp::FieldGrid& G = f->grid;
  for (size_t i = 0; i < n_targets; ++i) {
    const int* t = targets + 3 * i;
    if (t[0] < 0 || t[0] >= G.nrows || t[1] < 0 || t[1] >= G.ncols || t[2] < 0 || t[2] >= G.n_yaw) {
      c->last_error = "artp_field_plan: a target lies outside the rectangle or its heading outside [0, n_yaw)";
      return ARTP_ERR_INVALID_ARG;
    }
  }
  if (f->map_version != c->map_version.load()) {
    c->last_error = "artp_field_plan: the map changed since the field was computed (its poses are gone)";
    return ARTP_ERR_INVALID_ARG;
  }
  if (!c->have_field[0] || !c->have_field[1] || !c->have_z) {
    c->last_error = "artp_field_plan: checkMotion needs both validity layers and artp_set_z_bounds";
    return ARTP_ERR_NO_MAP;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->lane->stream;
  int rc = field_update_scratch(f, false);
  if (rc) return rc;
  rc = field_blocked_alloc(f);
  if (rc) return rc;
  FieldPlanBuf B;
  rc = field_plan_scratch(f, n_targets, std::max<size_t>(f->plan_states, 64 * n_targets), &B);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(B.targets, targets, 3 * n_targets * sizeof(int), hipMemcpyHostToDevice, st));

  artp_field_plan_stats_t ps{};
  f->plan_round_runs.clear();
  std::vector<uint32_t> pending(n_targets);
  for (size_t i = 0; i < n_targets; ++i) pending[i] = (uint32_t)i;
  std::vector<std::vector<int>> done_nodes(n_targets);
  std::vector<std::vector<double>> done_se3(n_targets);
  std::vector<artp::FieldPlanRec> recs(n_targets);
  std::vector<unsigned> fail(n_targets);
  for (size_t i = 0; i < n_targets; ++i) {
    statuses[i] = 2;
    costs[i] = INFINITY;
  }
  StreamTimer<3> tm(st);  // the stream time of a round's descent and of its check
  while (!pending.empty() && ps.rounds < (uint64_t)max_rounds) {
    const size_t np = pending.size();
    const auto h0 = std::chrono::steady_clock::now();
    tm.mark(0);
    // 1. the descents; run again with more room when the states did not fit
    unsigned long long tot[2] = {0, 0};
    for (;;) {
      HIP_TRY(c, hipMemcpyAsync(B.pend, pending.data(), np * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      HIP_TRY(c, hipMemsetAsync(B.tot, 0, 2 * sizeof(unsigned long long), st));
      HIP_TRY(c, hipMemsetAsync(B.fail, 0, n_targets * sizeof(unsigned), st));
      hipLaunchKernelGGL(artp::field_paths_kernel, dim3((unsigned)np), dim3(64), 0, st, G, (const uint32_t*)f->d_mask,
                         (const float*)f->d_h, (const double*)f->d_tab, (const uint16_t*)f->d_blk, (const double*)f->d_dist,
                         (const uint32_t*)f->d_hops, (const int*)B.targets, (const uint32_t*)B.pend, (long long)f->plan_states,
                         B.nodes, B.move_src, B.move_tgt, B.recs, B.tot);
      HIP_TRY(c, hipGetLastError());
      tm.mark(1);
      HIP_TRY(c, hipMemcpyAsync(tot, B.tot, sizeof(tot), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipMemcpyAsync(recs.data(), B.recs, n_targets * sizeof(artp::FieldPlanRec), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      if (tot[0] <= f->plan_states) break;
      rc = field_plan_scratch(f, n_targets, (size_t)tot[0] + (size_t)tot[0] / 2, &B);
      if (rc) return rc;
      HIP_TRY(c, hipMemcpyAsync(B.targets, targets, 3 * n_targets * sizeof(int), hipMemcpyHostToDevice, st));
    }
    for (uint32_t t : pending)
      if (recs[t].n < 0) {
        c->last_error = "artp_field_plan: no tight predecessor (the field is not at its fixed point)";
        return ARTP_ERR_HIP;
      }
    ++ps.rounds;
    const size_t n_states = (size_t)tot[0], n_moves = (size_t)tot[1];
    unsigned long long newly = 0;
    // 2. - 4. poses, pairs, checkMotion, the failures blocked
    if (n_states) {
      hipLaunchKernelGGL(artp::field_poses_kernel, dim3((unsigned)((n_states + 255) / 256)), dim3(256), 0, st, f->sampler, f->geom,
                         f->rect, (const int*)B.nodes, n_states, B.se3);
      HIP_TRY(c, hipGetLastError());
    }
    if (n_moves) {
      hipLaunchKernelGGL(artp::field_plan_pairs_kernel, dim3((unsigned)((7 * n_moves + 255) / 256)), dim3(256), 0, st,
                         (const double*)B.se3, (const uint32_t*)B.move_src, n_moves, B.s1, B.s2);
      HIP_TRY(c, hipGetLastError());
      rc = run_edges_dev(c, 0, B.s1, B.s2, n_moves, B.valid, nullptr);
      if (rc) return rc;
      HIP_TRY(c, hipMemsetAsync(f->d_acc, 0, f->n_tiles * sizeof(unsigned), st));
      HIP_TRY(c, hipMemsetAsync(f->d_ucnt, 0, 8 * sizeof(unsigned long long), st));
      hipLaunchKernelGGL(artp::field_block_kernel, dim3((unsigned)((n_moves + 255) / 256)), dim3(256), 0, st, G,
                         (const int*)B.nodes, (const int*)(B.nodes + 3), (const uint32_t*)B.move_src, (const uint8_t*)B.valid,
                         n_moves, reinterpret_cast<uint32_t*>(f->d_blk), f->d_acc, f->d_ucnt, (const uint32_t*)B.move_tgt, B.fail);
      HIP_TRY(c, hipGetLastError());
      tm.mark(2);
      HIP_TRY(c, hipMemcpyAsync(&newly, f->d_ucnt + 7, sizeof(newly), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipMemcpyAsync(fail.data(), B.fail, n_targets * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    } else {
      tm.mark(2);
      std::fill(fail.begin(), fail.end(), 0u);
    }
    HIP_TRY(c, hipStreamSynchronize(st));
    ps.moves_checked += n_moves;
    ps.moves_blocked += newly;
    f->n_blocked += newly;
    // 5. the targets that are finished: unreachable, or a path without a failing move (this round's path stays)
    std::vector<uint32_t> next;
    for (uint32_t t : pending) {
      const artp::FieldPlanRec& r = recs[t];
      if (r.n == 0) {
        statuses[t] = 1;
      } else if (!fail[t]) {
        statuses[t] = 0;
        costs[t] = r.cost;
        done_nodes[t].resize(3 * (size_t)r.n);
        done_se3[t].resize(7 * (size_t)r.n);
        HIP_TRY(c, hipMemcpyAsync(done_nodes[t].data(), B.nodes + 3 * r.off, 3 * (size_t)r.n * sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(done_se3[t].data(), B.se3 + 7 * r.off, 7 * (size_t)r.n * sizeof(double), hipMemcpyDeviceToHost, st));
      } else {
        next.push_back(t);
      }
    }
    HIP_TRY(c, hipStreamSynchronize(st));
    ps.descent_ms += tm.ms(0, 1, true);
    ps.check_ms += tm.ms(1, 2, true);
    const auto h1 = std::chrono::steady_clock::now();
    ps.round_ms += std::chrono::duration<double, std::milli>(h1 - h0).count();
    pending.swap(next);
    f->plan_round_runs.push_back(0);
    // 6. the field repaired once
    if (newly) {
      artp_field_update_stats_t us{};
      rc = field_plan_passes(f, &us);
      if (rc) return rc;
      ps.update_tile_runs += us.tile_launches;
      ps.last_update_tile_runs = us.tile_launches;
      f->plan_round_runs.back() = us.tile_launches;
      ++ps.updates;
      ps.passes_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h1).count();
    }
  }
  f->pstats = ps;
  uint64_t total = 0;
  for (size_t i = 0; i < n_targets; ++i) {
    if (path_offsets) path_offsets[i] = total;
    total += done_nodes[i].size() / 3;
  }
  if (path_offsets) path_offsets[n_targets] = total;
  if (!path_offsets || (!nodes_out && !se3_out)) return ARTP_OK;
  if (total > cap_states) {
    c->last_error = "artp_field_plan: cap_states is smaller than path_offsets[n_targets]";
    return ARTP_ERR_CAPACITY;
  }
  for (size_t i = 0; i < n_targets; ++i) {
    if (nodes_out && !done_nodes[i].empty())
      std::memcpy(nodes_out + 3 * path_offsets[i], done_nodes[i].data(), done_nodes[i].size() * sizeof(int));
    if (se3_out && !done_se3[i].empty())
      std::memcpy(se3_out + 7 * path_offsets[i], done_se3[i].data(), done_se3[i].size() * sizeof(double));
  }
  return ARTP_OK;
}

int artp_field_plan_round_tile_runs(artp_field* f, uint64_t* runs_out, size_t cap, size_t* n_rounds) {
  if (!f || !n_rounds || (cap && !runs_out)) return ARTP_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(f->ctx->mu);
  *n_rounds = f->plan_round_runs.size();
  for (size_t i = 0; i < cap && i < f->plan_round_runs.size(); ++i) runs_out[i] = f->plan_round_runs[i];
  return ARTP_OK;
}

int artp_field_plan_stats(artp_field* f, artp_field_plan_stats_t* out) {
  if (!f || !out) return ARTP_ERR_INVALID_ARG;
  *out = f->pstats;
  return ARTP_OK;
}

}  // extern "C"
