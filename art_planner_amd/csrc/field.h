// field.h -- cost-to-go fields: shortest lattice costs from a set of source poses to every cell and heading of a
// rectangle of the map (include/artp_c.h artp_field_*, DESIGN.md sections 12 and 13).
//
// Node (r, c, k) exists iff bit k of mask[r + c nrows] is set; node index = (r + c nrows) n_yaw + k, the pose order of
// reach.h.  Ten moves per node (eight neighbouring cells at the same heading, two rotations).  dist[] is the least fixed
// point of dist[v] = min(dist[u] + w(u, v)) with dist[source] = 0: fl(+) is monotone and the weights are non-negative, so
// that fixed point is unique and does not depend on the order of the relaxations -- every kernel here works IN PLACE and
// reads neighbours that other lanes or workgroups may be changing at the same time (an aligned 8-byte load or store is
// not torn; any value read is the cost of a real path, so it can only delay the fixed point, never miss it).
//
// Four rules decide what happens to one node, given its live neighbours u over the ten moves (PHASE 0 works on
// distances, PHASE 1 on hop counts at settled distances):
//   relax, PHASE 0      dist[v] = min(dist[v], dist[u] + w)
//   relax, PHASE 1      hops[v] = the fewest tight edges (dist[u] + w == dist[v] bit for bit) from a source, the rule of
//                       roadmap_many_hops_kernel.  Objective 0's rotations cost 0, so "tight" holds both ways there; a
//                       predecessor one hop closer cannot close a cycle.
//   unsupport, PHASE 0  a live node stays iff it is a source (the nodes at 0 hops) or some u has dist[u] + w == dist[v]
//                       AND hops[u] + 1 == hops[v]; the others go back to +inf / NONE.  "Dead" is that value itself,
//                       and dying only spreads, so a stale neighbour read delays a death, never prevents it.
//   unsupport, PHASE 1  the same test at the settled distances; only the hop count dies (NONE)
// Each rule is written twice, once per form, and nothing else is:
//   plain form   field_plain_kernel<PHASE> / field_unsupport_plain_kernel<PHASE>: one lane per node, neighbours in
//                global memory through field_walk; one launch per sweep and a device counter of the waves that changed
//                something: the stepping stone and the timing yardstick
//   tiled form   field_tile_kernel<PHASE, UNSUP>, the tile skeleton: a workgroup owns 16 x 16 cells x all headings.
//                dist of the tile plus a one-cell halo, the table, the mask words, the heights and (all rules but
//                relax PHASE 0) the hop counts go to LDS, heading-major planes so that the lanes of a wave read
//                neighbouring words.  One lane per cell applies field_tile_rule to its headings (neighbours in LDS
//                through field_tile_walk) until nothing changes or inner_sweeps are spent; the tile writes its own
//                cells back (plain vector stores; the halo is read-only), flags the neighbouring tiles whose halo it
//                changed for the next launch, and itself when it ran out of sweeps.  A launch covers every tile; the
//                ones nobody flagged leave at once.  The skeleton's body is one function, field_tile_body, of the tile
//                index and the per-field pointers; field_tile_many_kernel<PHASE, LEARNED> runs it (relax, (m, k) table) on a grid of
//                (tiles, fields) for a batch of fields that share mask, heights and table (field_many.h, DESIGN.md
//                section 23); with LEARNED it runs on the ONE streamed weight table of a batch of learned or
//                clearance-weighted fields.
// field_rounds is the host loop of both forms: launch, read the counters, stop when nothing was flagged, refuse after
// n_nodes + 2 rounds.  No launch waits for another workgroup and no kernel stays resident.
//
// artp_field_compute: relax PHASE 0 from the sources' tiles, then relax PHASE 1.  field_path_kernel: one wave walks from
// the target to a source (field_descend): lane m tests move m, the first tight one that is one hop closer wins.
// Every reader of a pull cost skips the slots of the field's blocked-move set (field_blocked_word; field_plan.h and
// DESIGN.md section 16), when the field has one.
// artp_field_update brings a computed field to the fixed point of an edited mask in place:
//   field_update_sources_kernel / field_diff_kernel   refuse a removed source; install the changed words (and heights),
//                       clear the removed nodes, flag the tiles around every changed cell
//   unsupport PHASE 0, relax PHASE 0 from the flagged tiles
//   field_hop_reset_kernel   hops = NONE where dist differs from the snapshot taken before
//   unsupport PHASE 1, relax PHASE 1 from the flagged tiles
//
// artp_field_compute_learned: objective 2, the motion-cost network.  The cost of a move depends on
// the start cell's features and on both poses, so it sits in neither the (m, k) table nor eight registers: a per-field
// table in global memory holds one f64 pull weight per (node, offset), tile-major (field_wtab_index), filled once per
// call by field_learned_rows_kernel -> the context's cost query -> field_learned_combine_kernel in chunks of at most
// FIELD_LEARNED_CHUNK rows.  The rules are the same ones; only the cost source differs (field_walk's branch, the LEARNED
// parameter of the tile skeleton).  w(a -> b) != w(b -> a) here, rotations included.
// artp_field_update_learned: the diff of artp_field_update, then every slot of the table priced
// again against the context's current network and feature map (field_learned_reprice_kernel: a slot whose bits change is
// written and flags its tile), then the same four passes, the tiled ones on the streamed table.
// artp_field_compute_clearance (clearance.h): objective id 3 inside the library.  The weights are the
// base objective's (0 or 1) inflated near obstacles; they sit in the same table, filled by one kernel without the cost query,
// and the same table-driven kernels search it (field_has_wtab).  A mask edit moves clearances, and with them weights, up to
// radius_cells around it: artp_field_update and artp_field_update_learned refuse such a field, artp_field_update_clearance
// (clearance.h) recomputes both on a window of tiles and runs the passes of artp_field_update.
// artp_field_shift: the map moved by whole cells under the rectangle.  field_shift_nodes_kernel and
// field_shift_cells_kernel move dist, hops, blocked words, mask words and heights by a constant offset, fill the cells that
// entered and flag the border through which cells left; then the diff against the whole new mask and the four passes.
// The host side of the updates and the shift is one procedure, field_update_run; an entry point adds its refusals and its own step.
#pragma once

#include <cstddef>
#include <deque>

namespace artp {

constexpr int FIELD_T = 16;                            // tile edge in cells
constexpr int FIELD_HP = FIELD_T + 2;                  // with the halo
constexpr int FIELD_PLANE = FIELD_HP * FIELD_HP;       // cells of a heading plane in LDS
constexpr int FIELD_TAB = 8 * 32 + 8;                  // objective 1: w[m][k]; then (dx^2 + dy^2)[m] for objective 0
constexpr uint32_t FIELD_NONE = 0xffffffffu;

struct FieldGrid {
  int nrows, ncols, n_yaw;
  int tiles_r, tiles_c;
  int objective, reverse;
  uint32_t yaw_bits;  // the low n_yaw bits
  double vlon;        // max_lon_vel
  double wrot;        // cost of a rotation move
};

__host__ __device__ constexpr int field_dr(int m) { return m < 3 ? -1 : (m < 5 ? 0 : 1); }
__host__ __device__ constexpr int field_dc(int m) { return (m == 0 || m == 3 || m == 5) ? -1 : ((m == 1 || m == 6) ? 0 : 1); }

// Objective 2's weight table: slot (v, j) = the weight of the edge the rules pull along at node v = (r, c, k) from its
// neighbour u by offset j (forward: w(u -> v), reverse: w(v -> u)); +inf where that edge does not exist.  Tile-major,
// [tile][k][j][lane] with lane = the cell inside the tile as field_tile_kernel numbers its lanes, edge tiles padded: the
// 64 lanes of a wave read 64 consecutive doubles for one (k, j).
constexpr size_t FIELD_LEARNED_CHUNK = size_t(1) << 22;  // rows of the cost query per chunk (scratch: 36 bytes a row)
__host__ __device__ inline size_t field_wtab_index(const FieldGrid& G, int r, int c, int k, int j) {
  const size_t tile = (size_t)(r / FIELD_T) + (size_t)(c / FIELD_T) * (size_t)G.tiles_r;
  return ((tile * (size_t)G.n_yaw + (size_t)k) * 10 + (size_t)j) * (FIELD_T * FIELD_T) + (size_t)((r % FIELD_T) + (c % FIELD_T) * FIELD_T);
}
__host__ __device__ inline size_t field_wtab_slots(const FieldGrid& G) {
  return (size_t)G.tiles_r * G.tiles_c * (size_t)G.n_yaw * 10 * (FIELD_T * FIELD_T);
}

// Objectives 2 (learned) and 3 (clearance-weighted, clearance.h): the pull weights sit in the per-field table.
__host__ __device__ inline bool field_has_wtab(const FieldGrid& G) { return G.objective >= 2; }

// cost of translation move m (0..7) from a cell of height ha to one of height hb at heading k; tab in LDS or global
__device__ __forceinline__ double field_move_cost(const FieldGrid& G, const double* tab, int m, int k, float ha, float hb) {
  if (G.objective == 0) {
    const double dz = (double)hb - (double)ha;
    return sqrt(tab[8 * 32 + m] + dz * dz) / G.vlon;
  }
  return tab[m * 32 + k];
}

// The edge between node v and its neighbour by move j that the rules pull along: forward fields use the move
// neighbour -> v (move 7 - j seen from the neighbour), reverse fields the move v -> neighbour (move j); a rotation (8, 9)
// costs the same both ways.
__device__ __forceinline__ double field_pull_cost(const FieldGrid& G, const double* tab, int j, int k, float hv, float hn) {
  if (j >= 8) return G.wrot;
  return G.reverse ? field_move_cost(G, tab, j, k, hv, hn) : field_move_cost(G, tab, 7 - j, k, hn, hv);
}

__global__ void __launch_bounds__(256)
field_heights_kernel(SamplerDev sm, MapGeom g, ReachRect rc, float* __restrict__ h) {
  const uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= (uint32_t)rc.nrows * (uint32_t)rc.ncols) return;
  const int row = rc.row0 + (int)(cell % (uint32_t)rc.nrows);
  const int col = rc.col0 + (int)(cell / (uint32_t)rc.nrows);
  h[cell] = sm.cells[2 * ((size_t)row + (size_t)col * g.rows)].x;
}

__global__ void __launch_bounds__(256)
field_init_kernel(size_t n, double* __restrict__ dist, uint32_t* __restrict__ hops) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  dist[i] = INFINITY;
  hops[i] = FIELD_NONE;
}

// one lane per source: not a node of the mask -> *bad; else dist = 0, hops = 0
__global__ void __launch_bounds__(64)
field_sources_kernel(FieldGrid G, const uint32_t* __restrict__ mask, const int* __restrict__ src, int n_src,
                     double* __restrict__ dist, uint32_t* __restrict__ hops, unsigned* __restrict__ bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_src) return;
  const int r = src[3 * i], c = src[3 * i + 1], k = src[3 * i + 2];  // inside the rectangle: checked by the host
  const size_t cell = (size_t)r + (size_t)c * G.nrows;
  if (!((mask[cell] >> k) & 1u)) {
    atomicAdd(bad, 1u);
    return;
  }
  dist[cell * G.n_yaw + k] = 0.0;
  hops[cell * G.n_yaw + k] = 0u;
}

// The first round's work: the tiles of the sources and the tiles around them (a source in a tile's border row is in
// its neighbour's halo, and no tile "changed" it).
__global__ void __launch_bounds__(64)
field_seed_tiles_kernel(FieldGrid G, const int* __restrict__ src, int n_src, unsigned* __restrict__ active) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_src) return;
  const int ti = src[3 * i] / FIELD_T, tj = src[3 * i + 1] / FIELD_T;
  for (int dj = -1; dj <= 1; ++dj)
    for (int di = -1; di <= 1; ++di)
      if (ti + di >= 0 && ti + di < G.tiles_r && tj + dj >= 0 && tj + dj < G.tiles_c)
        active[(ti + di) + (tj + dj) * G.tiles_r] = 1u;
}

// neighbour of (r, c, k) by move m (0..9); false when it leaves the rectangle (or n_yaw == 1 for a rotation)
__device__ __forceinline__ bool field_neighbour(const FieldGrid& G, int r, int c, int k, int m, int* nr, int* nc, int* nk) {
  if (m < 8) {
    *nr = r + field_dr(m);
    *nc = c + field_dc(m);
    *nk = k;
    return *nr >= 0 && *nr < G.nrows && *nc >= 0 && *nc < G.ncols;
  }
  *nr = r;
  *nc = c;
  *nk = m == 8 ? (k + 1 == G.n_yaw ? 0 : k + 1) : (k == 0 ? G.n_yaw - 1 : k - 1);
  return G.n_yaw > 1;
}

// the move that leads back: b = a's neighbour by move m  <=>  a = b's neighbour by move field_back_move(m)
__host__ __device__ constexpr int field_back_move(int m) { return m < 8 ? 7 - m : (m == 8 ? 9 : 8); }

// The blocked-move set of a field (field_plan.h): one 16-bit word per node, bit j set = pull slot
// (v, j) is blocked, an absent edge.  blk == nullptr: the field never blocked anything.  Every reader of a pull cost goes
// through this one function and skips the slots whose bit is set.
__device__ __forceinline__ uint32_t field_blocked_word(const uint16_t* __restrict__ blk, size_t node) {
  return blk ? (uint32_t)blk[node] : 0u;
}
// The bits of pull slot j.  At two headings moves 8 and 9 lead to the same neighbour: one directed rotation sits in both
// slots of its owner, and the two bits are set, tested and counted as one.
__device__ __forceinline__ uint32_t field_slot_bits(const FieldGrid& G, int j) {
  return (G.n_yaw == 2 && j >= 8) ? 0x300u : 1u << j;
}

// The live neighbours of node (cell, k) over the ten moves, for the kernels with one lane per node: visit(ni, w) with ni
// the neighbour's node index (its cell and heading) and w() the pull cost of that move, computed when a rule asks
// (objectives 2 and 3: read from the weight table, which `tab` then is).
template <class F>
__device__ __forceinline__ void field_walk(const FieldGrid& G, const uint32_t* __restrict__ mask, const float* __restrict__ h,
                                           const double* __restrict__ tab, const uint16_t* __restrict__ blk, uint32_t cell,
                                           int k, F&& visit) {
  const int r = (int)(cell % (uint32_t)G.nrows), c = (int)(cell / (uint32_t)G.nrows);
  const uint32_t bw = field_blocked_word(blk, (size_t)cell * G.n_yaw + k);
#pragma unroll
  for (int m = 0; m < 10; ++m) {
    int nr, nc, nk;
    if (((bw >> m) & 1u) || !field_neighbour(G, r, c, k, m, &nr, &nc, &nk)) continue;
    const uint32_t ncell = m < 8 ? (uint32_t)nr + (uint32_t)nc * (uint32_t)G.nrows : cell;  // a rotation: the node's own word
    if (!((mask[ncell] >> nk) & 1u)) continue;
    visit((size_t)ncell * G.n_yaw + nk, [&]() {
      return field_has_wtab(G) ? tab[field_wtab_index(G, r, c, k, m)] : field_pull_cost(G, tab, m, k, h[cell], h[ncell]);
    });
  }
}

template <int PHASE>
__global__ void __launch_bounds__(256)
field_plain_kernel(FieldGrid G, const uint32_t* __restrict__ mask, const float* __restrict__ h,
                   const double* __restrict__ tab, const uint16_t* __restrict__ blk, double* dist, uint32_t* hops,
                   unsigned* __restrict__ changed) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n = (size_t)G.nrows * G.ncols * G.n_yaw;
  bool ch = false;
  if (i < n) {
    const uint32_t cell = (uint32_t)(i / (uint32_t)G.n_yaw);
    const int k = (int)(i - (size_t)cell * G.n_yaw);
    if ((mask[cell] >> k) & 1u) {
      const double old = dist[i];
      if (PHASE == 0) {
        double best = old;
        field_walk(G, mask, h, tab, blk, cell, k, [&](size_t ni, auto&& w) {
          const double du = dist[ni];
          if (!(du < best)) return;  // w >= 0: no candidate below du
          const double cand = du + w();
          if (cand < best) best = cand;
        });
        if (best < old) {
          dist[i] = best;
          ch = true;
        }
      } else if (old < INFINITY) {
        const uint32_t hold = hops[i];
        uint32_t hb = hold;
        field_walk(G, mask, h, tab, blk, cell, k, [&](size_t ni, auto&& w) {
          const uint32_t hu = hops[ni];
          if (hu == FIELD_NONE || hu + 1u >= hb) return;
          if (dist[ni] + w() == old) hb = hu + 1u;
        });
        if (hb < hold) {
          hops[i] = hb;
          ch = true;
        }
      }
    }
  }
  if (__any(ch) && (threadIdx.x & 63) == 0) atomicAdd(changed, 1u);
}

// counters[0] += waves in which a node died, counters[2] += nodes that died
template <int PHASE>
__global__ void __launch_bounds__(256)
field_unsupport_plain_kernel(FieldGrid G, const uint32_t* __restrict__ mask, const float* __restrict__ h,
                             const double* __restrict__ tab, const uint16_t* __restrict__ blk, double* dist, uint32_t* hops,
                             unsigned* __restrict__ counters) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n = (size_t)G.nrows * G.ncols * G.n_yaw;
  bool die = false;
  if (i < n) {
    const uint32_t cell = (uint32_t)(i / (uint32_t)G.n_yaw);
    const int k = (int)(i - (size_t)cell * G.n_yaw);
    if ((mask[cell] >> k) & 1u) {
      const double dv = dist[i];
      const uint32_t hv = hops[i];
      // live, and not a source (the only nodes at 0 hops)
      if (dv < INFINITY && hv != 0u && !(PHASE == 1 && hv == FIELD_NONE)) {
        bool sup = false;
        if (hv != FIELD_NONE)
          field_walk(G, mask, h, tab, blk, cell, k, [&](size_t ni, auto&& w) {
            if (sup) return;
            const uint32_t hu = hops[ni];
            if (hu == FIELD_NONE || hu + 1u != hv) return;
            sup = dist[ni] + w() == dv;
          });
        if (!sup) {
          if (PHASE == 0) dist[i] = INFINITY;
          hops[i] = FIELD_NONE;
          die = true;
        }
      }
    }
  }
  const unsigned long long b = __ballot(die);
  if (b && (threadIdx.x & 63) == 0) {
    atomicAdd(&counters[0], 1u);
    atomicAdd(&counters[2], (unsigned)__popcll(b));
  }
}

// LDS of a tile launch: n_yaw distance planes | the table | mask words | heights | (hop_planes) n_yaw hop planes | 4 words.
// Relax PHASE 0 carries no hop planes: 88 KB at 32 headings against the 126 KB of the other three rules.
inline size_t field_tile_lds(int n_yaw, bool hop_planes) {
  return (size_t)n_yaw * FIELD_PLANE * 8 + FIELD_TAB * 8 + FIELD_PLANE * 4 * 2 + (hop_planes ? (size_t)n_yaw * FIELD_PLANE * 4 : 0) +
         16;
}

// What a lane of a tile keeps in registers about its cell while it sweeps (every index is a constant once unrolled).
struct FieldLane {
  int me;           // the cell in an LDS plane
  uint32_t mw;      // its mask word
  uint32_t nbm[8];  // the mask words of the eight cells around it
  double w8[8];     // objective 0: the eight translation costs of this cell
  int widx0, wsgn;  // objective 1: table row of offset j = reverse ? j : 7 - j
};

// the pull cost of move m (0..9) at heading k of the lane's cell
__device__ __forceinline__ double field_lane_cost(const FieldGrid& G, const FieldLane& L, const double* stab, int m, int k) {
  if (m >= 8) return G.wrot;
  return G.objective == 0 ? L.w8[m] : stab[(L.widx0 + L.wsgn * m) * 32 + k];
}

// The live neighbours of heading k of the lane's cell over the ten moves: visit(li, m) with li the neighbour's place in
// the LDS planes (heading included) and m the move, for field_lane_cost (not a cost callable as in field_walk: a closure
// over L sends the lane's arrays to scratch).  bw: the node's blocked word (field_blocked_word); a set bit hides the slot.
template <class F>
__device__ __forceinline__ void field_tile_walk(const FieldGrid& G, const FieldLane& L, int k, uint32_t bw, F&& visit) {
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if ((L.nbm[j] >> k) & ~(bw >> j) & 1u) visit(k * FIELD_PLANE + L.me + field_dr(j) + field_dc(j) * FIELD_HP, j);
  if (G.n_yaw > 1) {
    const int kp = k + 1 == G.n_yaw ? 0 : k + 1, km = k == 0 ? G.n_yaw - 1 : k - 1;
    if ((L.mw >> kp) & ~(bw >> 8) & 1u) visit(kp * FIELD_PLANE + L.me, 8);
    if ((L.mw >> km) & ~(bw >> 9) & 1u) visit(km * FIELD_PLANE + L.me, 9);
  }
}

// One of the four rules on heading k of the lane's cell, inside LDS; true when the node changed.
// LEARNED: the ten pull weights of this heading are wl[0..9], the lane's slots of the weight table.
template <int PHASE, bool UNSUP, bool LEARNED>
__device__ __forceinline__ bool field_tile_rule(const FieldGrid& G, const FieldLane& L, const double* stab, const double* wl,
                                                double* sd, uint32_t* shop, int k, uint32_t bw) {
  const int own = k * FIELD_PLANE + L.me;
  const double old = sd[own];
  if (UNSUP) {
    const uint32_t hv = shop[own];
    // live, and not a source (the only nodes at 0 hops)
    if (!(old < INFINITY) || hv == 0u || (PHASE == 1 && hv == FIELD_NONE)) return false;
    bool sup = false;
    if (hv != FIELD_NONE)
      field_tile_walk(G, L, k, bw, [&](int li, int m) {
        const uint32_t hu = shop[li];
        if (hu == FIELD_NONE || hu + 1u != hv) return;
        if (sd[li] + (LEARNED ? wl[m] : field_lane_cost(G, L, stab, m, k)) == old) sup = true;
      });
    if (sup) return false;
    if (PHASE == 0) sd[own] = INFINITY;
    shop[own] = FIELD_NONE;
    return true;
  }
  if (PHASE == 0) {
    double best = old;
    field_tile_walk(G, L, k, bw, [&](int li, int m) {
      const double cand = sd[li] + (LEARNED ? wl[m] : field_lane_cost(G, L, stab, m, k));
      if (cand < best) best = cand;
    });
    if (best < old) sd[own] = best;
    return best < old;
  }
  if (!(old < INFINITY)) return false;
  const uint32_t hold = shop[own];
  uint32_t hb = hold;
  field_tile_walk(G, L, k, bw, [&](int li, int m) {
    const uint32_t hu = shop[li];
    if (hu == FIELD_NONE || hu + 1u >= hb) return;
    if (sd[li] + (LEARNED ? wl[m] : field_lane_cost(G, L, stab, m, k)) == old) hb = hu + 1u;
  });
  if (hb < hold) shop[own] = hb;
  return hb < hold;
}

// The tile skeleton.  UNSUP = 0: relax (writes back the array of its PHASE; acc is not used); UNSUP = 1: unsupport
// (writes hops back, and dist in PHASE 0; every change of a rule is a death).  counters[0] += flags set for the next
// round, [1] += tiles that ran, [2] += nodes that died (all cumulative over the host's loop).  acc collects, over a whole
// update, the tiles whose own cells or halo an unsupport pass changed: the seeds of the relax pass that follows.
// LEARNED (objectives 2 and 3): tabg is the weight table.  It is streamed from global memory, not staged: at 16 headings a tile's
// weights are 328 KB.  The ten loads of a heading are issued in front of that heading's LDS reads.
// blk (may be nullptr): the blocked words, streamed the same way: one 16-bit load per lane and heading in front of the rule.
// The body is one function, field_tile_body, of the tile index and the per-field pointers; two kernels call it:
// field_tile_kernel (one field, grid = its tiles) and field_tile_many_kernel (a batch of fields).
template <int PHASE, bool UNSUP, bool LEARNED>
__device__ __forceinline__ void
field_tile_body(const FieldGrid& G, const int tile, const uint32_t* __restrict__ mask, const float* __restrict__ h,
                const double* __restrict__ tabg, const uint16_t* __restrict__ blk, double* dist, uint32_t* hops,
                unsigned* act_cur, unsigned* act_nxt, unsigned* acc, unsigned* __restrict__ counters, int inner_max) {
  constexpr bool HOPS = PHASE == 1 || UNSUP;  // hop planes in LDS
  extern __shared__ __attribute__((aligned(16))) char smem[];
  if (!act_cur[tile]) return;  // nobody writes act_cur in this launch before the barrier below: uniform
  const int ny = G.n_yaw;
  double* sd = reinterpret_cast<double*>(smem);
  double* stab = sd + (size_t)ny * FIELD_PLANE;
  uint32_t* smask = reinterpret_cast<uint32_t*>(stab + FIELD_TAB);
  float* sh = reinterpret_cast<float*>(smask + FIELD_PLANE);
  uint32_t* shop = reinterpret_cast<uint32_t*>(sh + FIELD_PLANE);
  unsigned* sflag = reinterpret_cast<unsigned*>(shop + (HOPS ? (size_t)ny * FIELD_PLANE : 0));  // [0] border bits, [1] deaths
  const int tid = threadIdx.x;
  const int ti = tile % G.tiles_r, tj = tile / G.tiles_r;
  const int r0 = ti * FIELD_T, c0 = tj * FIELD_T;

  for (int e = tid; e < FIELD_PLANE; e += 256) {
    const int r = r0 + e % FIELD_HP - 1, c = c0 + e / FIELD_HP - 1;
    const bool in = r >= 0 && r < G.nrows && c >= 0 && c < G.ncols;
    const size_t cell = in ? (size_t)r + (size_t)c * G.nrows : 0;
    smask[e] = in ? mask[cell] & G.yaw_bits : 0u;
    sh[e] = in ? h[cell] : 0.f;
  }
  for (int e = tid; e < FIELD_PLANE * ny; e += 256) {
    const int ci = e / ny, k = e - ci * ny;
    const int r = r0 + ci % FIELD_HP - 1, c = c0 + ci / FIELD_HP - 1;
    const bool in = r >= 0 && r < G.nrows && c >= 0 && c < G.ncols;
    const size_t node = in ? ((size_t)r + (size_t)c * G.nrows) * ny + k : 0;
    sd[k * FIELD_PLANE + ci] = in ? dist[node] : (double)INFINITY;
    if (HOPS) shop[k * FIELD_PLANE + ci] = in ? hops[node] : FIELD_NONE;
  }
  if (!LEARNED)
    for (int e = tid; e < FIELD_TAB; e += 256) stab[e] = tabg[e];
  if (tid < 2) sflag[tid] = 0u;
  __syncthreads();

  const int tr = tid & (FIELD_T - 1), tc = tid >> 4;
  FieldLane L;
  L.me = (tr + 1) + (tc + 1) * FIELD_HP;
  L.mw = smask[L.me];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int nb = L.me + field_dr(j) + field_dc(j) * FIELD_HP;
    L.nbm[j] = smask[nb];
    L.w8[j] = !LEARNED && G.objective == 0 ? field_pull_cost(G, stab, j, 0, sh[L.me], sh[nb]) : 0.0;
  }
  L.widx0 = G.reverse ? 0 : 7;
  L.wsgn = G.reverse ? 1 : -1;
  unsigned border = 0u;  // bit 0 / 1: a cell of the first / last row changed, bit 2 / 3: first / last column, bit 4: any
  const unsigned my_border = (tr == 0 ? 1u : 0u) | (tr == FIELD_T - 1 ? 2u : 0u) | (tc == 0 ? 4u : 0u) |
                             (tc == FIELD_T - 1 ? 8u : 0u) | 16u;
  unsigned changes = 0u;
  int still = 0;
  // the lane's node at heading 0 (a lane outside the rectangle has L.mw == 0 and never reads)
  const size_t node0 = ((size_t)(r0 + tr) + (size_t)(c0 + tc) * G.nrows) * ny;
  for (int sweep = 0; sweep < inner_max; ++sweep) {
    bool ch = false;
    for (int k = 0; k < ny; ++k) {
      if (!((L.mw >> k) & 1u)) continue;
      double wl[10];
      if (LEARNED) {  // the lane's slots (tile, k, j): 64 consecutive doubles per wave and j
        const double* wk = tabg + ((size_t)tile * ny + k) * (10 * FIELD_T * FIELD_T) + tid;
#pragma unroll
        for (int j = 0; j < 10; ++j) wl[j] = wk[j * (FIELD_T * FIELD_T)];
      }
      const uint32_t bw = field_blocked_word(blk, node0 + k);
      if (field_tile_rule<PHASE, UNSUP, LEARNED>(G, L, stab, wl, sd, shop, k, bw)) {
        ch = true;
        ++changes;
      }
    }
    if (ch) border |= my_border;
    still = __syncthreads_or(ch ? 1 : 0);
    if (!still) break;
  }
  if (border) atomicOr(&sflag[0], border);
  if (UNSUP && changes) atomicAdd(&sflag[1], changes);
  __syncthreads();
  const unsigned bits = sflag[0];
  if (bits) {  // own cells back; the halo belongs to the neighbours
    for (int e = tid; e < FIELD_T * FIELD_T * ny; e += 256) {
      const int ci = e / ny, k = e - ci * ny;
      const int lr = ci & (FIELD_T - 1), lc = ci >> 4;
      const int r = r0 + lr, c = c0 + lc;
      if (r >= G.nrows || c >= G.ncols) continue;
      const size_t node = ((size_t)r + (size_t)c * G.nrows) * ny + k;
      const int li = k * FIELD_PLANE + (lr + 1) + (lc + 1) * FIELD_HP;
      if (PHASE == 0) dist[node] = sd[li];
      if (PHASE == 1 || UNSUP) hops[node] = shop[li];
    }
  }
  if (tid < 8) {
    const int dr = field_dr(tid), dc = field_dc(tid);
    const int ni = ti + dr, nj = tj + dc;
    const bool rows_ok = dr == 0 || (bits & (dr < 0 ? 1u : 2u));
    const bool cols_ok = dc == 0 || (bits & (dc < 0 ? 4u : 8u));
    if (rows_ok && cols_ok && (bits & 16u) && ni >= 0 && ni < G.tiles_r && nj >= 0 && nj < G.tiles_c) {
      act_nxt[ni + nj * G.tiles_r] = 1u;
      if (UNSUP) acc[ni + nj * G.tiles_r] = 1u;
      atomicAdd(&counters[0], 1u);
    }
  } else if (tid == 8) {
    if (still) {  // inner_max spent while still changing: this tile goes on in the next round
      act_nxt[tile] = 1u;
      atomicAdd(&counters[0], 1u);
    }
    if (UNSUP && bits) acc[tile] = 1u;
    atomicAdd(&counters[1], 1u);
    if (UNSUP && sflag[1]) atomicAdd(&counters[2], sflag[1]);
    act_cur[tile] = 0u;  // every lane read it in front of the first barrier
  }
}

template <int PHASE, bool UNSUP, bool LEARNED = false>
__global__ void __launch_bounds__(256)
field_tile_kernel(FieldGrid G, const uint32_t* __restrict__ mask, const float* __restrict__ h,
                  const double* __restrict__ tabg, const uint16_t* __restrict__ blk, double* dist, uint32_t* hops,
                  unsigned* act_cur, unsigned* act_nxt, unsigned* acc, unsigned* __restrict__ counters, int inner_max) {
  field_tile_body<PHASE, UNSUP, LEARNED>(G, (int)blockIdx.x, mask, h, tabg, blk, dist, hops, act_cur, act_nxt, acc, counters,
                                         inner_max);
}

// What a field of a batch brings of its own (artp_field_compute_many): the mask, the heights, the (m, k) table and the
// grid are the batch's.  flags: the field's two arrays of n_tiles words; counters: its four words of the call's block.
struct FieldSlot {
  double* dist;
  uint32_t* hops;
  unsigned* flags;
  unsigned* counters;
};

// The relax rule of PHASE on a batch of fields: grid (n_tiles, n_sets), blockIdx.y picks the slot.  parity: which of the
// slot's two flag arrays is this round's (the other collects the next round's).  A tile flags tiles of its own field only:
// every flag it writes goes through its slot's pointers.
// LEARNED (objectives 2 and 3): tabg is the batch's ONE weight table, streamed by every field.  The
// grid stays (n_tiles, n_sets): a 1-D grid decoded so that all fields of a tile share linear id % 8 (one XCD's L2, as the
// chip deals workgroups today) was measured and lost, 103.0 against 99.2 ms and 91.4 against 84.8 ms at eight fields.
template <int PHASE, bool LEARNED = false>
__global__ void __launch_bounds__(256)
field_tile_many_kernel(FieldGrid G, const uint32_t* __restrict__ mask, const float* __restrict__ h,
                       const double* __restrict__ tabg, const FieldSlot* __restrict__ slots, int parity, int inner_max) {
  const FieldSlot s = slots[blockIdx.y];
  const size_t n_tiles = (size_t)G.tiles_r * (size_t)G.tiles_c;
  field_tile_body<PHASE, false, LEARNED>(G, (int)blockIdx.x, mask, h, tabg, nullptr, s.dist, s.hops,
                                         s.flags + (parity ? n_tiles : 0), s.flags + (parity ? 0 : n_tiles), nullptr, s.counters,
                                         inner_max);
}

// bad[i] = 1 where pose i (a triple inside the rectangle) is no node of the mask (the weighted cost matrices check every
// pose in front of the table build)
__global__ void __launch_bounds__(64)
field_pose_check_kernel(FieldGrid G, const uint32_t* __restrict__ mask, const int* __restrict__ poses, int n,
                        unsigned* __restrict__ bad) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bad[i] = ((mask[(size_t)poses[3 * i] + (size_t)poses[3 * i + 1] * G.nrows] >> poses[3 * i + 2]) & 1u) ? 0u : 1u;
}

// out[b n + j] = the distance of field b at node nodes[j] (artp_field_cost_matrix): grid (ceil(n / 256), n_sets)
__global__ void __launch_bounds__(256)
field_gather_kernel(const FieldSlot* __restrict__ slots, const uint32_t* __restrict__ nodes, uint32_t n,
                    double* __restrict__ out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  out[(size_t)blockIdx.y * n + j] = slots[blockIdx.y].dist[nodes[j]];
}

__global__ void __launch_bounds__(256)
field_count_kernel(size_t n, const double* __restrict__ dist, unsigned long long* __restrict__ count) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool fin = i < n && dist[i] < INFINITY;
  const unsigned long long b = __ballot(fin);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, (unsigned long long)__popcll(b));
}

// The descent of one wave from node (r, c, k), at hv hops and distance dv, to a source: lane m tests move m, the first tight
// one that is one hop closer and not blocked wins.  nodes (n = hv + 1 triples) in travel order.  false: no tight
// predecessor (cannot happen at the fixed point).  Shared by field_path_kernel and field_paths_kernel (field_plan.h).
__device__ __forceinline__ bool field_descend(const FieldGrid& G, const uint32_t* __restrict__ mask, const float* __restrict__ h,
                                              const double* __restrict__ tab, const uint16_t* __restrict__ blk,
                                              const double* __restrict__ dist, const uint32_t* __restrict__ hops, int r, int c,
                                              int k, uint32_t hv, double dv, int* __restrict__ nodes) {
  const int lane = threadIdx.x & 63;
  const long long n = (long long)hv + 1;
  for (long long step = 0;; ++step) {
    if (lane == 0) {
      int* o = nodes + 3 * (G.reverse ? step : n - 1 - step);
      o[0] = r;
      o[1] = c;
      o[2] = k;
    }
    if (hv == 0u) return true;
    bool ok = false;
    int nr = 0, nc = 0, nk = 0;
    const size_t cell = (size_t)r + (size_t)c * G.nrows;
    if (lane < 10 && !((field_blocked_word(blk, cell * G.n_yaw + k) >> lane) & 1u) &&
        field_neighbour(G, r, c, k, lane, &nr, &nc, &nk)) {
      const size_t ncell = (size_t)nr + (size_t)nc * G.nrows;
      if ((mask[ncell] >> nk) & 1u) {
        const size_t ni = ncell * G.n_yaw + nk;
        const double w = field_has_wtab(G) ? tab[field_wtab_index(G, r, c, k, lane)]
                                          : field_pull_cost(G, tab, lane, k, h[cell], h[ncell]);
        ok = hops[ni] + 1u == hv && dist[ni] + w == dv;
      }
    }
    const unsigned long long b = __ballot(ok);
    if (!b) return false;
    const int m = __ffsll((long long)b) - 1;
    field_neighbour(G, r, c, k, m, &nr, &nc, &nk);
    r = nr;
    c = nc;
    k = nk;
    dv = dist[((size_t)r + (size_t)c * G.nrows) * G.n_yaw + k];
    hv -= 1u;
  }
}

// One wave.  out_n: the states of the path (0 = unreachable, -1 = no tight predecessor: cannot happen at the fixed point);
// nodes (cap triples) in travel order when they fit.
__global__ void __launch_bounds__(64)
field_path_kernel(FieldGrid G, const uint32_t* __restrict__ mask, const float* __restrict__ h,
                  const double* __restrict__ tab, const uint16_t* __restrict__ blk, const double* __restrict__ dist,
                  const uint32_t* __restrict__ hops, int r, int c, int k, long long cap, int* __restrict__ nodes,
                  long long* __restrict__ out_n, double* __restrict__ out_cost) {
  const int lane = threadIdx.x;
  const size_t node = ((size_t)r + (size_t)c * G.nrows) * G.n_yaw + k;
  const uint32_t hv = hops[node];
  const double dv = dist[node];
  if (lane == 0) *out_cost = dv;
  if (hv == FIELD_NONE) {
    if (lane == 0) *out_n = 0;
    return;
  }
  const long long n = (long long)hv + 1;
  if (lane == 0) *out_n = n;
  if (n > cap) return;
  if (!field_descend(G, mask, h, tab, blk, dist, hops, r, c, k, hv, dv, nodes) && lane == 0) *out_n = -1;
}

// the lattice poses of n nodes (triples local to the rectangle)
__global__ void __launch_bounds__(256)
field_poses_kernel(SamplerDev sm, MapGeom g, ReachRect rc, const int* __restrict__ nodes, size_t n,
                   double* __restrict__ se3) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = ((uint32_t)nodes[3 * i] + (uint32_t)nodes[3 * i + 1] * (uint32_t)rc.nrows) * (uint32_t)rc.n_yaw +
                     (uint32_t)nodes[3 * i + 2];
  double st[7];
  reach_lattice_pose(sm, g, rc, p, st);
#pragma unroll
  for (int j = 0; j < 7; ++j) se3[7 * i + j] = st[j];
}

__global__ void __launch_bounds__(256)
field_edge_cost_kernel(FieldGrid G, const float* __restrict__ h, const double* __restrict__ tab,
                       const uint16_t* __restrict__ blk, const int* __restrict__ a, const int* __restrict__ b, size_t n,
                       double* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int r = a[3 * i], c = a[3 * i + 1], k = a[3 * i + 2];
  const int br = b[3 * i], bc = b[3 * i + 1], bk = b[3 * i + 2];
  double w = __longlong_as_double(0x7ff8000000000000ll);
  const bool in = r >= 0 && r < G.nrows && c >= 0 && c < G.ncols && k >= 0 && k < G.n_yaw && br >= 0 && br < G.nrows &&
                  bc >= 0 && bc < G.ncols && bk >= 0 && bk < G.n_yaw;
  if (in) {
    for (int m = 0; m < 10; ++m) {
      int nr, nc, nk;
      if (!field_neighbour(G, r, c, k, m, &nr, &nc, &nk) || nr != br || nc != bc || nk != bk) continue;
      if (field_has_wtab(G))  // the travel-direction cost of a -> b, where the field's direction stores it
        w = G.reverse ? tab[field_wtab_index(G, r, c, k, m)] : tab[field_wtab_index(G, br, bc, bk, field_back_move(m))];
      else
        w = m < 8 ? field_move_cost(G, tab, m, k, h[(size_t)r + (size_t)c * G.nrows], h[(size_t)br + (size_t)bc * G.nrows])
                  : G.wrot;
      // the slot that holds a -> b: (a, m) of a reverse field, (b, the move back) of a forward one
      const size_t owner = G.reverse ? ((size_t)r + (size_t)c * G.nrows) * G.n_yaw + k : ((size_t)br + (size_t)bc * G.nrows) * G.n_yaw + bk;
      if (field_blocked_word(blk, owner) & field_slot_bits(G, G.reverse ? m : field_back_move(m))) w = INFINITY;
      break;
    }
  }
  out[i] = w;
}

// ---- objective 2: the weight table -------------------------------------------------------------------------------

// Slot s of the weight table -> the edge it holds: false where the edge does not exist (a padded lane, an end outside the
// rectangle or missing from the mask); else the pose indices (reach.h's order) of its start and target.
__device__ __forceinline__ bool field_slot_edge(const FieldGrid& G, const uint32_t* __restrict__ mask, size_t s, uint32_t* from,
                                                uint32_t* to) {
  const int lane = (int)(s % (FIELD_T * FIELD_T));
  size_t t = s / (FIELD_T * FIELD_T);
  const int j = (int)(t % 10);
  t /= 10;
  const int k = (int)(t % (size_t)G.n_yaw);
  const size_t tile = t / (size_t)G.n_yaw;
  const int r = (int)(tile % (size_t)G.tiles_r) * FIELD_T + (lane & (FIELD_T - 1));
  const int c = (int)(tile / (size_t)G.tiles_r) * FIELD_T + (lane >> 4);
  if (r >= G.nrows || c >= G.ncols) return false;
  int nr, nc, nk;
  if (!field_neighbour(G, r, c, k, j, &nr, &nc, &nk)) return false;
  const uint32_t cell = (uint32_t)r + (uint32_t)c * (uint32_t)G.nrows, ncell = (uint32_t)nr + (uint32_t)nc * (uint32_t)G.nrows;
  if (!((mask[cell] >> k) & 1u) || !((mask[ncell] >> nk) & 1u)) return false;
  const uint32_t v = cell * (uint32_t)G.n_yaw + (uint32_t)k, u = ncell * (uint32_t)G.n_yaw + (uint32_t)nk;
  *from = G.reverse ? v : u;
  *to = G.reverse ? u : v;
  return true;
}

// One EdgeMatrix row per slot first .. first + n - 1: chain_edge_matrix_kernel's row of a chain of one sub-edge between the
// lattice poses of the two nodes -- target (x, y, yaw) then start (x, y, yaw), as floats.  A slot without an edge gets a
// row of zeros (the query clamps its cell; the combine kernel discards the answer).
__global__ void __launch_bounds__(256)
field_learned_rows_kernel(FieldGrid G, SamplerDev sm, MapGeom g, ReachRect rc, const uint32_t* __restrict__ mask, size_t first,
                          uint32_t n, float* __restrict__ rows) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float row[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  uint32_t from, to;
  if (field_slot_edge(G, mask, first + i, &from, &to)) {
    double a[7], b[7];
    reach_lattice_pose(sm, g, rc, from, a);
    reach_lattice_pose(sm, g, rc, to, b);
    row[0] = (float)b[0];
    row[1] = (float)b[1];
    row[2] = (float)yaw_from_quat(b + 3);
    row[3] = (float)a[0];
    row[4] = (float)a[1];
    row[5] = (float)yaw_from_quat(a + 3);
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) rows[6 * (size_t)i + q] = row[q];
}

// chain_motion_cost_kernel's pricing of a chain of one sub-edge, for slot s of the table with the network's answer c;
// an edge whose cost is negative or NaN does not exist (the rule of the roadmap's device search: the fixed point is unique
// for weights >= 0 only).  Never NaN, never -0.
struct FieldPricing {
  float w_energy, w_time, w_risk, risk_threshold;
};
__device__ __forceinline__ double field_learned_price(const FieldGrid& G, const uint32_t* __restrict__ mask, size_t s,
                                                      const float* __restrict__ c, const FieldPricing& p) {
  uint32_t from, to;
  if (!field_slot_edge(G, mask, s, &from, &to)) return INFINITY;
  const double en = c[0], ti = c[1], ri = c[2];
  double total = 0.0;
  total += en * p.w_energy + ti * p.w_time + ri * p.w_risk;
  double w = ri <= (double)p.risk_threshold ? total : (double)INFINITY;
  if (!(w >= 0.0)) w = INFINITY;
  return w;
}

__global__ void __launch_bounds__(256)
field_learned_combine_kernel(FieldGrid G, const uint32_t* __restrict__ mask, size_t first, uint32_t n,
                             const float* __restrict__ cost3, FieldPricing p, double* __restrict__ wtab) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  wtab[first + i] = field_learned_price(G, mask, first + i, cost3 + 3 * (size_t)i, p);
}

// artp_field_update_learned: the same price against the slot's old BIT PATTERN; only a slot that differs is written, and
// the tile that owns it is flagged in acc (the seeds of the update's passes) and in wacc (counted as weight_tiles).  A slot
// is read by its own node alone, and that node's rule runs in its own tile alone: no other tile needs the flag.  `first`
// and a tile's share of the table (2560 n_yaw slots) are multiples of 64: the slots of a wave lie in one tile.
// cnt[5] += changed slots, one atomic per wave.
__global__ void __launch_bounds__(256)
field_learned_reprice_kernel(FieldGrid G, const uint32_t* __restrict__ mask, size_t first, uint32_t n,
                             const float* __restrict__ cost3, FieldPricing p, double* __restrict__ wtab,
                             unsigned* __restrict__ acc, unsigned* __restrict__ wacc, unsigned long long* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const size_t s = first + i;
  bool ch = false;
  if (i < n) {
    const double w = field_learned_price(G, mask, s, cost3 + 3 * (size_t)i, p);
    ch = __double_as_longlong(w) != __double_as_longlong(wtab[s]);
    if (ch) wtab[s] = w;
  }
  const unsigned long long b = __ballot(ch);
  if (b && (threadIdx.x & 63) == 0) {
    const size_t tile = s / ((size_t)G.n_yaw * 10 * (FIELD_T * FIELD_T));  // lane 0 of a wave is never past n when b != 0
    acc[tile] = 1u;
    wacc[tile] = 1u;
    atomicAdd(&cnt[5], (unsigned long long)__popcll(b));
  }
}

// cnt[6] = the flags set among wacc[0 .. n_tiles - 1]
__global__ void __launch_bounds__(256)
field_count_flags_kernel(uint32_t n_tiles, const unsigned* __restrict__ wacc, unsigned long long* __restrict__ cnt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long b = __ballot(i < n_tiles && wacc[i] != 0u);
  if (b && (threadIdx.x & 63) == 0) atomicAdd(&cnt[6], (unsigned long long)__popcll(b));
}

// ---- artp_field_update ------------------------------------------------------------------------------------------

// the tiles that hold cell (r, c) or one of its eight neighbours: every tile that has the cell in its own cells or halo
__device__ __forceinline__ void field_flag_around(const FieldGrid& G, int r, int c, unsigned* flags) {
  for (int dc = -1; dc <= 1; ++dc)
    for (int dr = -1; dr <= 1; ++dr) {
      const int rr = r + dr, cc = c + dc;
      if (rr >= 0 && rr < G.nrows && cc >= 0 && cc < G.ncols) flags[rr / FIELD_T + (cc / FIELD_T) * G.tiles_r] = 1u;
    }
}

struct FieldSub {
  int row0, col0, nrows, ncols;  // local to the field's rectangle
};

// cnt[0] changed words, [1] removed bits, [2] added bits, [3] changed heights, [4] sources that are no nodes any more,
// [5] changed slots and [6] tiles flagged by them (artp_field_update_learned, artp_field_update_clearance), [7] nodes whose
// clearance changed (artp_field_update_clearance)

// one lane per source against the merged mask (the new word inside sub, the field's own outside)
__global__ void __launch_bounds__(64)
field_update_sources_kernel(FieldGrid G, FieldSub sub, const uint32_t* __restrict__ mask, const uint32_t* __restrict__ new_mask,
                            const int* __restrict__ src, int n_src, unsigned long long* __restrict__ cnt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_src) return;
  const int r = src[3 * i], c = src[3 * i + 1], k = src[3 * i + 2];
  const size_t cell = (size_t)r + (size_t)c * G.nrows;
  const bool in = r >= sub.row0 && r < sub.row0 + sub.nrows && c >= sub.col0 && c < sub.col0 + sub.ncols;
  if (!(((in ? new_mask[cell] : mask[cell]) >> k) & 1u)) atomicAdd(&cnt[4], 1ull);
}

// One lane per cell of sub, after field_update_sources_kernel in the same stream: nothing is written when cnt[4] != 0.
__global__ void __launch_bounds__(256)
field_diff_kernel(FieldGrid G, FieldSub sub, const uint32_t* __restrict__ new_mask, uint32_t* __restrict__ mask, int refresh,
                  SamplerDev sm, int map_rows, ReachRect rc, float* __restrict__ h, double* __restrict__ dist,
                  uint32_t* __restrict__ hops, unsigned* acc, unsigned long long* cnt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint32_t)sub.nrows * (uint32_t)sub.ncols) return;
  if (cnt[4]) return;
  const int r = sub.row0 + (int)(i % (uint32_t)sub.nrows), c = sub.col0 + (int)(i / (uint32_t)sub.nrows);
  const size_t cell = (size_t)r + (size_t)c * G.nrows;
  const uint32_t old = mask[cell], nw = new_mask[cell];
  const uint32_t diff = (old ^ nw) & G.yaw_bits;
  bool touched = diff != 0u;
  if (old != nw) mask[cell] = nw;
  if (diff) {
    const uint32_t gone = old & diff;
    for (int k = 0; k < G.n_yaw; ++k)
      if ((gone >> k) & 1u) {
        dist[cell * G.n_yaw + k] = INFINITY;
        hops[cell * G.n_yaw + k] = FIELD_NONE;
      }
    atomicAdd(&cnt[0], 1ull);
    if (gone) atomicAdd(&cnt[1], (unsigned long long)__popc(gone));
    if (nw & diff) atomicAdd(&cnt[2], (unsigned long long)__popc(nw & diff));
  }
  if (refresh) {
    const float hn = sm.cells[2 * ((size_t)(rc.row0 + r) + (size_t)(rc.col0 + c) * map_rows)].x;
    if (__float_as_uint(hn) != __float_as_uint(h[cell])) {  // bit patterns: a NaN height stays "unchanged"
      h[cell] = hn;
      touched = true;
      atomicAdd(&cnt[3], 1ull);
    }
  }
  if (touched) field_flag_around(G, r, c, acc);
}

// hops = NONE where the distance is not the one of the snapshot; the tiles around such a node are flagged
__global__ void __launch_bounds__(256)
field_hop_reset_kernel(FieldGrid G, const double* __restrict__ dist, const double* __restrict__ snap,
                       uint32_t* __restrict__ hops, unsigned* acc) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)G.nrows * G.ncols * G.n_yaw) return;
  if (__double_as_longlong(dist[i]) == __double_as_longlong(snap[i])) return;
  hops[i] = FIELD_NONE;
  const uint32_t cell = (uint32_t)(i / (uint32_t)G.n_yaw);
  field_flag_around(G, (int)(cell % (uint32_t)G.nrows), (int)(cell / (uint32_t)G.nrows), acc);
}

// ---- artp_field_shift ---------------------------------------------------------------------

// The map moved by (si, sj) whole cells under a rectangle that keeps its map indices: node (r, c, k) becomes node
// (r + si, c + sj, k).  The node index is (r + c nrows) n_yaw + k, so a destination reads the element a constant number
// of places in front of it -- (si + sj nrows) n_yaw nodes, si + sj nrows cells -- when its old cell lay inside the
// rectangle.  One lane per destination element: the lanes of a wave read and write consecutive addresses.  The rows that
// leave on one side are the rows that enter on the other, so a workgroup would read what another has written already:
// the kernels write into scratch, and the host copies back.
struct FieldShift {
  int si, sj;
  long long cell_off;  // si + sj nrows
};
__device__ __forceinline__ bool field_shift_inside(const FieldGrid& G, int r, int c) {
  return r >= 0 && r < G.nrows && c >= 0 && c < G.ncols;
}

// One lane per destination node: dist and hops (+inf / NONE in the cells that entered), and with blk != nullptr the
// blocked words (0 there).  A blocked word moves with its node and loses the translation slots whose neighbour now lies
// outside the rectangle; a node that left takes its word with it.  cnt[7] += blocked moves kept, counted as
// field_unblock_kernel counts them (blocked moves are few: one atomic per word that holds any).
__global__ void __launch_bounds__(256)
field_shift_nodes_kernel(FieldGrid G, FieldShift sh, const double* __restrict__ dist, const uint32_t* __restrict__ hops,
                         const uint16_t* __restrict__ blk, double* __restrict__ dist_o, uint32_t* __restrict__ hops_o,
                         uint16_t* __restrict__ blk_o, unsigned long long* __restrict__ cnt) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)G.nrows * G.ncols * G.n_yaw) return;
  const uint32_t cell = (uint32_t)(i / (uint32_t)G.n_yaw);
  const int r = (int)(cell % (uint32_t)G.nrows), c = (int)(cell / (uint32_t)G.nrows);
  const bool in = field_shift_inside(G, r - sh.si, c - sh.sj);
  const size_t s = in ? (size_t)((long long)i - sh.cell_off * G.n_yaw) : 0;
  dist_o[i] = in ? dist[s] : (double)INFINITY;
  hops_o[i] = in ? hops[s] : FIELD_NONE;
  if (!blk) return;
  uint32_t w = in ? (uint32_t)blk[s] : 0u;
  if (w) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (!field_shift_inside(G, r + field_dr(j), c + field_dc(j))) w &= ~(1u << j);
    if (w) atomicAdd(&cnt[7], (unsigned long long)(G.n_yaw == 2 ? __popc(w & 0xffu) + ((w & 0x300u) ? 1 : 0) : __popc(w)));
  }
  blk_o[i] = (uint16_t)w;
}

// One lane per destination cell: the mask word (0 in a cell that entered) and the height (there: the sampler layer's, as
// field_heights_kernel reads it).  cnt[5] += the nodes of the cells that left -- the lane's own old cell when (r + si,
// c + sj) lies outside -- one atomic per wave.  The rectangle's border row and column on the sides through which cells
// left flag the tiles around their cells in acc: a kept node there may have had its only support outside.  Its mask word
// does not change, so no diff would flag it, and the unsupport pass has to look at it.
__global__ void __launch_bounds__(256)
field_shift_cells_kernel(FieldGrid G, FieldShift sh, SamplerDev sm, int map_rows, ReachRect rc,
                         const uint32_t* __restrict__ mask, const float* __restrict__ h, uint32_t* __restrict__ mask_o,
                         float* __restrict__ h_o, unsigned* acc, unsigned long long* __restrict__ cnt) {
  const uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned left = 0u;
  if (cell < (uint32_t)G.nrows * (uint32_t)G.ncols) {
    const int r = (int)(cell % (uint32_t)G.nrows), c = (int)(cell / (uint32_t)G.nrows);
    const bool in = field_shift_inside(G, r - sh.si, c - sh.sj);
    const size_t s = in ? (size_t)((long long)cell - sh.cell_off) : 0;
    mask_o[cell] = in ? mask[s] : 0u;
    h_o[cell] = in ? h[s] : sm.cells[2 * ((size_t)(rc.row0 + r) + (size_t)(rc.col0 + c) * map_rows)].x;
    if (!field_shift_inside(G, r + sh.si, c + sh.sj)) left = (unsigned)__popc(mask[cell] & G.yaw_bits);
    if ((sh.si > 0 && r == G.nrows - 1) || (sh.si < 0 && r == 0) || (sh.sj > 0 && c == G.ncols - 1) || (sh.sj < 0 && c == 0))
      field_flag_around(G, r, c, acc);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) left += __shfl_down(left, d);
  if ((threadIdx.x & 63) == 0 && left) atomicAdd(&cnt[5], (unsigned long long)left);
}

}  // namespace artp

struct artp_field {
  artp_ctx* ctx = nullptr;
  artp_field_params params{};
  artp::ReachRect rect{};
  artp::FieldGrid grid{};
  MapGeom geom{};         // of the map the field was computed on (the poses of artp_field_path)
  SamplerDev sampler{};
  uint64_t map_version = 0;
  size_t n_nodes = 0, n_cells = 0, n_tiles = 0;
  double* d_dist = nullptr;
  uint32_t* d_hops = nullptr;
  uint32_t* d_mask = nullptr;
  float* d_h = nullptr;
  double* d_tab = nullptr;
  unsigned* d_flags = nullptr;   // two flag arrays of n_tiles words | counters[4]
  int* d_nodes = nullptr;        // sources at compute time; path / edge scratch later
  size_t nodes_cap = 0;          // ints
  double* d_out = nullptr;       // path poses / edge costs
  size_t out_cap = 0;            // doubles
  artp_field_stats_t stats{};
  // artp_field_update: the sources (d_nodes is path scratch after compute) and the scratch of the first update
  std::vector<int> h_src;
  int* d_src = nullptr;
  double* d_snap = nullptr;             // dist in front of the searches of an update
  unsigned* d_acc = nullptr;            // n_tiles flags: the tiles an update touched so far
  unsigned long long* d_ucnt = nullptr; // the eight counts of the diff
  uint32_t* d_stage = nullptr;          // a host mask's sub-rectangle, in the field's layout
  artp_field_update_stats_t ustats{};
  // artp_field_compute_learned: d_tab is the weight table (field_wtab_slots doubles); the scratch lives during the build
  artp_field_learned_params lparams{};
  artp_field_learned_stats_t lstats{};
  // artp_field_compute_clearance (clearance.h): grid.objective = 3, params = the base objective's, d_tab the weight table
  artp_field_clearance_params cparams{};
  uint16_t* d_d2 = nullptr;             // the clearance map of the field's own mask, one word per node
  double* d_btab = nullptr;             // the base objective's (m, k) table (FIELD_TAB doubles): d_tab is the weight table
  artp_field_clearance_update_stats_t custats{};  // artp_field_update_clearance; d_wacc stays from its first call on
  float* d_lscratch = nullptr;          // per chunk: 6 floats of EdgeMatrix row, then 3 floats of answer, per row
  // artp_field_update_learned: d_lscratch stays from the first update on
  unsigned* d_wacc = nullptr;           // n_tiles flags: the tiles a changed weight flagged
  artp_field_learned_update_stats_t lustats{};
  // the blocked-move set (field_plan.h): allocated by the first block, one 16-bit word per node (padded to 32-bit words)
  uint16_t* d_blk = nullptr;
  uint64_t n_blocked = 0;               // bits set in d_blk
  artp_field_plan_stats_t pstats{};
  std::vector<uint64_t> plan_round_runs;  // tile runs of the repair of every round of the last artp_field_plan (0: none)
  // artp_field_plan's scratch: per-target records, path nodes, poses, the move list, the (s1, s2) pairs and verdicts
  void* d_plan = nullptr;
  size_t plan_targets = 0, plan_states = 0;
  // artp_field_simplify_paths' scratch (field_simplify.h): one block, grown to the largest call
  char* d_simplify = nullptr;
  size_t simplify_cap = 0;              // bytes
  artp_field_simplify_stats_t sstats{};
  // artp_field_shift: where the move writes (hops | mask words | heights | blocked words; dist goes through d_snap),
  // allocated by the first shift
  char* d_shift = nullptr;
  artp_field_shift_stats_t shstats{};
  // artp_field_shift_clearance (clearance.h): the second weight table, allocated by the first call that moves and kept;
  // a move prices into it and swaps it with d_tab, which never leaves the library
  double* d_tab2 = nullptr;
  artp_field_clearance_shift_stats_t clshstats{};
  DeviceScratch mem;  // owns every d_* above: freed with the field, or earlier by mem.release
};

namespace {

// the caller has set the device
void field_free(artp_field* f) {
  (void)hipStreamSynchronize(f->ctx->lane->stream);
  delete f;
}

// a buffer of the field that is allocated by whoever needs it first
template <class T>
int field_lazy(artp_field* f, T** p, size_t count) {
  if (!*p) HIP_TRY(f->ctx, f->mem.alloc(p, count));
  return ARTP_OK;
}

// a buffer that grows to the largest request: the old block is freed ahead of the new one (its contents are scratch)
template <class T>
int field_grow(artp_field* f, T** p, size_t* cap, size_t count) {
  if (*cap >= count) return ARTP_OK;
  f->mem.release(*p);
  *p = nullptr;
  *cap = 0;
  HIP_TRY(f->ctx, f->mem.alloc(p, count));
  *cap = count;
  return ARTP_OK;
}

int field_ensure_scratch(artp_field* f, size_t ints, size_t doubles) {
  ARTP_TRY(field_grow(f, &f->d_nodes, &f->nodes_cap, ints));
  return field_grow(f, &f->d_out, &f->out_cap, doubles);
}

// rows of the cost query per chunk of a learned field's table, and of its scratch (d_lscratch: 36 bytes a row)
size_t field_learned_chunk(const artp::FieldGrid& G) { return std::min(artp::field_wtab_slots(G), artp::FIELD_LEARNED_CHUNK); }

// N timing events on a stream.  An event that could not be created is skipped; ms(i, j, clean) is the stream time between
// marks i and j, 0 unless both events exist and the caller says the run between them ended clean (and is synchronised).
template <int N>
class StreamTimer {
 public:
  explicit StreamTimer(hipStream_t st) : st_(st) {
    for (hipEvent_t& x : e_)
      if (hipEventCreate(&x) != hipSuccess) x = nullptr;
  }
  StreamTimer(const StreamTimer&) = delete;
  StreamTimer& operator=(const StreamTimer&) = delete;
  ~StreamTimer() {
    for (hipEvent_t x : e_)
      if (x) (void)hipEventDestroy(x);
  }
  void mark(int i) {
    if (e_[i]) (void)hipEventRecord(e_[i], st_);
  }
  double ms(int i, int j, bool clean) const {
    float t = 0.f;
    return clean && e_[i] && e_[j] && hipEventElapsedTime(&t, e_[i], e_[j]) == hipSuccess ? (double)t : 0.0;
  }

 private:
  hipStream_t st_;
  hipEvent_t e_[N];
};

// the (m, k) table of objective 1 and the squared planar step lengths of objective 0
void field_make_table(const artp_field_params& p, const MapGeom& g, int n_yaw, double* tab) {
  const double pi = 3.14159265358979323846;
  for (int m = 0; m < 8; ++m) {
    const double dx = g.res * (double)(-artp::field_dr(m)), dy = g.res * (double)(-artp::field_dc(m));
    tab[8 * 32 + m] = dx * dx + dy * dy;
    for (int k = 0; k < 32; ++k) {
      double yaw = (2.0 * pi / (double)n_yaw) * (double)k;
      if (yaw > pi) yaw -= 2.0 * pi;
      const double lon = std::cos(yaw) * dx + std::sin(yaw) * dy;
      const double lat = -std::sin(yaw) * dx + std::cos(yaw) * dy;
      const double t_lon = std::fabs(lon) / p.max_lon_vel, t_lat = std::fabs(lat) / p.max_lat_vel;
      tab[m * 32 + k] = k < n_yaw ? std::max(std::max(t_lon, t_lat), 0.0) : INFINITY;  // t_yaw = 0: a translation
    }
  }
}

struct FieldRounds {
  uint64_t rounds = 0;     // launches
  uint64_t tile_runs = 0;  // tiled form: tiles that ran in them
  uint64_t deaths = 0;     // unsupport: nodes that died
};

// The host loop of every pass: `batch` launches, one read of the counters, until a batch flagged nothing.
// launch(cur, nxt, counters) enqueues one round; cur / nxt are the two flag arrays of d_flags in turn (the tiled form's;
// the caller has seeded the first).  A round settles (or kills) at least what a plain sweep does, and sweep s settles every
// node whose best path has <= s edges: more rounds than nodes + 2 end the call with `too_many`.
template <class Launch>
int field_rounds(artp_field* f, int batch, const char* too_many, FieldRounds* out, Launch&& launch) {
  artp_ctx* c = f->ctx;
  hipStream_t st = c->lane->stream;
  unsigned* counters = f->d_flags + 2 * f->n_tiles;
  const uint64_t cap = (uint64_t)f->n_nodes + 2;
  unsigned seen = 0;
  for (uint64_t round = 0;;) {
    if (round > cap) {
      c->last_error = too_many;
      return ARTP_ERR_CAPACITY;
    }
    for (int b = 0; b < batch; ++b, ++round)
      launch(f->d_flags + (round & 1) * f->n_tiles, f->d_flags + ((round + 1) & 1) * f->n_tiles, counters);
    HIP_TRY(c, hipGetLastError());
    unsigned now[3] = {0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(now, counters, sizeof(now), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    *out = FieldRounds{round, now[1], now[2]};
    if (now[0] == seen) return ARTP_OK;  // nothing flagged for the next round
    seen = now[0];
  }
}

// One pass of one rule (UNSUP = 0: relax, 1: unsupport; PHASE 0: distances, 1: hop counts) to its fixed point, in the
// field's form.  The tiled form's first round runs the n_tiles flags of d_seed (artp_field_update: the tiles that changed
// so far, which an unsupport pass adds to), or the tiles of the sources without one.
template <int PHASE, bool UNSUP>
int field_pass(artp_field* f, unsigned* d_seed, FieldRounds* out) {
  artp_ctx* c = f->ctx;
  hipStream_t st = c->lane->stream;
  const artp::FieldGrid& G = f->grid;
  const char* too_many = UNSUP ? "artp_field_update: more unsupport rounds than nodes" : "artp_field_compute: more rounds than nodes";
  HIP_TRY(c, hipMemsetAsync(f->d_flags, 0, (2 * f->n_tiles + 4) * sizeof(unsigned), st));
  if (f->params.plain_sweeps) {
    const unsigned blocks = (unsigned)((f->n_nodes + 255) / 256);
    return field_rounds(f, 16, too_many, out, [&](unsigned*, unsigned*, unsigned* counters) {
      hipLaunchKernelGGL(UNSUP ? artp::field_unsupport_plain_kernel<PHASE> : artp::field_plain_kernel<PHASE>, dim3(blocks),
                         dim3(256), 0, st, G, (const uint32_t*)f->d_mask, (const float*)f->d_h, (const double*)f->d_tab,
                         (const uint16_t*)f->d_blk, f->d_dist, f->d_hops, counters);
    });
  }
  if (d_seed) {
    HIP_TRY(c, hipMemcpyAsync(f->d_flags, d_seed, f->n_tiles * sizeof(unsigned), hipMemcpyDeviceToDevice, st));
  } else {
    const int n_src = (int)(f->h_src.size() / 3);
    hipLaunchKernelGGL(artp::field_seed_tiles_kernel, dim3((unsigned)((n_src + 63) / 64)), dim3(64), 0, st, G,
                       (const int*)f->d_nodes, n_src, f->d_flags);
    HIP_TRY(c, hipGetLastError());
  }
  const size_t lds = artp::field_tile_lds(G.n_yaw, PHASE == 1 || UNSUP);
  auto kernel = &artp::field_tile_kernel<PHASE, UNSUP, false>;
  if (artp::field_has_wtab(G)) kernel = &artp::field_tile_kernel<PHASE, UNSUP, true>;
  // a workgroup may ask for more than 64 KB of dynamic LDS once the function says so (32 headings: 88 / 126 KB)
  if (lds > 64 * 1024)
    HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
  return field_rounds(f, 1, too_many, out, [&](unsigned* cur, unsigned* nxt, unsigned* counters) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)f->n_tiles), dim3(256), lds, st, G,
                       (const uint32_t*)f->d_mask, (const float*)f->d_h, (const double*)f->d_tab, (const uint16_t*)f->d_blk,
                       f->d_dist, f->d_hops, cur, nxt, UNSUP ? d_seed : nullptr, counters, f->params.inner_sweeps);
  });
}

int field_count_reached(artp_field* f, uint64_t* reached) {
  artp_ctx* c = f->ctx;
  hipStream_t st = c->lane->stream;
  unsigned long long* d_count = reinterpret_cast<unsigned long long*>(f->d_out);  // >= 8 doubles since the compute
  HIP_TRY(c, hipMemsetAsync(d_count, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(artp::field_count_kernel, dim3((unsigned)((f->n_nodes + 255) / 256)), dim3(256), 0, st, f->n_nodes,
                     (const double*)f->d_dist, d_count);
  HIP_TRY(c, hipGetLastError());
  unsigned long long n = 0;
  HIP_TRY(c, hipMemcpyAsync(&n, d_count, sizeof(n), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  *reached = n;
  return ARTP_OK;
}

// Objective 2: price every slot of the weight table f->d_tab from f->d_mask, in table order, in chunks of at most
// FIELD_LEARNED_CHUNK rows: the rows, the context's own cost query (always the device network: the kernels
// artp_cost_query_dev launches, on the context's stream, whatever artp_cost_set_external_query installed), then the
// combination (reprice = false: every slot is written) or the repricing (true: the slots that change are written and
// their tiles flagged in d_acc and d_wacc, their number added to d_ucnt[5]).  The scratch is allocated when there is
// none and left to the caller.  ms[0..2] += the device time of the three steps, *chunks += the query calls.
int field_learned_table(artp_ctx* c, artp_field* f, bool reprice, double ms[3], uint64_t* chunks) {
  hipStream_t st = c->lane->stream;
  const artp::FieldGrid& G = f->grid;
  const artp_field_learned_params& lp = f->lparams;
  const artp::FieldPricing price{lp.w_energy, lp.w_time, lp.w_risk, lp.risk_threshold};
  const size_t slots = artp::field_wtab_slots(G), chunk = field_learned_chunk(G);
  ARTP_TRY(field_lazy(f, &f->d_lscratch, chunk * 9));
  float* rows = f->d_lscratch;
  float* cost3 = f->d_lscratch + chunk * 6;
  std::deque<StreamTimer<4>> timers;  // one per chunk, read behind the one synchronisation
  int rc = ARTP_OK;
  for (size_t first = 0; first < slots && rc == ARTP_OK; first += chunk) {
    const uint32_t n = (uint32_t)(slots - first < chunk ? slots - first : chunk);
    const unsigned blocks = (n + 255) / 256;
    StreamTimer<4>& tm = timers.emplace_back(st);
    tm.mark(0);
    hipLaunchKernelGGL(artp::field_learned_rows_kernel, dim3(blocks), dim3(256), 0, st, G, f->sampler, f->geom, f->rect,
                       (const uint32_t*)f->d_mask, first, n, rows);
    tm.mark(1);
    rc = artp_cost_query_dev(c, rows, n, cost3);
    if (rc) break;
    tm.mark(2);
    if (reprice)
      hipLaunchKernelGGL(artp::field_learned_reprice_kernel, dim3(blocks), dim3(256), 0, st, G, (const uint32_t*)f->d_mask, first,
                         n, (const float*)cost3, price, f->d_tab, f->d_acc, f->d_wacc, f->d_ucnt);
    else
      hipLaunchKernelGGL(artp::field_learned_combine_kernel, dim3(blocks), dim3(256), 0, st, G, (const uint32_t*)f->d_mask, first,
                         n, (const float*)cost3, price, f->d_tab);
    tm.mark(3);
    if (hipGetLastError() != hipSuccess) rc = ARTP_ERR_HIP;
    ++*chunks;
  }
  if (hipStreamSynchronize(st) != hipSuccess && rc == ARTP_OK) rc = ARTP_ERR_HIP;
  for (const StreamTimer<4>& tm : timers)
    for (int q = 0; q < 3; ++q) ms[q] += tm.ms(q, q + 1, rc == ARTP_OK);
  timers.clear();
  (void)hipGetLastError();
  if (rc == ARTP_ERR_HIP && c->last_error.empty()) c->last_error = "learned field: pricing the weight table failed";
  return rc;
}

// artp_field_compute_learned's table: built once, the scratch given back
int field_learned_build(artp_ctx* c, artp_field* f) {
  double ms[3] = {0.0, 0.0, 0.0};
  const int rc = field_learned_table(c, f, false, ms, &f->lstats.chunks);
  if (rc) return rc;
  f->lstats.rows_ms = ms[0];
  f->lstats.query_ms = ms[1];
  f->lstats.combine_ms = ms[2];
  f->mem.release(f->d_lscratch);
  f->d_lscratch = nullptr;
  f->lstats.table_rows = artp::field_wtab_slots(f->grid);
  f->lstats.table_bytes = f->lstats.table_rows * sizeof(double);
  return ARTP_OK;
}

int field_clearance_build(artp_ctx* c, artp_field* f, const double* tab);  // clearance.h

int field_compute_impl(artp_ctx* c, artp_field* f, const uint32_t* mask, int mask_on_device, const int* sources,
                       size_t n_sources) {
  hipStream_t st = c->lane->stream;
  const artp::FieldGrid& G = f->grid;
  const bool learned = G.objective == 2, wtab = artp::field_has_wtab(G);
  const size_t tab_doubles = wtab ? artp::field_wtab_slots(G) : (size_t)artp::FIELD_TAB;
  if (wtab) {  // 80 bytes per node and the padding of the edge tiles, plus a chunk of query scratch (learned) or d2 (clearance)
    const size_t extra = learned ? field_learned_chunk(G) * 9 * sizeof(float) : f->n_nodes * sizeof(uint16_t) + artp::FIELD_TAB * sizeof(double);
    const size_t need = tab_doubles * sizeof(double) + extra + f->n_nodes * 12 + f->n_cells * 8;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
    if (need > free_b) {
      c->last_error = std::string(learned ? "artp_field_compute_learned" : "artp_field_compute_clearance") +
                      ": the weight table needs " + std::to_string(need >> 20) + " MB, the device has " +
                      std::to_string(free_b >> 20) + " MB free";
      return ARTP_ERR_CAPACITY;
    }
  }
  HIP_TRY(c, f->mem.alloc(&f->d_dist, f->n_nodes));
  HIP_TRY(c, f->mem.alloc(&f->d_hops, f->n_nodes));
  HIP_TRY(c, f->mem.alloc(&f->d_mask, f->n_cells));
  HIP_TRY(c, f->mem.alloc(&f->d_h, f->n_cells));
  HIP_TRY(c, f->mem.alloc(&f->d_tab, tab_doubles));
  HIP_TRY(c, f->mem.alloc(&f->d_flags, 2 * f->n_tiles + 4));
  int rc = field_ensure_scratch(f, 3 * n_sources, 8);
  if (rc) return rc;
  double tab[artp::FIELD_TAB];
  field_make_table(f->params, f->geom, G.n_yaw, tab);
  HIP_TRY(c, hipMemcpyAsync(f->d_mask, mask, f->n_cells * sizeof(uint32_t),
                            mask_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  if (!wtab) HIP_TRY(c, hipMemcpyAsync(f->d_tab, tab, sizeof(tab), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(f->d_nodes, sources, 3 * n_sources * sizeof(int), hipMemcpyHostToDevice, st));
  f->h_src.assign(sources, sources + 3 * n_sources);  // d_nodes becomes path scratch; artp_field_update needs them
  HIP_TRY(c, hipMemsetAsync(f->d_flags, 0, (2 * f->n_tiles + 4) * sizeof(unsigned), st));
  hipLaunchKernelGGL(artp::field_heights_kernel, dim3((unsigned)((f->n_cells + 255) / 256)), dim3(256), 0, st, f->sampler,
                     f->geom, f->rect, f->d_h);
  hipLaunchKernelGGL(artp::field_init_kernel, dim3((unsigned)((f->n_nodes + 255) / 256)), dim3(256), 0, st, f->n_nodes,
                     f->d_dist, f->d_hops);
  unsigned* counters = f->d_flags + 2 * f->n_tiles;
  hipLaunchKernelGGL(artp::field_sources_kernel, dim3((unsigned)((n_sources + 63) / 64)), dim3(64), 0, st, G,
                     (const uint32_t*)f->d_mask, (const int*)f->d_nodes, (int)n_sources, f->d_dist, f->d_hops, counters);
  HIP_TRY(c, hipGetLastError());
  unsigned bad = 0;
  HIP_TRY(c, hipMemcpyAsync(&bad, counters, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));  // the host copies of mask, table and sources are free from here
  if (bad) {
    c->last_error = "artp_field_compute: a source is not a node of the mask";
    return ARTP_ERR_INVALID_ARG;
  }
  if (learned) {
    rc = field_learned_build(c, f);
    if (rc) return rc;
  } else if (wtab) {
    rc = field_clearance_build(c, f, tab);
    if (rc) return rc;
  }
  FieldRounds dist_pass, hop_pass;
  const auto t0 = std::chrono::steady_clock::now();
  rc = field_pass<0, false>(f, nullptr, &dist_pass);
  if (rc) return rc;
  const auto t1 = std::chrono::steady_clock::now();
  rc = field_pass<1, false>(f, nullptr, &hop_pass);
  if (rc) return rc;
  f->lstats.dist_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
  f->lstats.hop_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
  (f->params.plain_sweeps ? f->stats.plain_sweeps : f->stats.outer_rounds) = dist_pass.rounds;
  f->stats.tile_launches = dist_pass.tile_runs;
  f->stats.hop_rounds = hop_pass.rounds;
  f->stats.hop_tile_launches = hop_pass.tile_runs;
  return field_count_reached(f, &f->stats.reached_nodes);
}

// What an update, a block or a plan works in, allocated by the first of them.  stage: d_stage, for a host mask; wacc:
// d_wacc, for the two kinds whose weights sit in the table.
int field_update_scratch(artp_field* f, bool stage, bool wacc = false) {
  artp_ctx* c = f->ctx;
  if (!f->d_src) {
    HIP_TRY(c, f->mem.alloc(&f->d_src, f->h_src.size()));
    HIP_TRY(c, hipMemcpyAsync(f->d_src, f->h_src.data(), f->h_src.size() * sizeof(int), hipMemcpyHostToDevice, c->lane->stream));
  }
  ARTP_TRY(field_lazy(f, &f->d_snap, f->n_nodes));
  ARTP_TRY(field_lazy(f, &f->d_acc, f->n_tiles));
  ARTP_TRY(field_lazy(f, &f->d_ucnt, 8));
  if (stage) ARTP_TRY(field_lazy(f, &f->d_stage, f->n_cells));
  if (wacc) ARTP_TRY(field_lazy(f, &f->d_wacc, f->n_tiles));
  return ARTP_OK;
}

// The passes of an update after the diff found a change: unsupport and relax on distances, then on hop counts, each from
// the tiles flagged so far.
int field_update_passes(artp_field* f, artp_field_update_stats_t* us) {
  artp_ctx* c = f->ctx;
  hipStream_t st = c->lane->stream;
  HIP_TRY(c, hipMemcpyAsync(f->d_snap, f->d_dist, f->n_nodes * sizeof(double), hipMemcpyDeviceToDevice, st));
  FieldRounds unsup[2], relax[2];
  int rc = field_pass<0, true>(f, f->d_acc, &unsup[0]);
  if (rc) return rc;
  rc = field_pass<0, false>(f, f->d_acc, &relax[0]);
  if (rc) return rc;
  hipLaunchKernelGGL(artp::field_hop_reset_kernel, dim3((unsigned)((f->n_nodes + 255) / 256)), dim3(256), 0, st, f->grid,
                     (const double*)f->d_dist, (const double*)f->d_snap, f->d_hops, f->d_acc);
  HIP_TRY(c, hipGetLastError());
  rc = field_pass<1, true>(f, f->d_acc, &unsup[1]);
  if (rc) return rc;
  rc = field_pass<1, false>(f, f->d_acc, &relax[1]);
  if (rc) return rc;
  us->dead_nodes = unsup[0].deaths;
  us->hop_dead_nodes = unsup[1].deaths;
  us->unsupport_rounds = unsup[0].rounds + unsup[1].rounds;
  us->dist_rounds = relax[0].rounds;
  us->hop_rounds = relax[1].rounds;
  us->tile_launches = unsup[0].tile_runs + relax[0].tile_runs + unsup[1].tile_runs + relax[1].tile_runs;
  return field_count_reached(f, &us->reached_nodes);
}

// The diff of an update (step 1 of section 13): the sources tested against the merged mask on the device, then the words
// of sub installed, the removed nodes cleared and the tiles around every changed cell flagged in d_acc; the caller has cleared d_acc and d_ucnt.
// cnt = the first five counts of d_ucnt; cnt[4] != 0: a source is gone and nothing was written.
int field_update_diff(artp_field* f, const uint32_t* new_mask, int mask_on_device, const artp::FieldSub& sub, bool refresh,
                      const SamplerDev& sm, unsigned long long cnt[5]) {
  artp_ctx* c = f->ctx;
  hipStream_t st = c->lane->stream;
  const artp::FieldGrid& G = f->grid;
  const uint32_t* nm = new_mask;
  if (!mask_on_device) {  // the columns of sub_rect only, to the same place of a buffer in the field's layout
    const size_t off = (size_t)sub.row0 + (size_t)sub.col0 * G.nrows, pitch = (size_t)G.nrows * sizeof(uint32_t);
    HIP_TRY(c, hipMemcpy2DAsync(f->d_stage + off, pitch, new_mask + off, pitch, (size_t)sub.nrows * sizeof(uint32_t),
                                (size_t)sub.ncols, hipMemcpyHostToDevice, st));
    nm = f->d_stage;
  }
  const int n_src = (int)(f->h_src.size() / 3);
  hipLaunchKernelGGL(artp::field_update_sources_kernel, dim3((unsigned)((n_src + 63) / 64)), dim3(64), 0, st, G, sub,
                     (const uint32_t*)f->d_mask, nm, (const int*)f->d_src, n_src, f->d_ucnt);
  const size_t sub_cells = (size_t)sub.nrows * sub.ncols;
  hipLaunchKernelGGL(artp::field_diff_kernel, dim3((unsigned)((sub_cells + 255) / 256)), dim3(256), 0, st, G, sub, nm,
                     f->d_mask, refresh ? 1 : 0, sm, f->geom.rows, f->rect, f->d_h, f->d_dist, f->d_hops, f->d_acc, f->d_ucnt);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(cnt, f->d_ucnt, 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));  // the host copy of the mask is free from here
  return ARTP_OK;
}

// sub_rect of an update or an unblock as a FieldSub (nullptr: the whole rectangle); `who` is the entry point in the error
int field_sub_rect(artp_field* f, const char* who, const int* sub_rect, artp::FieldSub* sub) {
  const artp::FieldGrid& G = f->grid;
  *sub = sub_rect ? artp::FieldSub{sub_rect[0], sub_rect[1], sub_rect[2], sub_rect[3]} : artp::FieldSub{0, 0, G.nrows, G.ncols};
  if (sub->nrows < 1 || sub->ncols < 1 || sub->row0 < 0 || sub->col0 < 0 || sub->row0 > G.nrows - sub->nrows ||
      sub->col0 > G.ncols - sub->ncols) {
    f->ctx->last_error = std::string(who) + ": sub_rect is empty or not inside the field's rectangle";
    return ARTP_ERR_INVALID_ARG;
  }
  return ARTP_OK;
}

// the context's sampler layers have the geometry the field was computed on
bool field_same_map(artp_ctx* c, const artp_field* f) {
  const MapGeom &a = f->geom, &b = c->geom;
  return reach_have_lattice(c) && a.rows == b.rows && a.cols == b.cols && a.len_x == b.len_x && a.len_y == b.len_y &&
         a.pos_x == b.pos_x && a.pos_y == b.pos_y && a.res == b.res;
}

// artp_field_path's poses: the current sampler layers, as a new field would take them
void field_adopt_sampler(artp_ctx* c, artp_field* f) {
  f->sampler = c->sampler;
  f->map_version = c->map_version.load();
}

// The stats of the two weight-table updates and of the shift begin with the members of artp_field_update_stats_t, at its offsets.
#define FIELD_STATS_PREFIX(X)                                                                                         \
  X(changed_words) X(removed_nodes) X(added_nodes) X(dead_nodes) X(hop_dead_nodes) X(unsupport_rounds) X(dist_rounds) \
  X(hop_rounds) X(tile_launches) X(reached_nodes)
#define FIELD_STATS_SAME_OFFSET(m)                                                                              \
  static_assert(offsetof(artp_field_learned_update_stats_t, m) == offsetof(artp_field_update_stats_t, m) &&     \
                    offsetof(artp_field_clearance_update_stats_t, m) == offsetof(artp_field_update_stats_t, m) && \
                    offsetof(artp_field_shift_stats_t, m) == offsetof(artp_field_update_stats_t, m) &&          \
                    offsetof(artp_field_clearance_shift_stats_t, m) == offsetof(artp_field_update_stats_t, m),  \
                "the update stats structs share their first ten members");
FIELD_STATS_PREFIX(FIELD_STATS_SAME_OFFSET)
static_assert(sizeof(artp_field_update_stats_t) == 10 * sizeof(uint64_t), "ten members, and FIELD_STATS_PREFIX names them all");
void field_store_stats(const artp_field_update_stats_t& ps, double, artp_field_update_stats_t* out) { *out = ps; }
template <class Stats>
void field_store_stats(const artp_field_update_stats_t& ps, double passes_ms, Stats* out) {
#define FIELD_STATS_COPY(m) out->m = ps.m;
  FIELD_STATS_PREFIX(FIELD_STATS_COPY)
  out->passes_ms = passes_ms;
}
#undef FIELD_STATS_COPY
#undef FIELD_STATS_SAME_OFFSET
#undef FIELD_STATS_PREFIX

// the tiles flagged in d_wacc counted into d_ucnt[6]; cnt[5 .. 5 + n) read from the device (synchronises)
int field_weight_counts(artp_field* f, unsigned long long* cnt, int n) {
  artp_ctx* c = f->ctx;
  hipLaunchKernelGGL(artp::field_count_flags_kernel, dim3((unsigned)((f->n_tiles + 255) / 256)), dim3(256), 0, c->lane->stream,
                     (uint32_t)f->n_tiles, (const unsigned*)f->d_wacc, f->d_ucnt);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(cnt + 5, f->d_ucnt + 5, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->lane->stream));
  HIP_TRY(c, hipStreamSynchronize(c->lane->stream));
  return ARTP_OK;
}

// The update of a field of any kind behind its entry point's checks: the scratch, the diff of
// new_mask inside sub (nullptr: no diff) behind the test of the sources, the kind's own step, the four passes, the
// sampler adopted where it fits the field (adopt), the stats stored.  middle(cnt, us, run) is the kind's step: cnt = the
// counts of d_ucnt read so far, us = its stats to complete; it sets *run when the passes are to run.  `who` is the entry
// point in the error.  A refusal writes nothing; a failure later leaves the field undefined.
// before() runs behind the cleared flags and counts and in front of the diff: artp_field_shift's move, which flags tiles
// in d_acc and counts into d_ucnt[5 ..] as the diff does (its own refusals are behind it by then).
template <class Stats, class Before, class Middle>
int field_update_run(artp_field* f, const char* who, const uint32_t* new_mask, int mask_on_device, const artp::FieldSub& sub,
                     bool refresh, bool adopt, Stats* stored, Before&& before, Middle&& middle) {
  artp_ctx* c = f->ctx;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->lane->stream;
  const bool wtab = artp::field_has_wtab(f->grid);
  ARTP_TRY(field_update_scratch(f, new_mask && !mask_on_device, wtab));
  HIP_TRY(c, hipMemsetAsync(f->d_acc, 0, f->n_tiles * sizeof(unsigned), st));
  if (wtab) HIP_TRY(c, hipMemsetAsync(f->d_wacc, 0, f->n_tiles * sizeof(unsigned), st));
  HIP_TRY(c, hipMemsetAsync(f->d_ucnt, 0, 8 * sizeof(unsigned long long), st));
  unsigned long long cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  ARTP_TRY(before());
  if (new_mask) {
    ARTP_TRY(field_update_diff(f, new_mask, mask_on_device, sub, refresh, refresh ? c->sampler : f->sampler, cnt));
    if (cnt[4]) {
      c->last_error = std::string(who) + ": a source is no longer a node of the mask (the field is unchanged)";
      return ARTP_ERR_INVALID_ARG;
    }
  }
  artp_field_update_stats_t ps{};
  ps.changed_words = cnt[0];
  ps.removed_nodes = cnt[1];
  ps.added_nodes = cnt[2];
  ps.reached_nodes = f->stats.reached_nodes;
  Stats us{};
  bool run = false;
  ARTP_TRY(middle(cnt, &us, &run));
  double passes_ms = 0.0;
  if (run) {
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = field_update_passes(f, &ps);
    if (rc) {
      (void)hipStreamSynchronize(st);
      return rc;
    }
    passes_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    f->stats.reached_nodes = ps.reached_nodes;  // the other numbers of the compute stay
  }
  if (adopt) field_adopt_sampler(c, f);
  field_store_stats(ps, passes_ms, &us);
  *stored = us;
  return ARTP_OK;
}
template <class Stats, class Middle>
int field_update_run(artp_field* f, const char* who, const uint32_t* new_mask, int mask_on_device, const artp::FieldSub& sub,
                     bool refresh, bool adopt, Stats* stored, Middle&& middle) {
  return field_update_run(f, who, new_mask, mask_on_device, sub, refresh, adopt, stored, [] { return (int)ARTP_OK; },
                          std::forward<Middle>(middle));
}

int field_check_sources(artp_ctx* c, const artp::ReachRect& r, int n_yaw, const int* sources, size_t n_sources) {
  for (size_t i = 0; i < n_sources; ++i) {
    const int sr = sources[3 * i], sc = sources[3 * i + 1], sk = sources[3 * i + 2];
    if (sr < 0 || sr >= r.nrows || sc < 0 || sc >= r.ncols || sk < 0 || sk >= n_yaw) {
      c->last_error = "artp_field_compute: a source lies outside the rectangle or its heading outside [0, n_yaw)";
      return ARTP_ERR_INVALID_ARG;
    }
  }
  return ARTP_OK;
}

// what artp_field_compute refuses about its params
int field_check_params(artp_ctx* c, const artp_field_params& p) {
  if (p.objective != 0 && p.objective != 1) {
    c->last_error = "artp_field_compute: objective must be 0 or 1 (the learned objective has no lattice form)";
    return ARTP_ERR_INVALID_ARG;
  }
  if (!(p.max_lon_vel > 0.0) || !(p.max_lat_vel > 0.0) || !(p.max_ang_vel > 0.0) || !std::isfinite(p.max_lon_vel) ||
      !std::isfinite(p.max_lat_vel) || !std::isfinite(p.max_ang_vel) || p.inner_sweeps < 1) {
    c->last_error = "artp_field_compute: velocities must be positive and finite, inner_sweeps >= 1, n_sources <= 2^24";
    return ARTP_ERR_INVALID_ARG;
  }
  return ARTP_OK;
}

int field_create(artp_ctx* c, const artp_field_params& params, const artp_field_learned_params* lp,
                 const artp_field_clearance_params* cp, const artp::ReachRect& r, const uint32_t* mask, int mask_on_device,
                 const int* sources, size_t n_sources, int reverse, artp_field** out);
artp_field* field_new(artp_ctx* c, const artp_field_params& params, const artp_field_learned_params* lp,
                      const artp_field_clearance_params* cp, const artp::ReachRect& r, int reverse);

// What a learned entry point (who: artp_field_compute_learned, or a batched one of field_many.h) refuses about the context,
// the rectangle and its params, behind the context's lock; *fp = the field params a learned field carries.
int field_learned_checks(artp_ctx* c, const char* who, const artp_field_learned_params& p, int n_yaw, const int* rect,
                         size_t n_sources, artp::ReachRect* r, artp_field_params* fp) {
  if (!c->have_weights) {
    c->last_error = std::string(who) + ": artp_cost_load_weights has not been called";
    return ARTP_ERR_NO_WEIGHTS;
  }
  if (!c->have_features) {
    c->last_error = std::string(who) + ": artp_cost_update_map has not been called";
    return ARTP_ERR_NO_MAP;
  }
  if (!reach_have_lattice(c)) return ARTP_ERR_NO_MAP;
  ARTP_TRY(reach_resolve(c, n_yaw, rect, r));
  const float wt[4] = {p.w_energy, p.w_time, p.w_risk, p.risk_threshold};
  for (float v : wt)
    if (!(v >= 0.0f) || !std::isfinite(v)) {
      c->last_error = std::string(who) + ": the weights and the risk threshold must be non-negative and finite";
      return ARTP_ERR_INVALID_ARG;
    }
  if (p.inner_sweeps < 1 || n_sources > (size_t)1 << 24) {
    c->last_error = std::string(who) + ": inner_sweeps >= 1, n_sources <= 2^24";
    return ARTP_ERR_INVALID_ARG;
  }
  artp_field_params_defaults(fp);  // the velocities are not used
  fp->objective = 2;
  fp->plain_sweeps = p.plain_sweeps;
  fp->inner_sweeps = p.inner_sweeps;
  return ARTP_OK;
}

}  // namespace

extern "C" {

void artp_field_params_defaults(artp_field_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->objective = 0;       // use_directional_cost{false} (params.h:70)
  p->plain_sweeps = 0;
  p->max_lon_vel = 0.5;   // params.h:71-73
  p->max_lat_vel = 0.1;
  p->max_ang_vel = 0.5;
  p->inner_sweeps = 64;
}

int artp_field_compute(artp_ctx* c, const artp_field_params* params, int n_yaw, const int* rect, const uint32_t* mask,
                       int mask_on_device, const int* sources, size_t n_sources, int reverse, artp_field** out) {
  if (out) *out = nullptr;
  if (!c || !params || !mask || !sources || !out || n_sources < 1) return ARTP_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  if (!reach_have_lattice(c)) return ARTP_ERR_NO_MAP;
  artp::ReachRect r;
  int rc = reach_resolve(c, n_yaw, rect, &r);
  if (rc) return rc;
  rc = field_check_params(c, *params);
  if (rc) return rc;
  if (n_sources > (size_t)1 << 24) {
    c->last_error = "artp_field_compute: velocities must be positive and finite, inner_sweeps >= 1, n_sources <= 2^24";
    return ARTP_ERR_INVALID_ARG;
  }
  rc = field_check_sources(c, r, n_yaw, sources, n_sources);
  if (rc) return rc;
  return field_create(c, *params, nullptr, nullptr, r, mask, mask_on_device, sources, n_sources, reverse, out);
}

void artp_field_learned_params_defaults(artp_field_learned_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  artp_roadmap_params rp;
  artp_roadmap_params_defaults(&rp);  // Params::planner.prm_motion_cost.cost_weights and risk_threshold
  p->w_energy = rp.w_energy;
  p->w_time = rp.w_time;
  p->w_risk = rp.w_risk;
  p->risk_threshold = rp.risk_threshold;
  p->plain_sweeps = 0;
  p->inner_sweeps = 64;
}

int artp_field_compute_learned(artp_ctx* c, const artp_field_learned_params* params, int n_yaw, const int* rect,
                               const uint32_t* mask, int mask_on_device, const int* sources, size_t n_sources, int reverse,
                               artp_field** out) {
  if (out) *out = nullptr;
  if (!c || !params || !mask || !sources || !out || n_sources < 1) return ARTP_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  artp::ReachRect r;
  artp_field_params fp;
  int rc = field_learned_checks(c, "artp_field_compute_learned", *params, n_yaw, rect, n_sources, &r, &fp);
  if (rc) return rc;
  rc = field_check_sources(c, r, n_yaw, sources, n_sources);
  if (rc) return rc;
  return field_create(c, fp, params, nullptr, r, mask, mask_on_device, sources, n_sources, reverse, out);
}

int artp_field_learned_stats(artp_field* f, artp_field_learned_stats_t* out) {
  if (!f || !out) return ARTP_ERR_INVALID_ARG;
  *out = f->lstats;
  return ARTP_OK;
}

}  // extern "C"

namespace {

// the part of artp_field_compute, _learned and _clearance behind their checks (lp: objective 2 only; cp: the clearance
// field, params = its base objective's); artp_field_compute_many (field_many.h) makes its fields with field_new
int field_create(artp_ctx* c, const artp_field_params& params, const artp_field_learned_params* lp,
                 const artp_field_clearance_params* cp, const artp::ReachRect& r, const uint32_t* mask, int mask_on_device,
                 const int* sources, size_t n_sources, int reverse, artp_field** out) {
  HIP_TRY(c, hipSetDevice(c->device));
  artp_field* f = field_new(c, params, lp, cp, r, reverse);
  const int rc = field_compute_impl(c, f, mask, mask_on_device, sources, n_sources);
  if (rc) {
    field_free(f);
    return rc;
  }
  *out = f;
  return ARTP_OK;
}

// a field of the rectangle with its grid and sizes, and no device memory yet
artp_field* field_new(artp_ctx* c, const artp_field_params& params, const artp_field_learned_params* lp,
                      const artp_field_clearance_params* cp, const artp::ReachRect& r, int reverse) {
  const int n_yaw = r.n_yaw;
  artp_field* f = new artp_field;
  f->ctx = c;
  f->params = params;
  if (lp) f->lparams = *lp;
  if (cp) f->cparams = *cp;
  f->rect = r;
  f->geom = c->geom;
  f->sampler = c->sampler;
  f->map_version = c->map_version.load();
  f->n_cells = (size_t)r.nrows * r.ncols;
  f->n_nodes = f->n_cells * (size_t)n_yaw;
  artp::FieldGrid& G = f->grid;
  G.nrows = r.nrows;
  G.ncols = r.ncols;
  G.n_yaw = n_yaw;
  G.tiles_r = (r.nrows + artp::FIELD_T - 1) / artp::FIELD_T;
  G.tiles_c = (r.ncols + artp::FIELD_T - 1) / artp::FIELD_T;
  G.objective = cp ? 3 : params.objective;
  G.reverse = reverse ? 1 : 0;
  G.yaw_bits = n_yaw == 32 ? 0xffffffffu : (1u << n_yaw) - 1u;
  G.vlon = params.max_lon_vel;
  G.wrot = params.objective == 0 ? 0.0 : (2.0 * 3.14159265358979323846 / (double)n_yaw) / params.max_ang_vel;
  f->n_tiles = (size_t)G.tiles_r * G.tiles_c;
  f->stats.nodes = f->n_nodes;
  f->stats.tiles = f->n_tiles;
  return f;
}

}  // namespace

extern "C" {

int artp_field_dist(artp_field* f, double* dist_out) {
  if (!f || !dist_out) return ARTP_ERR_INVALID_ARG;
  artp_ctx* c = f->ctx;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(dist_out, f->d_dist, f->n_nodes * sizeof(double), hipMemcpyDeviceToHost, c->lane->stream));
  HIP_TRY(c, hipStreamSynchronize(c->lane->stream));
  return ARTP_OK;
}

int artp_field_dist_dev(artp_field* f, const double** dist_dev) {
  if (!f || !dist_dev) return ARTP_ERR_INVALID_ARG;
  *dist_dev = f->d_dist;
  return ARTP_OK;
}

int artp_field_path(artp_field* f, const int* target, int* nodes_out, double* se3_out, size_t cap, size_t* n,
                    double* cost) {
  if (n) *n = 0;
  if (!f || !target || !n || !cost) return ARTP_ERR_INVALID_ARG;
  artp_ctx* c = f->ctx;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  const artp::FieldGrid& G = f->grid;
  if (target[0] < 0 || target[0] >= G.nrows || target[1] < 0 || target[1] >= G.ncols || target[2] < 0 ||
      target[2] >= G.n_yaw) {
    c->last_error = "artp_field_path: the target lies outside the rectangle or its heading outside [0, n_yaw)";
    return ARTP_ERR_INVALID_ARG;
  }
  if (se3_out && f->map_version != c->map_version.load()) {
    c->last_error = "artp_field_path: the map changed since the field was computed (its poses are gone)";
    return ARTP_ERR_INVALID_ARG;
  }
  if (cap > f->n_nodes) cap = f->n_nodes;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->lane->stream;
  int rc = field_ensure_scratch(f, 3 * cap + 4, 7 * cap + 8);
  if (rc) return rc;
  // d_out: [0] = cost, [1] = the count (as long long), [8 ..] = the poses
  long long* d_n = reinterpret_cast<long long*>(f->d_out + 1);
  hipLaunchKernelGGL(artp::field_path_kernel, dim3(1), dim3(64), 0, st, G, (const uint32_t*)f->d_mask, (const float*)f->d_h,
                     (const double*)f->d_tab, (const uint16_t*)f->d_blk, (const double*)f->d_dist, (const uint32_t*)f->d_hops, target[0], target[1],
                     target[2], (long long)cap, f->d_nodes, d_n, f->d_out);
  HIP_TRY(c, hipGetLastError());
  double head[2];
  HIP_TRY(c, hipMemcpyAsync(head, f->d_out, sizeof(head), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  long long cnt;
  std::memcpy(&cnt, &head[1], sizeof(cnt));
  *cost = head[0];
  if (cnt < 0) {
    c->last_error = "artp_field_path: no tight predecessor (the field is not at its fixed point)";
    return ARTP_ERR_HIP;
  }
  *n = (size_t)cnt;
  if (cnt == 0) return ARTP_OK;  // unreachable: *cost = +inf
  if ((size_t)cnt > cap) {
    c->last_error = "artp_field_path: cap is smaller than the path";
    return ARTP_ERR_CAPACITY;
  }
  if (nodes_out)
    HIP_TRY(c, hipMemcpyAsync(nodes_out, f->d_nodes, 3 * (size_t)cnt * sizeof(int), hipMemcpyDeviceToHost, st));
  if (se3_out) {
    hipLaunchKernelGGL(artp::field_poses_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, f->sampler, f->geom,
                       f->rect, (const int*)f->d_nodes, (size_t)cnt, f->d_out + 8);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(se3_out, f->d_out + 8, 7 * (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(c, hipStreamSynchronize(st));
  return ARTP_OK;
}

int artp_field_edge_costs(artp_field* f, const int* a, const int* b, size_t n, double* cost_out) {
  if (!f || (n && (!a || !b || !cost_out))) return ARTP_ERR_INVALID_ARG;
  if (!n) return ARTP_OK;
  artp_ctx* c = f->ctx;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->lane->stream;
  int rc = field_ensure_scratch(f, 6 * n, n + 8);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(f->d_nodes, a, 3 * n * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(f->d_nodes + 3 * n, b, 3 * n * sizeof(int), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(artp::field_edge_cost_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, f->grid,
                     (const float*)f->d_h, (const double*)f->d_tab, (const uint16_t*)f->d_blk, (const int*)f->d_nodes,
                     (const int*)(f->d_nodes + 3 * n),
                     n, f->d_out);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(cost_out, f->d_out, n * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return ARTP_OK;
}

int artp_field_stats(artp_field* f, artp_field_stats_t* out) {
  if (!f || !out) return ARTP_ERR_INVALID_ARG;
  *out = f->stats;
  return ARTP_OK;
}

int artp_field_update(artp_field* f, const uint32_t* new_mask, int mask_on_device, const int* sub_rect,
                      int refresh_heights) {
  if (!f || !new_mask) return ARTP_ERR_INVALID_ARG;
  artp_ctx* c = f->ctx;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  if (f->grid.objective == 3) {
    c->last_error = "artp_field_update: a clearance-weighted field is not updated by a mask edit alone (it moves clearances, and "
                    "with them the weights, up to radius_cells around it): artp_field_update_clearance takes it";
    return ARTP_ERR_INVALID_ARG;
  }
  if (f->grid.objective == 2) {
    c->last_error = "artp_field_update: a learned field is not updated by a mask edit alone (a map change moves the network's "
                    "features, and with them the weights, far beyond sub_rect): artp_field_update_learned prices it again";
    return ARTP_ERR_INVALID_ARG;
  }
  artp::FieldSub sub;
  ARTP_TRY(field_sub_rect(f, "artp_field_update", sub_rect, &sub));
  const bool same_map = field_same_map(c, f);
  if (refresh_heights && !same_map) {
    c->last_error = "artp_field_update: refresh_heights needs sampler layers of the geometry the field was computed on";
    return ARTP_ERR_INVALID_ARG;
  }
  // the kind's step: none.  The passes run when a word or a height changed.
  return field_update_run(f, "artp_field_update", new_mask, mask_on_device, sub, refresh_heights != 0, same_map, &f->ustats,
                          [](const unsigned long long* cnt, artp_field_update_stats_t*, bool* run) -> int {
                            *run = cnt[0] || cnt[3];
                            return ARTP_OK;
                          });
}

int artp_field_update_stats(artp_field* f, artp_field_update_stats_t* out) {
  if (!f || !out) return ARTP_ERR_INVALID_ARG;
  *out = f->ustats;
  return ARTP_OK;
}

}  // extern "C"

namespace {

// A move that passed field_shift_checks: (si, sj), the sources at their new places, new_mask on the device.
struct FieldMove {
  long long si = 0, sj = 0;
  std::vector<int> moved;
  const uint32_t* nm = nullptr;
  bool moves() const { return si != 0 || sj != 0; }
};

// What artp_field_shift and artp_field_shift_clearance refuse behind the test of the field's kind, in front of the first
// write: the host's tests, then the moved sources against new_mask on the device (field_update_sources_kernel on a copy of
// them).  `who` is the entry point in the error.
int field_shift_checks(artp_field* f, const char* who, const uint32_t* new_mask, int mask_on_device, FieldMove* mv) {
  artp_ctx* c = f->ctx;
  const artp::FieldGrid& G = f->grid;
  if (!reach_have_lattice(c)) return ARTP_ERR_NO_MAP;
  const MapGeom &a = f->geom, &b = c->geom;
  if (a.rows != b.rows || a.cols != b.cols || a.len_x != b.len_x || a.len_y != b.len_y || a.res != b.res) {
    c->last_error = std::string(who) + ": the context's map differs from the field's in rows, cols, lengths or resolution";
    return ARTP_ERR_INVALID_ARG;
  }
  // artp_preprocessed_change's convention: cell (i, j) of the new map lies over cell (i - si, j - sj) of the old one
  const double fi = (b.pos_x - a.pos_x) / b.res, fj = (b.pos_y - a.pos_y) / b.res;
  const bool overlap = std::fabs(fi) < (double)G.nrows && std::fabs(fj) < (double)G.ncols;  // false for a NaN too
  const long long si = overlap ? std::lround(fi) : 0, sj = overlap ? std::lround(fj) : 0;
  std::vector<int> moved(f->h_src);
  bool inside = overlap;
  for (size_t i = 0; i + 2 < moved.size() && inside; i += 3) {
    moved[i] += (int)si;
    moved[i + 1] += (int)sj;
    inside = moved[i] >= 0 && moved[i] < G.nrows && moved[i + 1] >= 0 && moved[i + 1] < G.ncols;
  }
  if (!inside) {
    c->last_error = std::string(who) + ": a source leaves the rectangle with the map's move (the field is unchanged)";
    return ARTP_ERR_INVALID_ARG;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->lane->stream;
  ARTP_TRY(field_update_scratch(f, !mask_on_device));
  ARTP_TRY(field_ensure_scratch(f, moved.size(), 8));
  const uint32_t* nm = new_mask;
  if (!mask_on_device) {
    HIP_TRY(c, hipMemcpyAsync(f->d_stage, new_mask, f->n_cells * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    nm = f->d_stage;
  }
  const artp::FieldSub whole{0, 0, G.nrows, G.ncols};
  const int n_src = (int)(moved.size() / 3);
  unsigned long long gone = 0;
  HIP_TRY(c, hipMemcpyAsync(f->d_nodes, moved.data(), moved.size() * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemsetAsync(f->d_ucnt, 0, 8 * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(artp::field_update_sources_kernel, dim3((unsigned)((n_src + 63) / 64)), dim3(64), 0, st, G, whole,
                     (const uint32_t*)f->d_mask, nm, (const int*)f->d_nodes, n_src, f->d_ucnt);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(&gone, f->d_ucnt + 4, sizeof(gone), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));  // the host copy of the mask is free from here
  if (gone) {
    c->last_error = std::string(who) + ": a moved source is not a node of new_mask (the field is unchanged)";
    return ARTP_ERR_INVALID_ARG;
  }
  mv->si = si;
  mv->sj = sj;
  mv->moved = std::move(moved);
  mv->nm = nm;
  return ARTP_OK;
}

// The move itself, as field_update_run's before(): the geometry and the sources adopted, then dist, hops, mask words,
// heights and blocked words moved through scratch and copied back.  tm marks 0 and 1 around the device work of a move.
int field_shift_move(artp_field* f, const FieldMove& mv, StreamTimer<2>& tm) {
  artp_ctx* c = f->ctx;
  hipStream_t st = c->lane->stream;
  const artp::FieldGrid& G = f->grid;
  f->geom = c->geom;
  if (!mv.moves()) return ARTP_OK;
  const artp::FieldShift sh{(int)mv.si, (int)mv.sj, mv.si + mv.sj * (long long)G.nrows};
  const size_t blk_words = (f->n_nodes + 1) / 2 * 2;  // field_blocked_alloc's
  ARTP_TRY(field_lazy(f, &f->d_shift, f->n_nodes * sizeof(uint32_t) + f->n_cells * 8 + blk_words * sizeof(uint16_t)));
  uint32_t* hops_o = reinterpret_cast<uint32_t*>(f->d_shift);
  uint32_t* mask_o = hops_o + f->n_nodes;
  float* h_o = reinterpret_cast<float*>(mask_o + f->n_cells);
  uint16_t* blk_o = reinterpret_cast<uint16_t*>(h_o + f->n_cells);
  f->h_src = mv.moved;
  HIP_TRY(c, hipMemcpyAsync(f->d_src, f->h_src.data(), f->h_src.size() * sizeof(int), hipMemcpyHostToDevice, st));
  tm.mark(0);
  hipLaunchKernelGGL(artp::field_shift_nodes_kernel, dim3((unsigned)((f->n_nodes + 255) / 256)), dim3(256), 0, st, G, sh,
                     (const double*)f->d_dist, (const uint32_t*)f->d_hops, (const uint16_t*)f->d_blk, f->d_snap, hops_o,
                     blk_o, f->d_ucnt);
  hipLaunchKernelGGL(artp::field_shift_cells_kernel, dim3((unsigned)((f->n_cells + 255) / 256)), dim3(256), 0, st, G, sh,
                     c->sampler, c->geom.rows, f->rect, (const uint32_t*)f->d_mask, (const float*)f->d_h, mask_o, h_o,
                     f->d_acc, f->d_ucnt);
  HIP_TRY(c, hipGetLastError());
  // dist stays the buffer artp_field_dist_dev handed out
  HIP_TRY(c, hipMemcpyAsync(f->d_dist, f->d_snap, f->n_nodes * sizeof(double), hipMemcpyDeviceToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(f->d_hops, hops_o, f->n_nodes * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(f->d_mask, mask_o, f->n_cells * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(f->d_h, h_o, f->n_cells * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (f->d_blk)
    HIP_TRY(c, hipMemcpyAsync(f->d_blk, blk_o, f->n_nodes * sizeof(uint16_t), hipMemcpyDeviceToDevice, st));
  tm.mark(1);
  return ARTP_OK;
}

// The move's counts, in the kind's step: d_ucnt[5 .. 7] read into cnt (synchronises), the blocked moves that stayed
// adopted, the shift's members of the stats filled.
template <class Stats>
int field_shift_counts(artp_field* f, const FieldMove& mv, StreamTimer<2>& tm, unsigned long long* cnt, Stats* us) {
  artp_ctx* c = f->ctx;
  hipStream_t st = c->lane->stream;
  const artp::FieldGrid& G = f->grid;
  if (mv.moves()) {
    HIP_TRY(c, hipMemcpyAsync(cnt + 5, f->d_ucnt + 5, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (f->d_blk) {
      us->dropped_blocked = f->n_blocked - cnt[7];
      f->n_blocked = cnt[7];
    }
  }
  const long long ai = mv.si < 0 ? -mv.si : mv.si, aj = mv.sj < 0 ? -mv.sj : mv.sj;
  us->shift_rows = mv.si;
  us->shift_cols = mv.sj;
  us->kept_cells = (uint64_t)(G.nrows - ai) * (uint64_t)(G.ncols - aj);
  us->left_nodes = cnt[5];
  us->move_ms = tm.ms(0, 1, mv.moves());
  return ARTP_OK;
}

}  // namespace

extern "C" {

// DESIGN.md section 20.  Every refusal comes in front of the first write (field_shift_checks), then field_update_run with
// the move in front of its diff.
int artp_field_shift(artp_field* f, const uint32_t* new_mask, int mask_on_device, int refresh_heights) {
  if (!f || !new_mask) return ARTP_ERR_INVALID_ARG;
  artp_ctx* c = f->ctx;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  const artp::FieldGrid& G = f->grid;
  if (artp::field_has_wtab(G)) {
    c->last_error = "artp_field_shift: a learned or a clearance-weighted field keeps a weight per node and move, which would "
                    "have to move too: compute it anew on the new map (a clearance-weighted field: artp_field_shift_clearance)";
    return ARTP_ERR_INVALID_ARG;
  }
  FieldMove mv;
  ARTP_TRY(field_shift_checks(f, "artp_field_shift", new_mask, mask_on_device, &mv));
  const artp::FieldSub whole{0, 0, G.nrows, G.ncols};
  StreamTimer<2> tm(c->lane->stream);
  return field_update_run(
      f, "artp_field_shift", mv.nm, 1, whole, refresh_heights != 0, true, &f->shstats,
      [&]() -> int { return field_shift_move(f, mv, tm); },
      // the kind's step: the move's counts.  After a move the passes always run: the border may have lost its support.
      [&](unsigned long long* cnt, artp_field_shift_stats_t* us, bool* run) -> int {
        ARTP_TRY(field_shift_counts(f, mv, tm, cnt, us));
        *run = mv.moves() || cnt[0] || cnt[3];
        return ARTP_OK;
      });
}

int artp_field_shift_stats(artp_field* f, artp_field_shift_stats_t* out) {
  if (!f || !out) return ARTP_ERR_INVALID_ARG;
  *out = f->shstats;
  return ARTP_OK;
}

int artp_field_update_learned(artp_field* f, const uint32_t* new_mask, int mask_on_device, const int* sub_rect) {
  if (!f) return ARTP_ERR_INVALID_ARG;
  artp_ctx* c = f->ctx;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  if (f->grid.objective != 2) {
    c->last_error = "artp_field_update_learned: not a field of artp_field_compute_learned (artp_field_update and "
                    "artp_field_update_clearance take the others)";
    return ARTP_ERR_INVALID_ARG;
  }
  if (!c->have_weights) {
    c->last_error = "artp_field_update_learned: artp_cost_load_weights has not been called";
    return ARTP_ERR_NO_WEIGHTS;
  }
  if (!c->have_features) {
    c->last_error = "artp_field_update_learned: artp_cost_update_map has not been called";
    return ARTP_ERR_NO_MAP;
  }
  artp::FieldSub sub;
  ARTP_TRY(field_sub_rect(f, "artp_field_update_learned", new_mask ? sub_rect : nullptr, &sub));
  if (!field_same_map(c, f)) {
    c->last_error = "artp_field_update_learned: the sampler layers do not have the geometry the field was computed on";
    return ARTP_ERR_INVALID_ARG;
  }
  // the kind's step: what a new field would hold -- the current sampler layers and their heights over the whole rectangle --
  // then every slot priced again (a slot whose bits change flags its tile).  The passes run when a word or a slot changed.
  return field_update_run(
      f, "artp_field_update_learned", new_mask, mask_on_device, sub, false, true, &f->lustats,
      [&](unsigned long long* cnt, artp_field_learned_update_stats_t* us, bool* run) -> int {
        field_adopt_sampler(c, f);
        hipLaunchKernelGGL(artp::field_heights_kernel, dim3((unsigned)((f->n_cells + 255) / 256)), dim3(256), 0, c->lane->stream,
                           f->sampler, f->geom, f->rect, f->d_h);
        HIP_TRY(c, hipGetLastError());
        double ms[3] = {0.0, 0.0, 0.0};
        uint64_t chunks = 0;
        ARTP_TRY(field_learned_table(c, f, true, ms, &chunks));
        ARTP_TRY(field_weight_counts(f, cnt, 2));
        us->repriced_slots = artp::field_wtab_slots(f->grid);
        us->changed_slots = cnt[5];
        us->weight_tiles = cnt[6];
        us->rows_ms = ms[0];
        us->query_ms = ms[1];
        us->reprice_ms = ms[2];
        *run = cnt[0] || cnt[5];
        return ARTP_OK;
      });
}

int artp_field_learned_update_stats(artp_field* f, artp_field_learned_update_stats_t* out) {
  if (!f || !out) return ARTP_ERR_INVALID_ARG;
  *out = f->lustats;
  return ARTP_OK;
}

void artp_field_destroy(artp_field* f) {
  if (!f) return;
  (void)hipSetDevice(f->ctx->device);
  field_free(f);
}

}  // extern "C"
