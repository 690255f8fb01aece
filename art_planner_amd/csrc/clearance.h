// clearance.h -- clearance maps and clearance-weighted cost-to-go fields (include/artp_c.h artp_clearance_map*,
// artp_field_compute_clearance, artp_field_clearance).
//
// d2[node] (uint16, node order of reach.h and field.h) = the exact squared distance, in cells, from node (r, c, k) to the
// nearest OBSTACLE of heading k within radius_cells R: a cell whose word lacks one of the bits k - s .. k + s (mod n_yaw),
// s = yaw_spread, and -- with outside_is_obstacle -- every cell outside the rectangle.  0 where bit k of the node's own
// word is clear, 0xffff where no obstacle lies within R.
//   clearance_map_kernel          a workgroup of 256 lanes owns a 16 x 16 tile (field.h's tiling).  It stages the ERODED
//                                 words of the tile and a halo of R cells in LDS: bit k of an eroded word is set iff the
//                                 bits k - s .. k + s of the word are (an AND of rotations within the low n_yaw bits), so
//                                 "obstacle for heading k" is "bit k clear", for all headings of a cell in one word.  One
//                                 lane per cell walks the offsets of the disc in order of increasing d^2 (the host's list):
//                                 hit = ~word & pending answers every heading in hit with this d^2.  The answers go to an
//                                 LDS staging tile, each (cell, heading) once, and leave as rows of 16 n_yaw neighbours.
//   field_clearance_table_kernel  one lane per slot of objective 2's weight table (field_slot_edge): the base cost of
//                                 artp_field_compute in the field's direction (field_pull_cost) times
//                                 1 + gain max(pen(a), pen(b)), pen(v) = max(0, 1 - res sqrt(d2[v]) / margin), 0 at 0xffff.
// The field (objective id 3 inside the library) is searched by the table-driven kernels of the learned field, unchanged.
// artp_field_update_clearance brings such a field to an edited mask in place: the diff of
// artp_field_update, then
//   clearance_window_kernel          clearance_map_kernel's tile (clearance_tile, the one body of both) on the tiles that
//                                    intersect sub_rect grown by R cells, written into the field's own d2; counts the
//                                    nodes whose value changed
//   field_clearance_reprice_kernel   field_clearance_table_kernel's price (field_clearance_price, shared) on the tiles
//                                    that intersect sub_rect grown by R + 1 cells, against the slot's old bit pattern: a
//                                    slot that differs is written and flags its tile, as field_learned_reprice_kernel does
// and the four passes of artp_field_update from the flagged tiles.  artp_field_update and artp_field_update_learned
// refuse the field.
// artp_field_shift_clearance carries such a field across a map move: the move and the diff of
// artp_field_shift, clearance_map_kernel over the whole rectangle, then
//   field_clearance_shift_table_kernel   every slot priced on the new state into a second table, against the weight its own
//                                        node carried for the same move in the old table (+inf where that node entered)
// and the same passes.  The second table is allocated by the first call that moves and kept until artp_field_destroy;
// the two tables swap roles after every move (d_tab never leaves the library).
#pragma once

namespace artp {

constexpr int CLEAR_MAX_R = 32;
constexpr int CLEAR_PITCH = FIELD_T * FIELD_T + 2;  // uint16 per heading of the staging tile: 129 words, one bank a heading
constexpr uint16_t CLEAR_NONE = 0xffffu;

struct ClearGrid {
  int nrows, ncols, n_yaw;
  int tiles_r;
  int R, spread, outside;
  int W;       // 16 + 2 R: edge of the staged window in cells
  int S;       // its column pitch in words
  uint32_t n_off;
  uint32_t yaw_bits;
};

// Column pitch of the window: the least S >= W with S = 16 (mod 32).  A wave holds 16 rows x 4 columns of the tile and a
// 32-lane group of ds_read_b32 two of those columns: their two runs of 16 words then lie in opposite halves of the 32 banks,
// at every offset of the walk (all lanes of a wave read the same offset, so the window only shifts).
__host__ __device__ constexpr int clearance_pitch(int W) { return ((W - 16 + 31) / 32) * 32 + 16; }

inline size_t clearance_lds(int R, int n_yaw) {
  const int W = FIELD_T + 2 * R;
  return (size_t)clearance_pitch(W) * W * sizeof(uint32_t) + (size_t)n_yaw * CLEAR_PITCH * sizeof(uint16_t);
}

// bit k of the result = bits k - s .. k + s (mod n) of w (w within its low n bits; 1 <= t <= s <= n / 2 keeps the shifts in 1 .. 31)
__device__ __forceinline__ uint32_t clearance_erode(uint32_t w, int n, int s, uint32_t yaw_bits) {
  uint32_t e = w;
  for (int t = 1; t <= s; ++t) e &= ((w << t) | (w >> (n - t))) & ((w >> t) | (w << (n - t)));
  return e & yaw_bits;
}

// The tile whose first cell is (r0, c0), by its workgroup.  offs[i] = (dr + dc S) << 16 | d2 of the i-th offset of the
// disc, d2 ascending, (0, 0) first.  COUNT = false: every node of the tile is written.  COUNT = true (the update's
// window): d2 holds an earlier map; only a word that differs is written, and *changed += their number, one atomic per wave.
template <bool COUNT>
__device__ __forceinline__ void clearance_tile(const ClearGrid& G, const uint32_t* __restrict__ mask,
                                               const int32_t* __restrict__ offs, uint16_t* __restrict__ d2, int r0, int c0,
                                               unsigned long long* __restrict__ changed) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint32_t* win = reinterpret_cast<uint32_t*>(smem);
  uint16_t* stage = reinterpret_cast<uint16_t*>(win + (size_t)G.S * G.W);
  const int tid = threadIdx.x;
  const int ny = G.n_yaw;

  for (int e = tid; e < G.W * G.W; e += 256) {
    const int wr = e % G.W, wc = e / G.W;
    const int r = r0 - G.R + wr, c = c0 - G.R + wc;
    uint32_t w = G.outside ? 0u : G.yaw_bits;  // outside the rectangle: an obstacle of every heading, or of none
    if (r >= 0 && r < G.nrows && c >= 0 && c < G.ncols)
      w = clearance_erode(mask[(size_t)r + (size_t)c * G.nrows] & G.yaw_bits, ny, G.spread, G.yaw_bits);
    win[wr + wc * G.S] = w;
  }
  __syncthreads();

  const int tr = tid & (FIELD_T - 1), tc = tid >> 4;
  const bool in = r0 + tr < G.nrows && c0 + tc < G.ncols;
  const uint32_t mw = in ? mask[(size_t)(r0 + tr) + (size_t)(c0 + tc) * G.nrows] & G.yaw_bits : 0u;
  const int me = (tr + G.R) + (tc + G.R) * G.S;
  uint16_t* mine = stage + tid;
  uint32_t pending = mw;  // the headings that are nodes and have no answer yet
  for (uint32_t i = 0; i < G.n_off && pending; ++i) {
    const int32_t o = offs[i];
    uint32_t hit = ~win[me + (o >> 16)] & pending;
    pending &= ~hit;
    while (hit) {
      const int k = __ffs((int)hit) - 1;
      hit &= hit - 1u;
      mine[k * CLEAR_PITCH] = (uint16_t)(o & 0xffff);
    }
  }
  while (pending) {  // no obstacle within R
    const int k = __ffs((int)pending) - 1;
    pending &= pending - 1u;
    mine[k * CLEAR_PITCH] = CLEAR_NONE;
  }
  uint32_t none = ~mw & G.yaw_bits;  // not a node
  while (none) {
    const int k = __ffs((int)none) - 1;
    none &= none - 1u;
    mine[k * CLEAR_PITCH] = 0;
  }
  __syncthreads();

  unsigned n_changed = 0;  // COUNT: of this wave (the loop's trip count is the same for every lane of the workgroup)
  for (int e = tid; e < FIELD_T * FIELD_T * ny; e += 256) {
    const int ci = e / ny, k = e - ci * ny;
    const int r = r0 + (ci & (FIELD_T - 1)), c = c0 + (ci >> 4);
    const bool inside = r < G.nrows && c < G.ncols;
    if (!COUNT) {
      if (inside) d2[((size_t)r + (size_t)c * G.nrows) * ny + k] = stage[k * CLEAR_PITCH + ci];
      continue;
    }
    bool ch = false;
    if (inside) {
      const size_t node = ((size_t)r + (size_t)c * G.nrows) * ny + k;
      const uint16_t v = stage[k * CLEAR_PITCH + ci];
      ch = d2[node] != v;
      if (ch) d2[node] = v;
    }
    n_changed += (unsigned)__popcll(__ballot(ch));
  }
  if (COUNT && n_changed && (tid & 63) == 0) atomicAdd(changed, (unsigned long long)n_changed);
}

// the whole rectangle: workgroup = tile, in field.h's order of tiles
__global__ void __launch_bounds__(256)
clearance_map_kernel(ClearGrid G, const uint32_t* __restrict__ mask, const int32_t* __restrict__ offs, uint16_t* __restrict__ d2) {
  const int tile = blockIdx.x;
  clearance_tile<false>(G, mask, offs, d2, (tile % G.tiles_r) * FIELD_T, (tile / G.tiles_r) * FIELD_T, nullptr);
}

// A window of tiles of a rectangle (artp_field_update_clearance): wn_r x (gridDim.x / wn_r) tiles from tile (t_r0, t_c0).
struct ClearWindow {
  int t_r0, t_c0, wn_r;
};
__global__ void __launch_bounds__(256)
clearance_window_kernel(ClearGrid G, ClearWindow w, const uint32_t* __restrict__ mask, const int32_t* __restrict__ offs,
                        uint16_t* __restrict__ d2, unsigned long long* __restrict__ changed) {
  const int b = blockIdx.x;
  clearance_tile<true>(G, mask, offs, d2, (w.t_r0 + b % w.wn_r) * FIELD_T, (w.t_c0 + b / w.wn_r) * FIELD_T, changed);
}

struct ClearWeight {
  double res, margin, gain;
};

__device__ __forceinline__ double clearance_pen(const ClearWeight& p, uint16_t d2) {
  if (d2 == CLEAR_NONE) return 0.0;
  return fmax(0.0, 1.0 - (p.res * sqrt((double)d2)) / p.margin);
}

// G carries the BASE objective (0 or 1) here: field_pull_cost prices with it.  tab: the (m, k) table of that objective.
// The weight of slot s of the table, for the build and for the update's repricing: +inf where the edge does not exist.
__device__ __forceinline__ double field_clearance_price(const FieldGrid& G, const uint32_t* __restrict__ mask,
                                                        const float* __restrict__ h, const double* __restrict__ tab,
                                                        const uint16_t* __restrict__ d2, const ClearWeight& p, size_t s) {
  uint32_t from, to;
  if (!field_slot_edge(G, mask, s, &from, &to)) return INFINITY;
  const uint32_t v = G.reverse ? from : to, u = G.reverse ? to : from;  // the slot's own node and its neighbour
  const uint32_t cv = v / (uint32_t)G.n_yaw, cu = u / (uint32_t)G.n_yaw;
  const int k = (int)(v - cv * (uint32_t)G.n_yaw);
  const int j = (int)((s / (FIELD_T * FIELD_T)) % 10);
  const double base = field_pull_cost(G, tab, j, k, h[cv], h[cu]);
  return base * (1.0 + p.gain * fmax(clearance_pen(p, d2[from]), clearance_pen(p, d2[to])));
}

__global__ void __launch_bounds__(256)
field_clearance_table_kernel(FieldGrid G, const uint32_t* __restrict__ mask, const float* __restrict__ h,
                             const double* __restrict__ tab, const uint16_t* __restrict__ d2, ClearWeight p, size_t slots,
                             double* __restrict__ wtab) {
  const size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= slots) return;
  wtab[s] = field_clearance_price(G, mask, h, tab, d2, p, s);
}

// artp_field_update_clearance: the same price against the slot's old BIT PATTERN, on a window of tiles (w as
// clearance_window_kernel takes it).  A tile's share of the table is 10 n_yaw runs of 256 slots: workgroup b prices run
// b % (10 n_yaw) of window tile b / (10 n_yaw), so every lane has a slot and the slots of a workgroup lie in one tile.
// Only a slot that differs is written; its tile is flagged in acc (the seeds of the passes) and in wacc (weight_tiles) --
// a slot is read by its own node's rule alone, which runs in its own tile alone.  cnt[5] += changed slots, one atomic per wave.
__global__ void __launch_bounds__(256)
field_clearance_reprice_kernel(FieldGrid G, ClearWindow w, const uint32_t* __restrict__ mask, const float* __restrict__ h,
                               const double* __restrict__ tab, const uint16_t* __restrict__ d2, ClearWeight p,
                               double* __restrict__ wtab, unsigned* __restrict__ acc, unsigned* __restrict__ wacc,
                               unsigned long long* __restrict__ cnt) {
  const uint32_t runs = 10u * (uint32_t)G.n_yaw;
  const uint32_t wt = blockIdx.x / runs, run = blockIdx.x - wt * runs;
  const size_t tile = (size_t)(w.t_r0 + (int)(wt % (uint32_t)w.wn_r)) + (size_t)(w.t_c0 + (int)(wt / (uint32_t)w.wn_r)) * (size_t)G.tiles_r;
  const size_t s = (tile * runs + run) * (FIELD_T * FIELD_T) + threadIdx.x;
  const double price = field_clearance_price(G, mask, h, tab, d2, p, s);
  const bool ch = __double_as_longlong(price) != __double_as_longlong(wtab[s]);
  if (ch) wtab[s] = price;
  const unsigned long long b = __ballot(ch);
  if (b && (threadIdx.x & 63) == 0) {
    acc[tile] = 1u;
    wacc[tile] = 1u;
    atomicAdd(&cnt[5], (unsigned long long)__popcll(b));
  }
}

// artp_field_shift_clearance: the map moved by (sh.si, sh.sj) cells, mask, h and d2 hold the new state, old_tab the table
// of the state before the move.  field_clearance_reprice_kernel's mapping over all tiles: workgroup b prices run
// b % (10 n_yaw) = (k, j) of tile b / (10 n_yaw), one slot a lane.  The slot's own node (r, c, k) was node (r - si, c - sj, k):
// its old weight is that node's slot of the same move when the old cell lay inside the rectangle, +inf otherwise (an entered
// cell had no edge; a padded slot of a last tile prices to +inf and had +inf: nothing is read for it).  The 16 lanes of a
// tile column read 16 consecutive slots of an old tile's row, split over at most two tiles.  Every slot of wtab is
// written; a slot whose bit pattern differs from its old one flags its tile in acc and wacc, cnt[5] += their number, one
// atomic per wave.
__global__ void __launch_bounds__(256)
field_clearance_shift_table_kernel(FieldGrid G, FieldShift sh, const uint32_t* __restrict__ mask, const float* __restrict__ h,
                                   const double* __restrict__ tab, const uint16_t* __restrict__ d2, ClearWeight p,
                                   const double* __restrict__ old_tab, double* __restrict__ wtab, unsigned* __restrict__ acc,
                                   unsigned* __restrict__ wacc, unsigned long long* __restrict__ cnt) {
  const uint32_t runs = 10u * (uint32_t)G.n_yaw;
  const uint32_t tile = blockIdx.x / runs, run = blockIdx.x - tile * runs;
  const size_t s = ((size_t)tile * runs + run) * (FIELD_T * FIELD_T) + threadIdx.x;
  const double price = field_clearance_price(G, mask, h, tab, d2, p, s);
  const int r = (int)(tile % (uint32_t)G.tiles_r) * FIELD_T + (int)(threadIdx.x & (FIELD_T - 1));
  const int c = (int)(tile / (uint32_t)G.tiles_r) * FIELD_T + (int)(threadIdx.x >> 4);
  const int k = (int)(run / 10u), j = (int)(run - 10u * (uint32_t)k);
  double old = INFINITY;
  if (r < G.nrows && c < G.ncols && field_shift_inside(G, r - sh.si, c - sh.sj))
    old = old_tab[field_wtab_index(G, r - sh.si, c - sh.sj, k, j)];
  wtab[s] = price;
  const unsigned long long b = __ballot(__double_as_longlong(price) != __double_as_longlong(old));
  if (b && (threadIdx.x & 63) == 0) {
    acc[tile] = 1u;
    wacc[tile] = 1u;
    atomicAdd(&cnt[5], (unsigned long long)__popcll(b));
  }
}

}  // namespace artp

namespace {

int clearance_check(artp_ctx* c, const artp_clearance_params& p, int n_yaw) {
  if (n_yaw < 1 || n_yaw > artp::ARTP_REACH_MAX_YAW) {
    c->last_error = "n_yaw must lie in [1, 32]";
    return ARTP_ERR_INVALID_ARG;
  }
  if (p.radius_cells < 1 || p.radius_cells > artp::CLEAR_MAX_R || p.yaw_spread < 0 || p.yaw_spread > n_yaw / 2 ||
      (p.outside_is_obstacle != 0 && p.outside_is_obstacle != 1)) {
    c->last_error = "clearance: radius_cells must lie in [1, 32], yaw_spread in [0, n_yaw / 2], outside_is_obstacle be 0 or 1";
    return ARTP_ERR_INVALID_ARG;
  }
  return ARTP_OK;
}

// The offsets of the disc of radius R in order of increasing d^2, on the device: built the first time a context meets R,
// then kept unchanged until artp_destroy (a kernel in flight on any stream may be reading it).
int clearance_offsets(artp_ctx* c, int R) {
  if (c->clear_offs[R].get()) return ARTP_OK;
  const int S = artp::clearance_pitch(artp::FIELD_T + 2 * R);
  std::vector<int32_t> offs;
  for (int dc = -R; dc <= R; ++dc)
    for (int dr = -R; dr <= R; ++dr)
      if (dr * dr + dc * dc <= R * R) offs.push_back((int32_t)((uint32_t)(dr + dc * S) << 16) | (dr * dr + dc * dc));
  std::stable_sort(offs.begin(), offs.end(), [](int32_t a, int32_t b) { return (a & 0xffff) < (b & 0xffff); });
  DeviceBuffer<int32_t>& d = c->clear_offs[R];
  HIP_TRY(c, d.reserve(offs.size() * sizeof(int32_t)));
  if (hipMemcpy(d.get(), offs.data(), offs.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
    (void)d.reset();
    c->last_error = "clearance: copying the offset list failed";
    return ARTP_ERR_HIP;
  }
  c->clear_n[R] = (uint32_t)offs.size();
  return ARTP_OK;
}

// The tiles that intersect sub grown by `grow` cells and clipped to the rectangle, as a window of tiles.
struct ClearTiles {
  artp::ClearWindow w;
  size_t n;  // tiles of the window
};
ClearTiles clearance_window(const artp::FieldGrid& G, const artp::FieldSub& sub, int grow) {
  const int T = artp::FIELD_T;
  const int r_lo = std::max(sub.row0 - grow, 0) / T, r_hi = std::min(sub.row0 + sub.nrows - 1 + grow, G.nrows - 1) / T;
  const int c_lo = std::max(sub.col0 - grow, 0) / T, c_hi = std::min(sub.col0 + sub.ncols - 1 + grow, G.ncols - 1) / T;
  return ClearTiles{artp::ClearWindow{r_lo, c_lo, r_hi - r_lo + 1}, (size_t)(r_hi - r_lo + 1) * (size_t)(c_hi - c_lo + 1)};
}

// clearance_map_kernel over a rectangle of device words into device d2, on the context's stream; the checks are the caller's.
// win: clearance_window_kernel on that window of tiles instead, d_d2 holding an earlier map, *d_changed += the nodes that changed.
int clearance_run(artp_ctx* c, const artp_clearance_params& p, int n_yaw, int nrows, int ncols, const uint32_t* d_mask,
                  uint16_t* d_d2, const ClearTiles* win = nullptr, unsigned long long* d_changed = nullptr) {
  const int R = p.radius_cells;
  ARTP_TRY(clearance_offsets(c, R));
  artp::ClearGrid G;
  G.nrows = nrows;
  G.ncols = ncols;
  G.n_yaw = n_yaw;
  G.tiles_r = (nrows + artp::FIELD_T - 1) / artp::FIELD_T;
  G.R = R;
  G.spread = p.yaw_spread;
  G.outside = p.outside_is_obstacle;
  G.W = artp::FIELD_T + 2 * R;
  G.S = artp::clearance_pitch(G.W);
  G.n_off = c->clear_n[R];
  G.yaw_bits = n_yaw == 32 ? 0xffffffffu : (1u << n_yaw) - 1u;
  const size_t tiles = (size_t)G.tiles_r * ((ncols + artp::FIELD_T - 1) / artp::FIELD_T);
  if (win)
    hipLaunchKernelGGL(artp::clearance_window_kernel, dim3((unsigned)win->n), dim3(256), artp::clearance_lds(R, n_yaw), c->lane->stream,
                       G, win->w, d_mask, (const int32_t*)c->clear_offs[R].get(), d_d2, d_changed);
  else
    hipLaunchKernelGGL(artp::clearance_map_kernel, dim3((unsigned)tiles), dim3(256), artp::clearance_lds(R, n_yaw), c->lane->stream, G,
                       d_mask, (const int32_t*)c->clear_offs[R].get(), d_d2);
  HIP_TRY(c, hipGetLastError());
  return ARTP_OK;
}

int clearance_map_args(artp_ctx* c, const artp_clearance_params* p, int n_yaw, int nrows, int ncols) {
  ARTP_TRY(clearance_check(c, *p, n_yaw));
  if (nrows < 1 || ncols < 1 || (uint64_t)nrows * (uint64_t)ncols * (uint64_t)n_yaw >= (1ull << 32)) {
    c->last_error = "clearance: nrows and ncols must be positive and nrows * ncols * n_yaw stay below 2^32";
    return ARTP_ERR_INVALID_ARG;
  }
  return ARTP_OK;
}

// artp_field_compute_clearance's part of field_compute_impl: the field's d2 from its own mask, then the weight table.
// tab: the host's (m, k) table of the base objective; its device copy stays with the field (artp_field_update_clearance
// prices with it again).
int field_clearance_build(artp_ctx* c, artp_field* f, const double* tab) {
  hipStream_t st = c->lane->stream;
  const artp_field_clearance_params& cp = f->cparams;
  HIP_TRY(c, f->mem.alloc(&f->d_btab, artp::FIELD_TAB));
  double* d_tab = f->d_btab;
  HIP_TRY(c, f->mem.alloc(&f->d_d2, f->n_nodes));
  HIP_TRY(c, hipMemcpyAsync(d_tab, tab, artp::FIELD_TAB * sizeof(double), hipMemcpyHostToDevice, st));
  StreamTimer<3> tm(st);
  tm.mark(0);
  int rc = clearance_run(c, cp.clearance, f->grid.n_yaw, f->grid.nrows, f->grid.ncols, f->d_mask, f->d_d2);
  tm.mark(1);
  const size_t slots = artp::field_wtab_slots(f->grid);
  if (rc == ARTP_OK) {
    artp::FieldGrid Gb = f->grid;
    Gb.objective = f->params.objective;
    const artp::ClearWeight w{f->geom.res, cp.margin, cp.gain};
    hipLaunchKernelGGL(artp::field_clearance_table_kernel, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, Gb,
                       (const uint32_t*)f->d_mask, (const float*)f->d_h, (const double*)d_tab, (const uint16_t*)f->d_d2, w, slots,
                       f->d_tab);
    if (hipGetLastError() != hipSuccess) rc = ARTP_ERR_HIP;
  }
  tm.mark(2);
  if (hipStreamSynchronize(st) != hipSuccess && rc == ARTP_OK) rc = ARTP_ERR_HIP;  // the host table is free from here
  f->lstats.rows_ms = tm.ms(0, 1, rc == ARTP_OK);
  f->lstats.combine_ms = tm.ms(1, 2, rc == ARTP_OK);
  if (rc == ARTP_ERR_HIP && c->last_error.empty()) c->last_error = "clearance field: building the weight table failed";
  f->lstats.table_rows = slots;
  f->lstats.table_bytes = slots * sizeof(double);
  return rc;
}

// What a clearance-weighted entry point (who: artp_field_compute_clearance, or a batched one below) refuses about the
// context, the rectangle and its params, behind the context's lock.
int field_clearance_checks(artp_ctx* c, const char* who, const artp_field_clearance_params& p, int n_yaw, const int* rect,
                           size_t n_sources, artp::ReachRect* r) {
  if (!reach_have_lattice(c)) return ARTP_ERR_NO_MAP;
  ARTP_TRY(reach_resolve(c, n_yaw, rect, r));
  ARTP_TRY(field_check_params(c, p.base));
  if (n_sources > (size_t)1 << 24) {
    c->last_error = std::string(who) + ": n_sources <= 2^24";
    return ARTP_ERR_INVALID_ARG;
  }
  ARTP_TRY(clearance_check(c, p.clearance, n_yaw));
  if (!(p.margin > 0.0) || !std::isfinite(p.margin) || !(p.gain >= 0.0) || !std::isfinite(p.gain)) {
    c->last_error = std::string(who) + ": margin must be positive and finite, gain non-negative and finite";
    return ARTP_ERR_INVALID_ARG;
  }
  if (p.margin > (double)p.clearance.radius_cells * c->geom.res) {
    c->last_error = std::string(who) + ": margin exceeds radius_cells * resolution (clearance beyond the cap is unknown)";
    return ARTP_ERR_INVALID_ARG;
  }
  return ARTP_OK;
}

}  // namespace

extern "C" {

void artp_clearance_params_defaults(artp_clearance_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->radius_cells = 12;
  p->yaw_spread = 0;
  p->outside_is_obstacle = 0;
}

int artp_clearance_map_dev(artp_ctx* c, const artp_clearance_params* params, int n_yaw, int nrows, int ncols,
                           const uint32_t* mask, int mask_on_device, uint16_t* d2_dev) {
  if (!c || !params || !mask || !d2_dev) return ARTP_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  ARTP_TRY(clearance_map_args(c, params, n_yaw, nrows, ncols));
  HIP_TRY(c, hipSetDevice(c->device));
  const uint32_t* d_mask = mask;
  if (!mask_on_device) {  // staged through the context's scratch: the host words are read before the call returns
    const size_t bytes = (size_t)nrows * ncols * sizeof(uint32_t);
    ARTP_TRY(ensure_scratch(c, c->lane->host_args, bytes));
    HIP_TRY(c, hipMemcpyAsync(c->lane->host_args.get(), mask, bytes, hipMemcpyHostToDevice, c->lane->stream));
    HIP_TRY(c, hipStreamSynchronize(c->lane->stream));
    d_mask = c->lane->host_args.as<const uint32_t>();
  }
  return clearance_run(c, *params, n_yaw, nrows, ncols, d_mask, d2_dev);
}

int artp_clearance_map(artp_ctx* c, const artp_clearance_params* params, int n_yaw, int nrows, int ncols, const uint32_t* mask,
                       int mask_on_device, uint16_t* d2_out) {
  if (!c || !params || !mask || !d2_out) return ARTP_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  ARTP_TRY(clearance_map_args(c, params, n_yaw, nrows, ncols));
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t bytes = (size_t)nrows * ncols * n_yaw * sizeof(uint16_t);
  ARTP_TRY(ensure_scratch(c, c->lane->host_results, bytes));
  ARTP_TRY(artp_clearance_map_dev(c, params, n_yaw, nrows, ncols, mask, mask_on_device, c->lane->host_results.as<uint16_t>()));
  HIP_TRY(c, hipMemcpyAsync(d2_out, c->lane->host_results.get(), bytes, hipMemcpyDeviceToHost, c->lane->stream));
  HIP_TRY(c, hipStreamSynchronize(c->lane->stream));
  return ARTP_OK;
}

void artp_field_clearance_params_defaults(artp_field_clearance_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  artp_field_params_defaults(&p->base);
  artp_clearance_params_defaults(&p->clearance);
  p->margin = 0.2;
  p->gain = 2.0;
}

int artp_field_compute_clearance(artp_ctx* c, const artp_field_clearance_params* params, int n_yaw, const int* rect,
                                 const uint32_t* mask, int mask_on_device, const int* sources, size_t n_sources, int reverse,
                                 artp_field** out) {
  if (out) *out = nullptr;
  if (!c || !params || !mask || !sources || !out || n_sources < 1) return ARTP_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  artp::ReachRect r;
  ARTP_TRY(field_clearance_checks(c, "artp_field_compute_clearance", *params, n_yaw, rect, n_sources, &r));
  ARTP_TRY(field_check_sources(c, r, n_yaw, sources, n_sources));
  return field_create(c, params->base, nullptr, params, r, mask, mask_on_device, sources, n_sources, reverse, out);
}

// The batched forms (field_many.h): one clearance map and one weight table for the whole batch.
int artp_field_compute_many_clearance(artp_ctx* c, const artp_field_clearance_params* params, int n_yaw, const int* rect,
                                      const uint32_t* mask, int mask_on_device, const int* sources,
                                      const uint64_t* set_offsets, size_t n_sets, int reverse, artp_field** out_fields) {
  if (out_fields)
    for (size_t b = 0; b < n_sets && b < 65536; ++b) out_fields[b] = nullptr;
  if (!c || !params || !mask || !sources || !set_offsets || !out_fields) return ARTP_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  const char* who = "artp_field_compute_many_clearance";
  ARTP_TRY(field_many_check_count(c, who, n_sets));
  artp::ReachRect r;
  ARTP_TRY(field_clearance_checks(c, who, *params, n_yaw, rect, 1, &r));
  ARTP_TRY(field_many_tiled_only(c, who, params->base.plain_sweeps));
  FieldManyTable wt;
  wt.cp = params;
  return field_many_run(c, who, params->base, r, mask, mask_on_device, sources, set_offsets, n_sets, reverse, out_fields, &wt);
}

int artp_field_cost_matrix_clearance(artp_ctx* c, const artp_field_clearance_params* params, int n_yaw, const int* rect,
                                     const uint32_t* mask, int mask_on_device, const int* poses, size_t n, size_t batch,
                                     double* matrix_out, artp_field_many_stats_t* stats_out,
                                     artp_field_many_table_stats_t* table_out) {
  if (stats_out) std::memset(stats_out, 0, sizeof(*stats_out));
  if (table_out) std::memset(table_out, 0, sizeof(*table_out));
  if (!c || !params || !mask || !poses || !matrix_out) return ARTP_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  const char* who = "artp_field_cost_matrix_clearance";
  ARTP_TRY(field_matrix_check_count(c, who, n));
  artp::ReachRect r;
  ARTP_TRY(field_clearance_checks(c, who, *params, n_yaw, rect, 1, &r));
  ARTP_TRY(field_many_tiled_only(c, who, params->base.plain_sweeps));
  FieldManyTable wt;
  wt.cp = params;
  return field_matrix_run(c, who, params->base, r, mask, mask_on_device, poses, n, batch, matrix_out, stats_out, &wt, table_out);
}

int artp_field_clearance(artp_field* f, uint16_t* d2_out) {
  if (!f || !d2_out) return ARTP_ERR_INVALID_ARG;
  artp_ctx* c = f->ctx;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  if (!f->d_d2) {
    c->last_error = "artp_field_clearance: not a field of artp_field_compute_clearance";
    return ARTP_ERR_INVALID_ARG;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipMemcpyAsync(d2_out, f->d_d2, f->n_nodes * sizeof(uint16_t), hipMemcpyDeviceToHost, c->lane->stream));
  HIP_TRY(c, hipStreamSynchronize(c->lane->stream));
  return ARTP_OK;
}

int artp_field_update_clearance(artp_field* f, const uint32_t* new_mask, int mask_on_device, const int* sub_rect,
                                int refresh_heights) {
  if (!f || !new_mask) return ARTP_ERR_INVALID_ARG;
  artp_ctx* c = f->ctx;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  const artp::FieldGrid& G = f->grid;
  if (G.objective != 3) {
    c->last_error = "artp_field_update_clearance: not a field of artp_field_compute_clearance (artp_field_update and "
                    "artp_field_update_learned take the others)";
    return ARTP_ERR_INVALID_ARG;
  }
  artp::FieldSub sub;
  ARTP_TRY(field_sub_rect(f, "artp_field_update_clearance", sub_rect, &sub));
  const bool same_map = field_same_map(c, f);
  if (refresh_heights && !same_map) {
    c->last_error = "artp_field_update_clearance: refresh_heights needs sampler layers of the geometry the field was computed on";
    return ARTP_ERR_INVALID_ARG;
  }
  // The kind's step, when a word or a height changed: d2 again on the tiles within R cells of sub_rect (d_ucnt[7] += the
  // nodes whose value changed), then the slots of the tiles within R + 1 cells priced again; a slot whose bits change flags
  // its tile.  The passes run whenever the windows ran.
  return field_update_run(
      f, "artp_field_update_clearance", new_mask, mask_on_device, sub, refresh_heights != 0, same_map, &f->custats,
      [&](unsigned long long* cnt, artp_field_clearance_update_stats_t* us, bool* run) -> int {
        if (!cnt[0] && !cnt[3]) return ARTP_OK;
        hipStream_t st = c->lane->stream;
        const int R = f->cparams.clearance.radius_cells;
        const ClearTiles cw = clearance_window(G, sub, R), pw = clearance_window(G, sub, R + 1);
        StreamTimer<3> tm(st);
        tm.mark(0);
        int rc = clearance_run(c, f->cparams.clearance, G.n_yaw, G.nrows, G.ncols, f->d_mask, f->d_d2, &cw, f->d_ucnt + 7);
        tm.mark(1);
        if (rc == ARTP_OK) {
          artp::FieldGrid Gb = G;
          Gb.objective = f->params.objective;
          const artp::ClearWeight w{f->geom.res, f->cparams.margin, f->cparams.gain};
          hipLaunchKernelGGL(artp::field_clearance_reprice_kernel, dim3((unsigned)(pw.n * 10 * (size_t)G.n_yaw)), dim3(256), 0, st, Gb,
                             pw.w, (const uint32_t*)f->d_mask, (const float*)f->d_h, (const double*)f->d_btab,
                             (const uint16_t*)f->d_d2, w, f->d_tab, f->d_acc, f->d_wacc, f->d_ucnt);
          if (hipGetLastError() != hipSuccess) rc = ARTP_ERR_HIP;
        }
        tm.mark(2);
        if (rc == ARTP_OK) rc = field_weight_counts(f, cnt, 3);
        if (rc) {
          (void)hipStreamSynchronize(st);
          if (rc == ARTP_ERR_HIP && c->last_error.empty()) c->last_error = "artp_field_update_clearance: repricing the weight table failed";
          return rc;
        }
        us->clearance_ms = tm.ms(0, 1, true);
        us->reprice_ms = tm.ms(1, 2, true);
        us->clearance_tiles = cw.n;
        us->changed_d2 = cnt[7];
        us->repriced_slots = pw.n * 10 * (uint64_t)G.n_yaw * (artp::FIELD_T * artp::FIELD_T);
        us->changed_slots = cnt[5];
        us->weight_tiles = cnt[6];
        *run = true;
        return ARTP_OK;
      });
}

int artp_field_clearance_update_stats(artp_field* f, artp_field_clearance_update_stats_t* out) {
  if (!f || !out) return ARTP_ERR_INVALID_ARG;
  *out = f->custats;
  return ARTP_OK;
}

int artp_field_shift_clearance(artp_field* f, const uint32_t* new_mask, int mask_on_device, int refresh_heights) {
  if (!f || !new_mask) return ARTP_ERR_INVALID_ARG;
  artp_ctx* c = f->ctx;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  const artp::FieldGrid& G = f->grid;
  if (G.objective != 3) {
    c->last_error = "artp_field_shift_clearance: not a field of artp_field_compute_clearance (artp_field_shift takes a plain "
                    "field; a learned field is computed anew)";
    return ARTP_ERR_INVALID_ARG;
  }
  FieldMove mv;
  ARTP_TRY(field_shift_checks(f, "artp_field_shift_clearance", new_mask, mask_on_device, &mv));
  hipStream_t st = c->lane->stream;
  if (!mv.moves()) {
    // artp_field_update_clearance over the whole rectangle, on the geometry a shift adopts; its own stats stay
    const artp_field_clearance_update_stats_t kept = f->custats;
    f->geom = c->geom;
    const int rc = artp_field_update_clearance(f, mv.nm, 1, nullptr, refresh_heights);
    const artp_field_clearance_update_stats_t cu = f->custats;
    f->custats = kept;
    if (rc) return rc;
    artp_field_clearance_shift_stats_t us{};
    artp_field_update_stats_t ps;
    std::memcpy(&ps, &cu, sizeof(ps));  // the ten shared members, at their offsets
    field_store_stats(ps, cu.passes_ms, &us);
    us.kept_cells = f->n_cells;
    us.changed_slots = cu.changed_slots;
    us.weight_tiles = cu.weight_tiles;
    us.clearance_ms = cu.clearance_ms;
    us.table_ms = cu.reprice_ms;
    f->clshstats = us;
    return ARTP_OK;
  }
  const artp::FieldSub whole{0, 0, G.nrows, G.ncols};
  const size_t slots = artp::field_wtab_slots(G);
  StreamTimer<2> tm(st);
  // The kind's step: the move's counts, then d2 of the whole rectangle and the table priced into d_tab2 against the moved
  // old slots; cnt[5] counts the changed slots from zero again.  After a move the passes always run.
  return field_update_run(
      f, "artp_field_shift_clearance", mv.nm, 1, whole, refresh_heights != 0, true, &f->clshstats,
      [&]() -> int {
        ARTP_TRY(field_lazy(f, &f->d_tab2, slots));
        return field_shift_move(f, mv, tm);
      },
      [&](unsigned long long* cnt, artp_field_clearance_shift_stats_t* us, bool* run) -> int {
        ARTP_TRY(field_shift_counts(f, mv, tm, cnt, us));
        HIP_TRY(c, hipMemsetAsync(f->d_ucnt + 5, 0, sizeof(unsigned long long), st));
        const artp::FieldShift sh{(int)mv.si, (int)mv.sj, mv.si + mv.sj * (long long)G.nrows};
        StreamTimer<3> tc(st);
        tc.mark(0);
        int rc = clearance_run(c, f->cparams.clearance, G.n_yaw, G.nrows, G.ncols, f->d_mask, f->d_d2);
        tc.mark(1);
        if (rc == ARTP_OK) {
          artp::FieldGrid Gb = G;
          Gb.objective = f->params.objective;
          const artp::ClearWeight w{f->geom.res, f->cparams.margin, f->cparams.gain};
          hipLaunchKernelGGL(artp::field_clearance_shift_table_kernel, dim3((unsigned)(f->n_tiles * 10 * (size_t)G.n_yaw)), dim3(256), 0,
                             st, Gb, sh, (const uint32_t*)f->d_mask, (const float*)f->d_h, (const double*)f->d_btab,
                             (const uint16_t*)f->d_d2, w, (const double*)f->d_tab, f->d_tab2, f->d_acc, f->d_wacc, f->d_ucnt);
          if (hipGetLastError() != hipSuccess) rc = ARTP_ERR_HIP;
        }
        tc.mark(2);
        if (rc == ARTP_OK) rc = field_weight_counts(f, cnt, 2);
        if (rc) {
          (void)hipStreamSynchronize(st);
          if (rc == ARTP_ERR_HIP && c->last_error.empty()) c->last_error = "artp_field_shift_clearance: pricing the weight table failed";
          return rc;
        }
        std::swap(f->d_tab, f->d_tab2);  // the kernel has run: the searches read the new table, the next move writes the other
        us->clearance_ms = tc.ms(0, 1, true);
        us->table_ms = tc.ms(1, 2, true);
        us->changed_slots = cnt[5];
        us->weight_tiles = cnt[6];
        *run = true;
        return ARTP_OK;
      });
}

int artp_field_clearance_shift_stats(artp_field* f, artp_field_clearance_shift_stats_t* out) {
  if (!f || !out) return ARTP_ERR_INVALID_ARG;
  *out = f->clshstats;
  return ARTP_OK;
}

}  // extern "C"
