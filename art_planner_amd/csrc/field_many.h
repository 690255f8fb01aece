// field_many.h -- many cost-to-go fields in one batched search, and pose-to-pose cost matrices (include/artp_c.h
// artp_field_compute_many and artp_field_cost_matrix; their learned and clearance-weighted forms,
// artp_field_compute_many_learned / _clearance and artp_field_cost_matrix_learned / _clearance).
//
// A batch is B fields of one mask, one rectangle, one objective and one direction that differ in their sources alone.
// Every field is an ordinary artp_field with its own dist, hops, mask, heights, table and flags, so that afterwards each
// one is updated, shifted, blocked, planned on and destroyed alone.  The search is shared: field_tile_many_kernel
// (field.h) runs the tile body of field_tile_kernel on a grid of (tiles, fields), blockIdx.y picks the field's
// FieldSlot, and the mask, the heights and the (m, k) table are read from the first field's copies.  The rules and the
// tile protocol are those of field.h; nothing about them is written here.
//   field_many_pass    the host loop of one rule over the batch: one launch per round, then ONE copy of all the fields'
//                      counters (four words a field, contiguous in the call's own block).  A field is finished after the
//                      first round that leaves its flag counter unchanged: both of its flag arrays are zero then, every
//                      workgroup of it leaves on its first load, and only its own tiles could flag it again.  The loop
//                      ends when every field is finished; the cap of n_nodes + 2 rounds is field_rounds'.
//   field_many_compute allocation (after a look at hipMemGetInfo), upload, per-field init / sources / seed through the
//                      kernels of field.h, the source check of all sets in one copy, the two passes, the counts
// A batch of learned or clearance-weighted fields (FieldManyTable) searches ONE weight table with
// field_tile_many_kernel<PHASE, true>.  The table is priced once, by the builds of the single fields (field_learned_build,
// field_clearance_build) and by nothing else: in field 0 of artp_field_compute_many_*, whose other fields then get their
// own device-to-device copies (and d2 and the base table of a clearance field) in front of the search; in a field of the
// call's own for a cost matrix, whose groups' fields borrow its table and never free it.
// The call writes nothing into the context beyond what the single learned call writes: it runs on the current lane's
// stream and owns its block (slots, counters, sources) for its own duration.
#pragma once

#include <memory>
#include <string>
#include <vector>

namespace {

struct FieldBatch {
  std::vector<artp_field*> fields;
  DeviceScratch mem;                  // slots | counters | sources: freed with the call
  artp::FieldSlot* d_slots = nullptr;
  unsigned* d_cnt = nullptr;          // four words per field: flags set, tiles run, (deaths: not used), spare
  int* d_src = nullptr;               // the source triples of all sets
  uint64_t dist_rounds = 0, hop_rounds = 0;  // launches of the two passes
  uint64_t tile_runs = 0, hop_tile_runs = 0;
  FieldBatch() = default;
  FieldBatch(const FieldBatch&) = delete;
  FieldBatch& operator=(const FieldBatch&) = delete;
  // the caller has set the device
  void destroy_fields() {
    for (artp_field* f : fields) field_free(f);
    fields.clear();
  }
};

// The weight table of a batch of learned (lp) or clearance-weighted (cp) fields: exactly one of the two is set.
struct FieldManyTable {
  const artp_field_learned_params* lp = nullptr;
  const artp_field_clearance_params* cp = nullptr;
  // cost matrices: the call's own field, which holds the one table (with its mask, heights and d2) for all groups; a
  // group's fields borrow its d_tab, which is in none of their `mem`.  nullptr: field 0 of the batch builds the table and
  // every other field gets its own copy.
  artp_field* owner = nullptr;
  artp_field_many_table_stats_t ts{};
};

struct FieldFree {
  void operator()(artp_field* f) const { field_free(f); }  // the caller has set the device
};

// device bytes a field of a batch holds when the call returns (dist 8 + hops 4 a node, mask 4 + heights 4 a cell, table,
// flags, scratch), with a page of slack for each of its eight allocations
size_t field_many_bytes(size_t n_nodes, size_t n_cells, size_t n_tiles) {
  return n_nodes * 12 + n_cells * 8 + artp::FIELD_TAB * sizeof(double) + (2 * n_tiles + 4) * sizeof(unsigned) + 8 * 4096;
}

// the bytes of a weight table over n_tiles tiles, and what its build holds next to it: a chunk of query scratch
// (learned), or d2 and the base objective's table (clearance), which a clearance-weighted field keeps
size_t field_many_table_bytes(size_t n_tiles, int n_yaw) {
  return n_tiles * (size_t)n_yaw * 10 * (artp::FIELD_T * artp::FIELD_T) * sizeof(double);
}
size_t field_many_build_bytes(const FieldManyTable& wt, size_t n_tiles, size_t n_nodes, int n_yaw) {
  if (wt.cp) return n_nodes * sizeof(uint16_t) + artp::FIELD_TAB * sizeof(double) + 2 * 4096;
  return std::min(field_many_table_bytes(n_tiles, n_yaw) / sizeof(double), artp::FIELD_LEARNED_CHUNK) * 9 * sizeof(float) + 4096;
}

// The one build of a batch's table, in f (its mask, heights and d_tab are in place): the single field's own build.
int field_many_table_build(artp_ctx* c, artp_field* f, FieldManyTable* wt) {
  if (wt->lp) {
    ARTP_TRY(field_learned_build(c, f));
  } else {
    double tab[artp::FIELD_TAB];
    field_make_table(f->params, f->geom, f->grid.n_yaw, tab);
    ARTP_TRY(field_clearance_build(c, f, tab));  // synchronises: the host table is free when it returns
  }
  wt->ts.table_builds += 1;
  wt->ts.table_rows = f->lstats.table_rows;
  wt->ts.table_bytes = f->lstats.table_bytes;
  wt->ts.build_ms += f->lstats.rows_ms + f->lstats.query_ms + f->lstats.combine_ms;
  return ARTP_OK;
}

// One rule (relax, PHASE 0 or 1) over the whole batch to every field's fixed point, from the tiles of each field's sources.
template <int PHASE>
int field_many_pass(artp_ctx* c, FieldBatch& bt, const uint64_t* off, const char* too_many, std::vector<FieldRounds>* out,
                    uint64_t* launches) {
  hipStream_t st = c->lane->stream;
  const size_t B = bt.fields.size();
  artp_field* f0 = bt.fields[0];
  const artp::FieldGrid& G = f0->grid;
  HIP_TRY(c, hipMemsetAsync(bt.d_cnt, 0, 4 * B * sizeof(unsigned), st));
  for (size_t b = 0; b < B; ++b) {
    artp_field* f = bt.fields[b];
    const int n_src = (int)(off[b + 1] - off[b]);
    HIP_TRY(c, hipMemsetAsync(f->d_flags, 0, (2 * f->n_tiles + 4) * sizeof(unsigned), st));
    hipLaunchKernelGGL(artp::field_seed_tiles_kernel, dim3((unsigned)((n_src + 63) / 64)), dim3(64), 0, st, G,
                       (const int*)(bt.d_src + 3 * off[b]), n_src, f->d_flags);
  }
  HIP_TRY(c, hipGetLastError());
  const size_t lds = artp::field_tile_lds(G.n_yaw, PHASE == 1);
  auto kernel = &artp::field_tile_many_kernel<PHASE, false>;
  if (artp::field_has_wtab(G)) kernel = &artp::field_tile_many_kernel<PHASE, true>;  // f0->d_tab is the batch's weight table
  // its own opt-in: the attribute belongs to a function, and neither of the two is field_tile_kernel or the other one
  // (32 headings: 88 / 126 KB)
  if (lds > 64 * 1024)
    HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds));
  std::vector<unsigned> now(4 * B, 0u), seen(B, 0u);
  std::vector<char> done(B, 0);
  size_t left = B;
  out->assign(B, FieldRounds{});
  const uint64_t cap = (uint64_t)f0->n_nodes + 2;
  for (uint64_t round = 0;;) {
    if (round > cap) {
      c->last_error = too_many;
      return ARTP_ERR_CAPACITY;
    }
    hipLaunchKernelGGL(kernel, dim3((unsigned)f0->n_tiles, (unsigned)B), dim3(256), lds, st, G, (const uint32_t*)f0->d_mask,
                       (const float*)f0->d_h, (const double*)f0->d_tab, (const artp::FieldSlot*)bt.d_slots, (int)(round & 1),
                       f0->params.inner_sweeps);
    ++round;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(now.data(), bt.d_cnt, 4 * B * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    for (size_t b = 0; b < B; ++b) {
      if (done[b]) continue;
      if (now[4 * b] == seen[b]) {  // nothing flagged for the next round: this field is at its fixed point
        done[b] = 1;
        --left;
        (*out)[b] = FieldRounds{round, now[4 * b + 1], 0};
      } else {
        seen[b] = now[4 * b];
      }
    }
    if (!left) {
      *launches = round;
      return ARTP_OK;
    }
  }
}

// The batch behind the checks of its entry point: bt.fields on success, nothing on failure (the caller destroys what
// bt.fields holds).  who: the entry point, for the texts; what / base: a bad source is reported as "<what> <base + set>".
// wt: the weight table of a learned or clearance-weighted batch (params: the field params such a field carries), nullptr
// for objectives 0 and 1.
int field_many_compute(artp_ctx* c, FieldBatch& bt, const artp_field_params& params, const artp::ReachRect& r,
                       const uint32_t* mask, int mask_on_device, const int* sources, const uint64_t* off, size_t B, int reverse,
                       const char* who, const char* what, size_t base, FieldManyTable* wt = nullptr) {
  hipStream_t st = c->lane->stream;
  const size_t n_cells = (size_t)r.nrows * r.ncols, n_nodes = n_cells * (size_t)r.n_yaw;
  const size_t n_tiles = (size_t)((r.nrows + artp::FIELD_T - 1) / artp::FIELD_T) * (size_t)((r.ncols + artp::FIELD_T - 1) / artp::FIELD_T);
  const size_t total_src = (size_t)off[B];
  const bool own_tables = wt && !wt->owner;  // field 0 builds, the others copy
  const size_t tab_doubles = own_tables ? field_many_table_bytes(n_tiles, r.n_yaw) / sizeof(double) : (size_t)artp::FIELD_TAB;
  const size_t d2_bytes = n_nodes * sizeof(uint16_t) + artp::FIELD_TAB * sizeof(double) + 2 * 4096;  // with the base table
  {  // the weight-table check of field_compute_impl, for B fields and the call's block
    size_t need = B * field_many_bytes(n_nodes, n_cells, n_tiles) + 3 * total_src * 2 * sizeof(int) +
                  B * (sizeof(artp::FieldSlot) + 4 * sizeof(unsigned)) + 3 * 4096;
    if (own_tables)  // the table and its B - 1 copies, what the build holds, and a clearance field's d2 and base table
      need += B * tab_doubles * sizeof(double) + field_many_build_bytes(*wt, n_tiles, n_nodes, r.n_yaw) + (wt->cp ? (B - 1) * d2_bytes : 0);
    size_t free_b = 0, total_b = 0;
    HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
    if (need > free_b) {
      c->last_error = std::string(who) + ": " + std::to_string(B) + " fields need " + std::to_string(need >> 20) +
                      " MB, the device has " + std::to_string(free_b >> 20) + " MB free";
      return ARTP_ERR_CAPACITY;
    }
  }
  HIP_TRY(c, bt.mem.alloc(&bt.d_slots, B));
  HIP_TRY(c, bt.mem.alloc(&bt.d_cnt, 4 * B));
  HIP_TRY(c, bt.mem.alloc(&bt.d_src, 3 * total_src));
  std::vector<artp::FieldSlot> slots(B);
  bt.fields.reserve(B);
  for (size_t b = 0; b < B; ++b) {
    artp_field* f = field_new(c, params, wt ? wt->lp : nullptr, wt ? wt->cp : nullptr, r, reverse);
    bt.fields.push_back(f);
    HIP_TRY(c, f->mem.alloc(&f->d_dist, f->n_nodes));
    HIP_TRY(c, f->mem.alloc(&f->d_hops, f->n_nodes));
    HIP_TRY(c, f->mem.alloc(&f->d_mask, f->n_cells));
    HIP_TRY(c, f->mem.alloc(&f->d_h, f->n_cells));
    if (wt && wt->owner)
      f->d_tab = wt->owner->d_tab;  // borrowed: not in f->mem, so the field does not free it
    else
      HIP_TRY(c, f->mem.alloc(&f->d_tab, tab_doubles));
    HIP_TRY(c, f->mem.alloc(&f->d_flags, 2 * f->n_tiles + 4));
    if (own_tables && wt->cp && b) {  // field 0 gets the two from its build
      HIP_TRY(c, f->mem.alloc(&f->d_btab, (size_t)artp::FIELD_TAB));
      HIP_TRY(c, f->mem.alloc(&f->d_d2, f->n_nodes));
    }
    const size_t n_src = (size_t)(off[b + 1] - off[b]);
    ARTP_TRY(field_ensure_scratch(f, 3 * n_src, 8));
    f->h_src.assign(sources + 3 * off[b], sources + 3 * off[b + 1]);
    slots[b] = artp::FieldSlot{f->d_dist, f->d_hops, f->d_flags, bt.d_cnt + 4 * b};
  }
  artp_field* f0 = bt.fields[0];
  const artp::FieldGrid& G = f0->grid;
  double tab[artp::FIELD_TAB];
  field_make_table(params, f0->geom, G.n_yaw, tab);
  HIP_TRY(c, hipMemcpyAsync(bt.d_slots, slots.data(), B * sizeof(artp::FieldSlot), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(bt.d_src, sources, 3 * total_src * sizeof(int), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemsetAsync(bt.d_cnt, 0, 4 * B * sizeof(unsigned), st));
  HIP_TRY(c, hipMemcpyAsync(f0->d_mask, mask, n_cells * sizeof(uint32_t),
                            mask_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  if (!wt) HIP_TRY(c, hipMemcpyAsync(f0->d_tab, tab, sizeof(tab), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(artp::field_heights_kernel, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, st, f0->sampler,
                     f0->geom, f0->rect, f0->d_h);
  for (size_t b = 0; b < B; ++b) {
    artp_field* f = bt.fields[b];
    const size_t n_src = (size_t)(off[b + 1] - off[b]);
    if (b) {  // the field's own copies of what the search shares: its later life (update, shift, plan) is its own
      HIP_TRY(c, hipMemcpyAsync(f->d_mask, f0->d_mask, n_cells * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
      HIP_TRY(c, hipMemcpyAsync(f->d_h, f0->d_h, n_cells * sizeof(float), hipMemcpyDeviceToDevice, st));
      if (!wt) HIP_TRY(c, hipMemcpyAsync(f->d_tab, f0->d_tab, sizeof(tab), hipMemcpyDeviceToDevice, st));
    }
    hipLaunchKernelGGL(artp::field_init_kernel, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, st, n_nodes, f->d_dist,
                       f->d_hops);
    hipLaunchKernelGGL(artp::field_sources_kernel, dim3((unsigned)((n_src + 63) / 64)), dim3(64), 0, st, G,
                       (const uint32_t*)f0->d_mask, (const int*)(bt.d_src + 3 * off[b]), (int)n_src, f->d_dist, f->d_hops,
                       bt.d_cnt + 4 * b);
  }
  HIP_TRY(c, hipGetLastError());
  std::vector<unsigned> bad(4 * B, 0u);
  HIP_TRY(c, hipMemcpyAsync(bad.data(), bt.d_cnt, 4 * B * sizeof(unsigned), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));  // the host copies of mask, table, slots and sources are free from here
  for (size_t b = 0; b < B; ++b)
    if (bad[4 * b]) {
      c->last_error = std::string(who) + ": a source of " + what + " " + std::to_string(base + b) + " is not a node of the mask";
      return ARTP_ERR_INVALID_ARG;
    }
  if (own_tables) {  // priced once, behind the source check; then every other field's own copy, in front of the search
    ARTP_TRY(field_many_table_build(c, f0, wt));
    for (size_t b = 1; b < B; ++b) {
      artp_field* f = bt.fields[b];
      HIP_TRY(c, hipMemcpyAsync(f->d_tab, f0->d_tab, tab_doubles * sizeof(double), hipMemcpyDeviceToDevice, st));
      if (wt->cp) {
        HIP_TRY(c, hipMemcpyAsync(f->d_d2, f0->d_d2, n_nodes * sizeof(uint16_t), hipMemcpyDeviceToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(f->d_btab, f0->d_btab, artp::FIELD_TAB * sizeof(double), hipMemcpyDeviceToDevice, st));
      }
      wt->ts.table_copies += 1;
    }
  }
  std::vector<FieldRounds> dist_pass, hop_pass;
  const std::string too_many = std::string(who) + ": more rounds than nodes";
  const auto t0 = std::chrono::steady_clock::now();
  ARTP_TRY(field_many_pass<0>(c, bt, off, too_many.c_str(), &dist_pass, &bt.dist_rounds));
  const auto t1 = std::chrono::steady_clock::now();
  ARTP_TRY(field_many_pass<1>(c, bt, off, too_many.c_str(), &hop_pass, &bt.hop_rounds));
  const auto t2 = std::chrono::steady_clock::now();
  for (size_t b = 0; b < B; ++b) {
    artp_field* f = bt.fields[b];
    if (wt) {  // the shared build and the batch's two passes
      f->lstats = (wt->owner ? wt->owner : f0)->lstats;
      f->lstats.dist_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
      f->lstats.hop_ms = std::chrono::duration<double, std::milli>(t2 - t1).count();
    }
    f->stats.outer_rounds = dist_pass[b].rounds;
    f->stats.tile_launches = dist_pass[b].tile_runs;
    f->stats.hop_rounds = hop_pass[b].rounds;
    f->stats.hop_tile_launches = hop_pass[b].tile_runs;
    bt.tile_runs += dist_pass[b].tile_runs;
    bt.hop_tile_runs += hop_pass[b].tile_runs;
    ARTP_TRY(field_count_reached(f, &f->stats.reached_nodes));
  }
  return ARTP_OK;
}

// a batch runs in the tiled form only
int field_many_tiled_only(artp_ctx* c, const char* who, int plain_sweeps) {
  if (plain_sweeps != 0) {
    c->last_error = std::string(who) + ": plain_sweeps must be 0 (a batch runs in the tiled form only)";
    return ARTP_ERR_INVALID_ARG;
  }
  return ARTP_OK;
}

// what both entry points refuse about the context, the rectangle and the params; the context's lock is held
int field_many_checks(artp_ctx* c, const char* who, const artp_field_params& params, int n_yaw, const int* rect,
                      artp::ReachRect* r) {
  if (!reach_have_lattice(c)) return ARTP_ERR_NO_MAP;
  ARTP_TRY(reach_resolve(c, n_yaw, rect, r));
  ARTP_TRY(field_check_params(c, params));
  return field_many_tiled_only(c, who, params.plain_sweeps);
}

int field_many_check_count(artp_ctx* c, const char* who, size_t n_sets) {
  if (n_sets < 1 || n_sets > 65535) {
    c->last_error = std::string(who) + ": n_sets must lie in [1, 65535]";
    return ARTP_ERR_INVALID_ARG;
  }
  return ARTP_OK;
}

// artp_field_compute_many and its weighted forms behind the checks of the context, the rectangle and the params: the
// checks of the sets and the sources, the batch, the fields handed over
int field_many_run(artp_ctx* c, const char* who, const artp_field_params& params, const artp::ReachRect& r, const uint32_t* mask,
                   int mask_on_device, const int* sources, const uint64_t* set_offsets, size_t n_sets, int reverse,
                   artp_field** out_fields, FieldManyTable* wt) {
  if (set_offsets[0] != 0) {
    c->last_error = std::string(who) + ": set_offsets must start at 0";
    return ARTP_ERR_INVALID_ARG;
  }
  for (size_t b = 0; b < n_sets; ++b) {
    if (set_offsets[b + 1] <= set_offsets[b]) {
      c->last_error = std::string(who) + ": set " + std::to_string(b) +
                      (set_offsets[b + 1] == set_offsets[b] ? " is empty" : " ends before it starts (set_offsets must increase)");
      return ARTP_ERR_INVALID_ARG;
    }
    if (set_offsets[b + 1] > (uint64_t)1 << 24) {
      c->last_error = std::string(who) + ": more than 2^24 sources";
      return ARTP_ERR_INVALID_ARG;
    }
  }
  ARTP_TRY(field_check_sources(c, r, r.n_yaw, sources, (size_t)set_offsets[n_sets]));
  HIP_TRY(c, hipSetDevice(c->device));
  FieldBatch bt;
  const int rc = field_many_compute(c, bt, params, r, mask, mask_on_device, sources, set_offsets, n_sets, reverse, who, "set", 0, wt);
  if (rc) {
    bt.destroy_fields();
    return rc;
  }
  for (size_t b = 0; b < n_sets; ++b) out_fields[b] = bt.fields[b];
  return ARTP_OK;
}

// artp_field_cost_matrix and its weighted forms behind the same checks (n included).  wt: the call prices ONE table, in a
// field of its own that lives until the call returns, behind a check of every pose; every group borrows it.
int field_matrix_run(artp_ctx* c, const char* who, const artp_field_params& params, const artp::ReachRect& r,
                     const uint32_t* mask, int mask_on_device, const int* poses, size_t n, size_t batch, double* matrix_out,
                     artp_field_many_stats_t* stats_out, FieldManyTable* wt, artp_field_many_table_stats_t* table_out) {
  const int n_yaw = r.n_yaw;
  ARTP_TRY(field_check_sources(c, r, n_yaw, poses, n));
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->lane->stream;
  const size_t n_cells = (size_t)r.nrows * r.ncols, n_nodes = n_cells * (size_t)n_yaw;
  const size_t n_tiles = (size_t)((r.nrows + artp::FIELD_T - 1) / artp::FIELD_T) * (size_t)((r.ncols + artp::FIELD_T - 1) / artp::FIELD_T);
  DeviceScratch mem;  // the call's own: the mask on the device (a host mask goes up once), the nodes, a group's values
  std::unique_ptr<artp_field, FieldFree> owner;  // freed once, on every way out, behind the groups' fields
  uint32_t* d_mask = nullptr;
  uint32_t* d_nodes = nullptr;
  double* d_vals = nullptr;
  if (wt) {
    const size_t need = field_many_table_bytes(n_tiles, n_yaw) + field_many_build_bytes(*wt, n_tiles, n_nodes, n_yaw) +
                        n_cells * 8 + n * 4 * sizeof(int) + field_many_bytes(n_nodes, n_cells, n_tiles);
    size_t free_b = 0, total_b = 0;
    HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
    if (need > free_b) {
      c->last_error = std::string(who) + ": the weight table and one field need " + std::to_string(need >> 20) +
                      " MB, the device has " + std::to_string(free_b >> 20) + " MB free";
      return ARTP_ERR_CAPACITY;
    }
    artp_field* f = field_new(c, params, wt->lp, wt->cp, r, 0);
    owner.reset(f);
    wt->owner = f;
    int* d_poses = nullptr;
    unsigned* d_bad = nullptr;
    HIP_TRY(c, f->mem.alloc(&f->d_mask, n_cells));
    HIP_TRY(c, f->mem.alloc(&f->d_h, n_cells));
    HIP_TRY(c, f->mem.alloc(&f->d_tab, field_many_table_bytes(n_tiles, n_yaw) / sizeof(double)));
    HIP_TRY(c, mem.alloc(&d_poses, 3 * n));
    HIP_TRY(c, mem.alloc(&d_bad, n));
    HIP_TRY(c, hipMemcpyAsync(f->d_mask, mask, n_cells * sizeof(uint32_t),
                              mask_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_poses, poses, 3 * n * sizeof(int), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(artp::field_heights_kernel, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, st, f->sampler, f->geom,
                       f->rect, f->d_h);
    hipLaunchKernelGGL(artp::field_pose_check_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, f->grid,
                       (const uint32_t*)f->d_mask, (const int*)d_poses, (int)n, d_bad);
    HIP_TRY(c, hipGetLastError());
    std::vector<unsigned> bad(n, 0u);
    HIP_TRY(c, hipMemcpyAsync(bad.data(), d_bad, n * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    mem.release(d_poses);
    mem.release(d_bad);
    for (size_t i = 0; i < n; ++i)
      if (bad[i]) {
        c->last_error = std::string(who) + ": a source of pose " + std::to_string(i) + " is not a node of the mask";
        return ARTP_ERR_INVALID_ARG;
      }
    ARTP_TRY(field_many_table_build(c, f, wt));
    mask = f->d_mask;
    mask_on_device = 1;
  }
  if (batch == 0) {  // the largest group that fits in half of the free memory (the table is allocated: it is not in it)
    size_t free_b = 0, total_b = 0;
    HIP_TRY(c, hipMemGetInfo(&free_b, &total_b));
    batch = std::max<size_t>((free_b / 2) / field_many_bytes(n_nodes, n_cells, n_tiles), 1);
  }
  batch = std::min<size_t>(std::min<size_t>(batch, n), 65535);
  if (!mask_on_device) {
    HIP_TRY(c, mem.alloc(&d_mask, n_cells));
    HIP_TRY(c, hipMemcpyAsync(d_mask, mask, n_cells * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  }
  HIP_TRY(c, mem.alloc(&d_nodes, n));
  HIP_TRY(c, mem.alloc(&d_vals, batch * n));
  std::vector<uint32_t> nodes(n);
  for (size_t i = 0; i < n; ++i)
    nodes[i] = ((uint32_t)poses[3 * i] + (uint32_t)poses[3 * i + 1] * (uint32_t)r.nrows) * (uint32_t)n_yaw + (uint32_t)poses[3 * i + 2];
  HIP_TRY(c, hipMemcpyAsync(d_nodes, nodes.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  std::vector<uint64_t> off(batch + 1);
  for (size_t b = 0; b <= batch; ++b) off[b] = b;
  artp_field_many_stats_t ms{};
  for (size_t g0 = 0; g0 < n; g0 += batch) {
    const size_t B = std::min(batch, n - g0);
    FieldBatch bt;
    int rc = field_many_compute(c, bt, params, r, mask_on_device ? mask : d_mask, 1, poses + 3 * g0, off.data(), B, 0, who,
                                "pose", g0, wt);
    if (rc == ARTP_OK) {
      hipLaunchKernelGGL(artp::field_gather_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)B), dim3(256), 0, st,
                         (const artp::FieldSlot*)bt.d_slots, (const uint32_t*)d_nodes, (uint32_t)n, d_vals);
      if (hipGetLastError() != hipSuccess ||
          hipMemcpyAsync(matrix_out + g0 * n, d_vals, B * n * sizeof(double), hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipStreamSynchronize(st) != hipSuccess) {
        c->last_error = std::string(who) + ": gathering a group's values failed";
        rc = ARTP_ERR_HIP;
      }
    }
    bt.destroy_fields();  // before the next group starts
    if (rc) return rc;
    ms.groups += 1;
    ms.fields += B;
    ms.dist_rounds += bt.dist_rounds;
    ms.hop_rounds += bt.hop_rounds;
    ms.tile_runs += bt.tile_runs;
    ms.hop_tile_runs += bt.hop_tile_runs;
  }
  if (stats_out) *stats_out = ms;
  if (wt && table_out) *table_out = wt->ts;
  return ARTP_OK;
}

int field_matrix_check_count(artp_ctx* c, const char* who, size_t n) {
  if (n < 1 || n > (size_t)1 << 16) {
    c->last_error = std::string(who) + ": n must lie in [1, 65536]";
    return ARTP_ERR_INVALID_ARG;
  }
  return ARTP_OK;
}

}  // namespace

extern "C" {

int artp_field_compute_many(artp_ctx* c, const artp_field_params* params, int n_yaw, const int* rect, const uint32_t* mask,
                            int mask_on_device, const int* sources, const uint64_t* set_offsets, size_t n_sets, int reverse,
                            artp_field** out_fields) {
  if (out_fields)
    for (size_t b = 0; b < n_sets && b < 65536; ++b) out_fields[b] = nullptr;
  if (!c || !params || !mask || !sources || !set_offsets || !out_fields) return ARTP_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  const char* who = "artp_field_compute_many";
  ARTP_TRY(field_many_check_count(c, who, n_sets));
  artp::ReachRect r;
  ARTP_TRY(field_many_checks(c, who, *params, n_yaw, rect, &r));
  return field_many_run(c, who, *params, r, mask, mask_on_device, sources, set_offsets, n_sets, reverse, out_fields, nullptr);
}

int artp_field_cost_matrix(artp_ctx* c, const artp_field_params* params, int n_yaw, const int* rect, const uint32_t* mask,
                           int mask_on_device, const int* poses, size_t n, size_t batch, double* matrix_out,
                           artp_field_many_stats_t* stats_out) {
  if (stats_out) std::memset(stats_out, 0, sizeof(*stats_out));
  if (!c || !params || !mask || !poses || !matrix_out) return ARTP_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  const char* who = "artp_field_cost_matrix";
  ARTP_TRY(field_matrix_check_count(c, who, n));
  artp::ReachRect r;
  ARTP_TRY(field_many_checks(c, who, *params, n_yaw, rect, &r));
  return field_matrix_run(c, who, *params, r, mask, mask_on_device, poses, n, batch, matrix_out, stats_out, nullptr, nullptr);
}

int artp_field_compute_many_learned(artp_ctx* c, const artp_field_learned_params* params, int n_yaw, const int* rect,
                                    const uint32_t* mask, int mask_on_device, const int* sources, const uint64_t* set_offsets,
                                    size_t n_sets, int reverse, artp_field** out_fields) {
  if (out_fields)
    for (size_t b = 0; b < n_sets && b < 65536; ++b) out_fields[b] = nullptr;
  if (!c || !params || !mask || !sources || !set_offsets || !out_fields) return ARTP_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  const char* who = "artp_field_compute_many_learned";
  ARTP_TRY(field_many_check_count(c, who, n_sets));
  artp::ReachRect r;
  artp_field_params fp;
  ARTP_TRY(field_learned_checks(c, who, *params, n_yaw, rect, 1, &r, &fp));
  ARTP_TRY(field_many_tiled_only(c, who, params->plain_sweeps));
  FieldManyTable wt;
  wt.lp = params;
  return field_many_run(c, who, fp, r, mask, mask_on_device, sources, set_offsets, n_sets, reverse, out_fields, &wt);
}

int artp_field_cost_matrix_learned(artp_ctx* c, const artp_field_learned_params* params, int n_yaw, const int* rect,
                                   const uint32_t* mask, int mask_on_device, const int* poses, size_t n, size_t batch,
                                   double* matrix_out, artp_field_many_stats_t* stats_out,
                                   artp_field_many_table_stats_t* table_out) {
  if (stats_out) std::memset(stats_out, 0, sizeof(*stats_out));
  if (table_out) std::memset(table_out, 0, sizeof(*table_out));
  if (!c || !params || !mask || !poses || !matrix_out) return ARTP_ERR_INVALID_ARG;
  std::lock_guard<std::recursive_mutex> lock(c->mu);
  const char* who = "artp_field_cost_matrix_learned";
  ARTP_TRY(field_matrix_check_count(c, who, n));
  artp::ReachRect r;
  artp_field_params fp;
  ARTP_TRY(field_learned_checks(c, who, *params, n_yaw, rect, 1, &r, &fp));
  ARTP_TRY(field_many_tiled_only(c, who, params->plain_sweeps));
  FieldManyTable wt;
  wt.lp = params;
  return field_matrix_run(c, who, fp, r, mask, mask_on_device, poses, n, batch, matrix_out, stats_out, &wt, table_out);
}

}  // extern "C"
