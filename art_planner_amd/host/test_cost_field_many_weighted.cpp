// Exercises Planner::computeLearnedCostFields / computeClearanceCostFields (artp_field_compute_many_learned / _clearance)
// and Planner::computeLearnedCostMatrix / computeClearanceCostMatrix (artp_field_cost_matrix_learned / _clearance) through
// the host mirror on the map of test_cost_field_many.cpp: 90 x 70 cells at 0.1 m, flat ground with a raised block and a
// trench, the mask from Planner::computeReachability with a keep-out zone cut into it.  The motion-cost network comes from
// the blob file named on the command line (the runner writes seeded random parameters).  Under each cost, three source
// sets (one of two sources) go through one batched call; every field is compared bit for bit with the single call on its
// set -- dist, reached_nodes, the path to the set's farthest node, and the clearance map of a clearance field -- and stays
// usable after its neighbours are destroyed.  The matrix of four poses is compared with single fields' dist at the poses,
// in one group and in groups of three; its table is built once and never copied.  A bad source in set 1 throws and names it.
//   test_cost_field_many_weighted <weights.blob>
// Exit code 0 = every check holds; 3 = no GPU (the constructor throws: no CPU fallback); 2 = no blob file.
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <functional>
#include <iterator>
#include <memory>
#include <string>
#include <vector>

#include "art_planner/planner.h"

using namespace art_planner;

static int fails = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++fails;                                                      \
    }                                                               \
  } while (0)

using Pose = std::array<int, 3>;
using Sets = std::vector<std::vector<Pose>>;

static const int rows = 90, cols = 70, n_yaw = 8;
static const size_t cells = static_cast<size_t>(rows) * cols, nodes = cells * n_yaw;

static size_t node_of(const Pose& p) { return (p[0] + static_cast<size_t>(p[1]) * rows) * n_yaw + p[2]; }

// the fields of one batched call against single(set, &kept) on every set; returns the mismatches
static size_t compare_fields(const std::vector<artp_field*>& many, const Sets& sets,
                             const std::function<std::vector<double>(const std::vector<Pose>&, artp_field**)>& single,
                             bool clearance) {
  size_t mismatches = 0;
  std::vector<double> got(nodes);
  std::vector<int> pa(3 * nodes), pb(3 * nodes);
  std::vector<uint16_t> da(nodes), db(nodes);
  for (size_t b = 0; b < sets.size(); ++b) {
    CHECK(many[b] != nullptr);
    if (!many[b]) return mismatches + 1;
    artp_field* one = nullptr;
    const std::vector<double> dist = single(sets[b], &one);
    CHECK(one != nullptr && dist.size() == nodes);
    if (!one || dist.size() != nodes) return mismatches + 1;
    CHECK(artp_field_dist(many[b], got.data()) == ARTP_OK);
    mismatches += std::memcmp(got.data(), dist.data(), nodes * sizeof(double)) != 0;
    artp_field_stats_t sm, ss;
    CHECK(artp_field_stats(many[b], &sm) == ARTP_OK && artp_field_stats(one, &ss) == ARTP_OK);
    mismatches += sm.reached_nodes != ss.reached_nodes || sm.nodes != ss.nodes || sm.tiles != ss.tiles;
    CHECK(sm.outer_rounds > 0 && sm.hop_rounds > 0 && sm.plain_sweeps == 0 && sm.reached_nodes > cells);
    artp_field_learned_stats_t lm, ls;
    CHECK(artp_field_learned_stats(many[b], &lm) == ARTP_OK && artp_field_learned_stats(one, &ls) == ARTP_OK);
    mismatches += lm.table_rows != ls.table_rows || lm.table_bytes != ls.table_bytes;
    for (const auto& s : sets[b]) CHECK(dist[node_of(s)] == 0.0);
    size_t far = 0;   // the path to the farthest node of this field: the same states from both
    double farthest = -1.0;
    for (size_t i = 0; i < nodes; ++i)
      if (std::isfinite(dist[i]) && dist[i] > farthest) {
        farthest = dist[i];
        far = i;
      }
    const int target[3] = {static_cast<int>((far / n_yaw) % rows), static_cast<int>((far / n_yaw) / rows),
                           static_cast<int>(far % n_yaw)};
    size_t na = 0, nb = 0;
    double ca = 0.0, cb = 0.0;
    CHECK(artp_field_path(many[b], target, pa.data(), nullptr, nodes, &na, &ca) == ARTP_OK);
    CHECK(artp_field_path(one, target, pb.data(), nullptr, nodes, &nb, &cb) == ARTP_OK);
    CHECK(na > 1 && ca == farthest);
    mismatches += na != nb || std::memcmp(&ca, &cb, sizeof(double)) != 0 ||
                  std::memcmp(pa.data(), pb.data(), 3 * std::min(na, nb) * sizeof(int)) != 0;
    if (clearance) {
      CHECK(artp_field_clearance(many[b], da.data()) == ARTP_OK && artp_field_clearance(one, db.data()) == ARTP_OK);
      mismatches += std::memcmp(da.data(), db.data(), nodes * sizeof(uint16_t)) != 0;
    }
    artp_field_destroy(one);
  }
  return mismatches;
}

// matrix (n x n) against the forward single fields of the poses; returns the mismatches
static size_t compare_matrix(const std::vector<double>& mat, const std::vector<Pose>& poses,
                             const std::function<std::vector<double>(const std::vector<Pose>&, artp_field**)>& single) {
  const size_t n = poses.size();
  size_t mismatches = mat.size() != n * n;
  for (size_t i = 0; i < n && !mismatches; ++i) {
    const std::vector<double> dist = single({poses[i]}, nullptr);
    for (size_t j = 0; j < n; ++j) mismatches += std::memcmp(&dist[node_of(poses[j])], &mat[i * n + j], sizeof(double)) != 0;
    CHECK(mat[i * n + i] == 0.0);
  }
  return mismatches;
}

int main(int argc, char** argv) {
  const double res = 0.1, pos_x = 0.3, pos_y = -0.2;
  std::vector<float> elev(cells, 0.0f), trav(elev.size(), 1.0f);
  for (int c = 30; c < 42; ++c)
    for (int r = 40; r < 50; ++r) elev[r + static_cast<size_t>(c) * rows] = 0.6f;   // block
  for (int c = 5; c < 60; ++c)
    for (int r = 15; r < 18; ++r) elev[r + static_cast<size_t>(c) * rows] = -0.5f;  // trench
  auto params = std::make_shared<Params>();
  // shipped YAML robot (art_planner_ros/config/params.yaml:55-71)
  params->robot.torso.length = 1.31; params->robot.torso.width = 0.65; params->robot.torso.height = 0.3;
  params->robot.torso.offset.z = 0.04;
  params->robot.feet.offset.x = 0.51; params->robot.feet.offset.y = 0.2; params->robot.feet.offset.z = -0.475;
  params->robot.feet.reach.x = 0.2; params->robot.feet.reach.y = 0.2; params->robot.feet.reach.z = 0.2;
  params->objectives.custom_path_length.use_directional_cost = true;
  params->planner.prm_motion_cost.cost_weights.energy = 0.5f;
  params->planner.prm_motion_cost.cost_weights.time = 1.0f;
  params->planner.prm_motion_cost.cost_weights.risk = 2.0f;
  params->planner.prm_motion_cost.risk_threshold = 1.0f;   // the risk is 1 - probability: every edge is feasible
  std::unique_ptr<Planner> planner;
  try {
    planner.reset(new Planner(params, 0));
  } catch (const std::exception& e) {
    std::printf("no GPU context: %s\n", e.what());
    return 3;
  }
  if (argc < 2) {
    std::printf("usage: test_cost_field_many_weighted <weights.blob>\n");
    return 2;
  }
  std::ifstream in(argv[1], std::ios::binary);
  const std::vector<char> blob((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  if (blob.empty()) {
    std::printf("cannot read %s\n", argv[1]);
    return 2;
  }
  std::unique_ptr<Map> m(new Map);
  m->setGeometry(Map::Geometry{rows, cols, res, rows * res, cols * res, pos_x, pos_y});
  m->addLayer("elevation", elev.data());
  m->addLayer("traversability", trav.data());
  planner->setMap(std::move(m));
  artp_ctx* ctx = planner->gpu()->get();

  std::vector<uint32_t> mask = planner->computeReachability(n_yaw);
  CHECK(mask.size() == cells);
  if (mask.size() != cells) return 1;
  for (int c = 20; c < 24; ++c)
    for (int r = 50; r < 80; ++r) mask[r + static_cast<size_t>(c) * rows] = 0;  // a keep-out zone the caller draws
  // four poses: the first fully valid cell at or after four places spread over the map, at four headings
  const int want[4][2] = {{65, 10}, {30, 12}, {62, 50}, {25, 55}};
  std::vector<Pose> poses;
  for (int i = 0; i < 4; ++i) {
    Pose p{{-1, -1, (3 * i) % n_yaw}};
    for (int r = want[i][0]; r < rows && p[0] < 0; ++r)
      for (int c = want[i][1]; c < cols; ++c)
        if (mask[r + static_cast<size_t>(c) * rows] == (1u << n_yaw) - 1u) {
          p[0] = r;
          p[1] = c;
          break;
        }
    CHECK(p[0] >= 0);
    if (p[0] < 0) return 1;
    poses.push_back(p);
  }
  const Sets sets = {{poses[0]}, {poses[1], poses[2]}, {poses[3]}};

  // without a network the mirror passes the library's refusal on
  bool threw = false;
  try {
    planner->computeLearnedCostFields(mask, n_yaw, sets);
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);

  // the network on the map's heights: row-major, the row index growing along world x (the cost server's array)
  CHECK(artp_cost_load_weights(ctx, blob.data(), blob.size()) == ARTP_OK);
  std::vector<float> a(cells);
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) a[static_cast<size_t>(r) * cols + c] = elev[(rows - 1 - r) + static_cast<size_t>(cols - 1 - c) * rows];
  CHECK(artp_cost_update_map(ctx, a.data(), rows, cols, res, rows * res, cols * res, pos_x, pos_y) == ARTP_OK);
  if (fails) return 1;

  const auto learned = [&](const std::vector<Pose>& s, artp_field** keep) {
    return planner->computeLearnedCostField(mask, n_yaw, s, false, keep);
  };
  const double margin = 0.5, gain = 2.0;
  const int radius = 6;
  const auto clearance = [&](const std::vector<Pose>& s, artp_field** keep) {
    return planner->computeClearanceCostField(mask, n_yaw, s, margin, gain, radius, 0, false, false, keep);
  };
  std::vector<double> got(nodes);

  // ---- learned
  std::vector<artp_field*> many = planner->computeLearnedCostFields(mask, n_yaw, sets);
  CHECK(many.size() == sets.size());
  if (many.size() != sets.size()) return 1;
  size_t mismatches = compare_fields(many, sets, learned, false);
  std::printf("learned fields: %zu mismatches over %zu fields\n", mismatches, sets.size());
  CHECK(mismatches == 0);
  artp_field_destroy(many[0]);   // the fields live on their own tables: destroy the one that built, the others still answer
  CHECK(artp_field_dist(many[1], got.data()) == ARTP_OK);
  CHECK(got[node_of(poses[1])] == 0.0 && got[node_of(poses[2])] == 0.0);
  CHECK(artp_field_update_learned(many[2], nullptr, 0, nullptr) == ARTP_OK);   // nothing changed: the same bits
  CHECK(artp_field_dist(many[2], got.data()) == ARTP_OK);
  {
    const std::vector<double> dist = learned(sets[2], nullptr);
    CHECK(std::memcmp(got.data(), dist.data(), nodes * sizeof(double)) == 0);
  }
  artp_field_destroy(many[1]);
  artp_field_destroy(many[2]);

  artp_field_many_stats_t st1, st2;
  artp_field_many_table_stats_t ts1, ts2;
  const std::vector<double> mat = planner->computeLearnedCostMatrix(mask, n_yaw, poses, 0, &st1, &ts1);
  const std::vector<double> mat3 = planner->computeLearnedCostMatrix(mask, n_yaw, poses, 3, &st2, &ts2);
  CHECK(mat.size() == 16 && mat3.size() == 16);
  if (mat.size() != 16 || mat3.size() != 16) return 1;
  CHECK(st1.groups == 1 && st1.fields == 4 && st2.groups == 2 && st2.fields == 4);
  CHECK(ts1.table_builds == 1 && ts1.table_copies == 0 && ts2.table_builds == 1 && ts2.table_copies == 0);
  CHECK(ts1.table_bytes == 8 * ts1.table_rows && ts1.table_rows > 0 && ts1.build_ms > 0.0);
  size_t mat_mismatches = (std::memcmp(mat.data(), mat3.data(), 16 * sizeof(double)) != 0) + compare_matrix(mat, poses, learned);
  size_t asym = 0;
  for (size_t i = 0; i < 4; ++i)
    for (size_t j = 0; j < i; ++j) asym += mat[i * 4 + j] != mat[j * 4 + i];
  CHECK(asym > 0);   // the learned cost is not symmetric
  std::printf("learned matrix: %zu mismatches over 16 entries, %zu of 6 pairs differ from their transpose\n", mat_mismatches,
              asym);
  CHECK(mat_mismatches == 0);

  // ---- clearance-weighted
  many = planner->computeClearanceCostFields(mask, n_yaw, sets, margin, gain, radius);
  CHECK(many.size() == sets.size());
  if (many.size() != sets.size()) return 1;
  mismatches = compare_fields(many, sets, clearance, true);
  std::printf("clearance fields: %zu mismatches over %zu fields\n", mismatches, sets.size());
  CHECK(mismatches == 0);
  artp_field_destroy(many[0]);
  std::vector<uint16_t> d2(nodes);
  CHECK(artp_field_clearance(many[1], d2.data()) == ARTP_OK);
  CHECK(artp_field_dist(many[2], got.data()) == ARTP_OK && got[node_of(poses[3])] == 0.0);
  artp_field_destroy(many[1]);
  artp_field_destroy(many[2]);

  const std::vector<double> cmat = planner->computeClearanceCostMatrix(mask, n_yaw, poses, 0, margin, gain, radius, 0, false,
                                                                       &st1, &ts1);
  const std::vector<double> cmat3 = planner->computeClearanceCostMatrix(mask, n_yaw, poses, 3, margin, gain, radius, 0, false,
                                                                        &st2, &ts2);
  CHECK(cmat.size() == 16 && cmat3.size() == 16);
  if (cmat.size() != 16 || cmat3.size() != 16) return 1;
  CHECK(st1.groups == 1 && st2.groups == 2 && ts1.table_builds == 1 && ts2.table_builds == 1 && ts2.table_copies == 0);
  mat_mismatches = (std::memcmp(cmat.data(), cmat3.data(), 16 * sizeof(double)) != 0) + compare_matrix(cmat, poses, clearance);
  std::printf("clearance matrix: %zu mismatches over 16 entries\n", mat_mismatches);
  CHECK(mat_mismatches == 0);

  // a source in the keep-out zone, in set 1: the whole call throws and names the set
  for (int kind = 0; kind < 2; ++kind) {
    bool thrown = false;
    const Sets bad = {{poses[0]}, {poses[1], {{60, 21, 0}}}};
    try {
      if (kind == 0) planner->computeLearnedCostFields(mask, n_yaw, bad);
      else planner->computeClearanceCostFields(mask, n_yaw, bad, margin, gain, radius);
    } catch (const std::exception& e) {
      thrown = std::string(e.what()).find("set 1") != std::string::npos;
      if (!thrown) std::printf("unexpected text: %s\n", e.what());
    }
    CHECK(thrown);
  }
  return fails ? 1 : 0;
}
