// Exercises Planner::computeCostFields (artp_field_compute_many) and Planner::computeCostMatrix (artp_field_cost_matrix)
// through the host mirror on the map of test_cost_field.cpp: 90 x 70 cells at 0.1 m, flat ground with a raised block and a
// trench, the mask from Planner::computeReachability with a keep-out zone cut into it.  Four source sets (one of two
// sources) go through one batched call; every field is compared bit for bit with Planner::computeCostField on its set --
// dist, reached_nodes and the path to the set's farthest node -- and stays usable after its neighbours are destroyed.
// The matrix of five poses is compared with those fields' dist at the poses, in one group and in groups of two.  A bad
// source in set 1 throws, names the set and leaves no field behind.
//   test_cost_field_many
// Exit code 0 = every check holds; 3 = no GPU (the constructor throws: no CPU fallback).
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
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

int main() {
  const int rows = 90, cols = 70, n_yaw = 8;
  const double res = 0.1;
  std::vector<float> elev(static_cast<size_t>(rows) * cols, 0.0f), trav(elev.size(), 1.0f);
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
  std::unique_ptr<Planner> planner;
  try {
    planner.reset(new Planner(params, 0));
  } catch (const std::exception& e) {
    std::printf("no GPU context: %s\n", e.what());
    return 3;
  }
  std::unique_ptr<Map> m(new Map);
  m->setGeometry(Map::Geometry{rows, cols, res, rows * res, cols * res, 0.3, -0.2});
  m->addLayer("elevation", elev.data());
  m->addLayer("traversability", trav.data());
  planner->setMap(std::move(m));

  std::vector<uint32_t> mask = planner->computeReachability(n_yaw);
  const size_t cells = static_cast<size_t>(rows) * cols, nodes = cells * n_yaw;
  CHECK(mask.size() == cells);
  if (mask.size() != cells) return 1;
  for (int c = 20; c < 24; ++c)
    for (int r = 50; r < 80; ++r) mask[r + static_cast<size_t>(c) * rows] = 0;  // a keep-out zone the caller draws
  // five poses: the first fully valid cell at or after five places spread over the map, at five headings
  const int want[5][2] = {{65, 10}, {30, 12}, {62, 50}, {25, 55}, {8, 35}};
  std::vector<std::array<int, 3>> poses;
  for (int i = 0; i < 5; ++i) {
    std::array<int, 3> p{{-1, -1, (3 * i) % n_yaw}};
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
  const std::vector<std::vector<std::array<int, 3>>> sets = {{poses[0]}, {poses[1], poses[2]}, {poses[3]}, {poses[4]}};

  std::vector<artp_field*> many = planner->computeCostFields(mask, n_yaw, sets);
  CHECK(many.size() == sets.size());
  if (many.size() != sets.size()) return 1;
  size_t mismatches = 0, reached_total = 0;
  std::vector<double> got(nodes);
  std::vector<int> pa(3 * nodes), pb(3 * nodes);
  for (size_t b = 0; b < sets.size(); ++b) {
    CHECK(many[b] != nullptr);
    if (!many[b]) return 1;
    artp_field* single = nullptr;
    const std::vector<double> dist = planner->computeCostField(mask, n_yaw, sets[b], false, &single);
    CHECK(single != nullptr && dist.size() == nodes);
    if (!single || dist.size() != nodes) return 1;
    CHECK(artp_field_dist(many[b], got.data()) == ARTP_OK);
    mismatches += std::memcmp(got.data(), dist.data(), nodes * sizeof(double)) != 0;
    artp_field_stats_t sm, ss;
    CHECK(artp_field_stats(many[b], &sm) == ARTP_OK && artp_field_stats(single, &ss) == ARTP_OK);
    mismatches += sm.reached_nodes != ss.reached_nodes || sm.nodes != ss.nodes || sm.tiles != ss.tiles;
    CHECK(sm.outer_rounds > 0 && sm.hop_rounds > 0 && sm.plain_sweeps == 0);
    reached_total += sm.reached_nodes;
    for (const auto& s : sets[b]) CHECK(dist[(s[0] + static_cast<size_t>(s[1]) * rows) * n_yaw + s[2]] == 0.0);
    // the path to the farthest node of this field: the same states from both
    size_t far = 0;
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
    CHECK(artp_field_path(single, target, pb.data(), nullptr, nodes, &nb, &cb) == ARTP_OK);
    CHECK(na > 1 && ca == farthest);
    mismatches += na != nb || std::memcmp(&ca, &cb, sizeof(double)) != 0 ||
                  std::memcmp(pa.data(), pb.data(), 3 * std::min(na, nb) * sizeof(int)) != 0;
    artp_field_destroy(single);
  }
  std::printf("cost fields: %zu mismatches over %zu fields, %zu nodes reached in all\n", mismatches, sets.size(),
              reached_total);
  CHECK(mismatches == 0);

  // the matrix against the fields: row i = dist of the forward field of pose i at the five poses
  artp_field_many_stats_t st1, st2;
  const std::vector<double> mat = planner->computeCostMatrix(mask, n_yaw, poses, 0, &st1);
  const std::vector<double> mat2 = planner->computeCostMatrix(mask, n_yaw, poses, 2, &st2);
  CHECK(mat.size() == 25 && mat2.size() == 25);
  if (mat.size() != 25 || mat2.size() != 25) return 1;
  CHECK(st1.groups == 1 && st1.fields == 5 && st2.groups == 3 && st2.fields == 5);
  CHECK(st1.dist_rounds > 0 && st1.hop_rounds > 0 && st1.tile_runs > 0);
  size_t mat_mismatches = std::memcmp(mat.data(), mat2.data(), 25 * sizeof(double)) != 0;
  const size_t row_of_field[4] = {0, 1, 3, 4};   // sets 0, 2, 3 are single poses 0, 3, 4; pose 1 and 2 share set 1
  for (size_t b = 0; b < sets.size(); ++b) {
    if (sets[b].size() != 1) continue;
    CHECK(artp_field_dist(many[b], got.data()) == ARTP_OK);
    for (size_t j = 0; j < 5; ++j) {
      const double d = got[(poses[j][0] + static_cast<size_t>(poses[j][1]) * rows) * n_yaw + poses[j][2]];
      mat_mismatches += std::memcmp(&d, &mat[row_of_field[b] * 5 + j], sizeof(double)) != 0;
    }
  }
  for (size_t i = 1; i <= 2; ++i) {   // poses 1 and 2: their own single fields
    artp_field* single = nullptr;
    const std::vector<double> dist = planner->computeCostField(mask, n_yaw, {poses[i]}, false, &single);
    for (size_t j = 0; j < 5; ++j) {
      const double d = dist[(poses[j][0] + static_cast<size_t>(poses[j][1]) * rows) * n_yaw + poses[j][2]];
      mat_mismatches += std::memcmp(&d, &mat[i * 5 + j], sizeof(double)) != 0;
    }
    artp_field_destroy(single);
  }
  for (size_t i = 0; i < 5; ++i) CHECK(mat[i * 5 + i] == 0.0);
  std::printf("cost matrix: %zu mismatches over 25 entries, %llu + %llu rounds in one group\n", mat_mismatches,
              static_cast<unsigned long long>(st1.dist_rounds), static_cast<unsigned long long>(st1.hop_rounds));
  CHECK(mat_mismatches == 0);

  // the fields live on their own: destroy two, the others still answer
  artp_field_destroy(many[0]);
  artp_field_destroy(many[2]);
  CHECK(artp_field_dist(many[1], got.data()) == ARTP_OK);
  CHECK(got[(poses[1][0] + static_cast<size_t>(poses[1][1]) * rows) * n_yaw + poses[1][2]] == 0.0);
  CHECK(got[(poses[2][0] + static_cast<size_t>(poses[2][1]) * rows) * n_yaw + poses[2][2]] == 0.0);
  CHECK(artp_field_dist(many[3], got.data()) == ARTP_OK);
  artp_field_destroy(many[1]);
  artp_field_destroy(many[3]);

  // a source in the keep-out zone, in set 1: the whole call throws and names the set
  bool thrown = false;
  try {
    planner->computeCostFields(mask, n_yaw, {{poses[0]}, {poses[1], {{60, 21, 0}}}});
  } catch (const std::exception& e) {
    thrown = std::string(e.what()).find("set 1") != std::string::npos;
    if (!thrown) std::printf("unexpected text: %s\n", e.what());
  }
  CHECK(thrown);
  thrown = false;
  try {
    planner->computeCostFields(mask, n_yaw, {});
  } catch (const std::exception&) {
    thrown = true;
  }
  CHECK(thrown);
  return fails ? 1 : 0;
}
