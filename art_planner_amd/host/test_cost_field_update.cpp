// Exercises Planner::updateCostField (artp_field_update) through the host mirror on the map of test_cost_field.cpp:
// 90 x 70 cells at 0.1 m, flat ground with a raised block and a trench, the mask from Planner::computeReachability.
// A reverse field from one goal is computed and kept; a keep-out zone is drawn into the mask and the kept field updated
// with the zone's rectangle; then the zone is lifted again.  After each update dist must equal, bit for bit, a second
// computeCostField on the edited mask, the "cost_to_go" layer must follow, and a path of the kept field must avoid the zone.
//   test_cost_field_update
// Exit code 0 = every check holds; 3 = no GPU (the constructor throws: no CPU fallback).
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
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

struct HostPlanner : Planner {
  using Planner::Planner;
  const std::shared_ptr<Map>& mapPtr() const { return map_; }
};

static size_t differing(const std::vector<double>& a, const std::vector<double>& b) {
  if (a.size() != b.size()) return a.size() + b.size() + 1;
  size_t n = 0;
  for (size_t i = 0; i < a.size(); ++i) n += std::memcmp(&a[i], &b[i], sizeof(double)) != 0;
  return n;
}

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
  std::unique_ptr<HostPlanner> planner;
  try {
    planner.reset(new HostPlanner(params, 0));
  } catch (const std::exception& e) {
    std::printf("no GPU context: %s\n", e.what());
    return 3;
  }
  std::unique_ptr<Map> m(new Map);
  m->setGeometry(Map::Geometry{rows, cols, res, rows * res, cols * res, 0.3, -0.2});
  m->addLayer("elevation", elev.data());
  m->addLayer("traversability", trav.data());
  planner->setMap(std::move(m));

  const std::vector<uint32_t> mask = planner->computeReachability(n_yaw);
  const size_t cells = static_cast<size_t>(rows) * cols;
  CHECK(mask.size() == cells);
  if (mask.size() != cells) return 1;
  std::array<int, 3> goal{{-1, -1, 0}};
  for (int r = 60; r < 80 && goal[0] < 0; ++r)
    for (int c = 8; c < 16; ++c)
      if (mask[r + static_cast<size_t>(c) * rows] == (1u << n_yaw) - 1u) {
        goal = {{r, c, 0}};
        break;
      }
  CHECK(goal[0] >= 0);
  if (goal[0] < 0) return 1;

  artp_field* field = nullptr;
  const std::vector<double> first = planner->computeCostField(mask, n_yaw, {goal}, true, &field);
  CHECK(first.size() == cells * n_yaw && field != nullptr);
  if (first.size() != cells * n_yaw || !field) return 1;

  // a keep-out zone between the goal and the upper half of the map, open at one end only
  const std::array<int, 4> zone{{50, 20, 30, 4}};
  std::vector<uint32_t> edited = mask;
  for (int c = zone[1]; c < zone[1] + zone[3]; ++c)
    for (int r = zone[0]; r < zone[0] + zone[2]; ++r) edited[r + static_cast<size_t>(c) * rows] = 0;
  const std::vector<double> updated = planner->updateCostField(field, edited, &zone);
  const std::vector<double> anew = planner->computeCostField(edited, n_yaw, {goal}, true);
  const size_t mism1 = differing(updated, anew);
  CHECK(mism1 == 0);
  CHECK(differing(updated, first) > 0);
  artp_field_update_stats_t us;
  CHECK(artp_field_update_stats(field, &us) == ARTP_OK);
  CHECK(us.changed_words > 0 && us.removed_nodes > 0 && us.added_nodes == 0 && us.dead_nodes > 0);
  size_t finite = 0;
  for (double d : anew) finite += std::isfinite(d);
  CHECK(us.reached_nodes == finite);
  artp_field_stats_t st;
  CHECK(artp_field_stats(field, &st) == ARTP_OK && st.reached_nodes == finite);

  // the layer follows the update (computeCostField above wrote the same numbers; write it again from the update)
  const std::vector<double> again = planner->updateCostField(field, edited);   // nothing changes
  CHECK(differing(again, anew) == 0);
  CHECK(artp_field_update_stats(field, &us) == ARTP_OK && us.changed_words == 0 && us.dead_nodes == 0);
  const std::shared_ptr<Map>& map = planner->mapPtr();
  CHECK(map && map->exists("cost_to_go"));
  if (map && map->exists("cost_to_go")) {
    const std::vector<float>& layer = map->getLayer("cost_to_go");
    size_t wrong = layer.size() != cells;
    for (size_t i = 0; i < cells && i < layer.size(); ++i) {
      double b = INFINITY;
      for (int k = 0; k < n_yaw; ++k) b = std::min(b, again[i * n_yaw + k]);
      wrong += layer[i] != static_cast<float>(b);
    }
    CHECK(wrong == 0);
  }

  // a path of the kept field from beyond the zone ends at the goal and stays out of the zone
  std::array<int, 3> from{{-1, -1, 0}};
  for (int r = 55; r < 75 && from[0] < 0; ++r)
    for (int c = 30; c < 60; ++c)
      if (std::isfinite(again[(r + static_cast<size_t>(c) * rows) * n_yaw])) {
        from = {{r, c, 0}};
        break;
      }
  CHECK(from[0] >= 0);
  size_t n = 0;
  if (from[0] >= 0) {
    std::vector<int> nodes(3 * 4096);
    double cost = 0.0;
    CHECK(artp_field_path(field, from.data(), nodes.data(), nullptr, 4096, &n, &cost) == ARTP_OK);
    CHECK(n > 1 && cost == again[(from[0] + static_cast<size_t>(from[1]) * rows) * n_yaw]);
    if (n > 1) {
      CHECK(nodes[0] == from[0] && nodes[1] == from[1] && nodes[2] == from[2]);   // a reverse field: travel order
      CHECK(nodes[3 * (n - 1)] == goal[0] && nodes[3 * (n - 1) + 1] == goal[1] && nodes[3 * (n - 1) + 2] == goal[2]);
      size_t off = 0;
      for (size_t i = 0; i < n; ++i)
        off += !((edited[nodes[3 * i] + static_cast<size_t>(nodes[3 * i + 1]) * rows] >> nodes[3 * i + 2]) & 1u);
      CHECK(off == 0);
    }
  }

  // lifting the zone again gives the first field back
  const std::vector<double> lifted = planner->updateCostField(field, mask, &zone);
  const size_t mism2 = differing(lifted, first);
  CHECK(mism2 == 0);
  CHECK(artp_field_update_stats(field, &us) == ARTP_OK && us.added_nodes > 0 && us.removed_nodes == 0);

  // a mask without the goal is refused and the field stays
  std::vector<uint32_t> no_goal = mask;
  no_goal[goal[0] + static_cast<size_t>(goal[1]) * rows] &= ~1u;
  bool threw = false;
  try {
    planner->updateCostField(field, no_goal);
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
  std::vector<double> kept(cells * n_yaw);
  CHECK(artp_field_dist(field, kept.data()) == ARTP_OK && differing(kept, first) == 0);
  artp_field_destroy(field);

  std::printf("cost field update: %zu of %zu nodes reached behind the zone, path of %zu states, %zu + %zu mismatches\n",
              finite, cells * n_yaw, n, mism1, mism2);
  return fails ? 1 : 0;
}
