// Exercises Planner::computeReachability (artp_reachability_map) through the host mirror on a map built here:
// 90 x 70 cells at 0.1 m, flat ground with a raised block and a trench.  Every mask bit must equal
// artp_validate_states on the lattice poses artp_reachability_poses hands out, and the planner's Map must carry the
// "reachability" layer (valid headings / n_yaw).
//   test_reachability
// Exit code 0 = every check holds; 3 = no GPU (the constructor throws: no CPU fallback).
#include <cmath>
#include <cstdio>
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

// PlannerRos publishes the planner's map_ (planner_ros.cpp:339): a subclass sees it
struct HostPlanner : Planner {
  using Planner::Planner;
  const std::shared_ptr<Map>& mapPtr() const { return map_; }
};

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
  artp_ctx* ctx = planner->gpu()->get();
  std::vector<double> poses(cells * n_yaw * 7);
  throwOnError(ctx, artp_reachability_poses(ctx, n_yaw, nullptr, poses.data()), "artp_reachability_poses");
  std::vector<uint8_t> valid(cells * n_yaw);
  throwOnError(ctx, artp_validate_states(ctx, poses.data(), valid.size(), valid.data(), nullptr), "artp_validate_states");
  size_t mismatches = 0, full = 0, none = 0, finite = 0;
  for (size_t i = 0; i < cells; ++i) {
    uint32_t bits = 0;
    for (int k = 0; k < n_yaw; ++k) bits |= (valid[i * n_yaw + k] ? 1u : 0u) << k;
    bool fin = true;
    for (int k = 0; k < n_yaw; ++k)
      for (int j = 0; j < 7; ++j) fin = fin && std::isfinite(poses[(i * n_yaw + k) * 7 + j]);
    finite += fin;
    mismatches += mask[i] != bits;
    full += mask[i] == (1u << n_yaw) - 1u;
    none += mask[i] == 0u;
  }
  CHECK(finite == cells);
  CHECK(mismatches == 0);
  CHECK(full > 0 && none > 0 && full + none < cells);  // standable, blocked and partly blocked cells
  // the layer the planner's map now carries, read the way a PlannerRos-shaped subclass reaches map_
  const std::shared_ptr<Map>& map = planner->mapPtr();
  CHECK(map && map->exists("reachability"));
  if (map && map->exists("reachability")) {
    const std::vector<float>& layer = map->getLayer("reachability");
    CHECK(layer.size() == cells);
    size_t bad = 0;
    for (size_t i = 0; i < cells && i < layer.size(); ++i)
      bad += layer[i] != static_cast<float>(__builtin_popcount(mask[i])) / static_cast<float>(n_yaw);
    CHECK(bad == 0);
  }
  // a second call at another heading count replaces the layer
  const std::vector<uint32_t> mask1 = planner->computeReachability(1);
  size_t agree = 0;
  for (size_t i = 0; i < cells; ++i) agree += (mask1[i] & 1u) == (mask[i] & 1u);   // bin 0 is heading 0 at both counts
  CHECK(agree == cells);
  CHECK(map->getLayer("reachability")[0] == static_cast<float>(mask1[0]));
  std::printf("reachability: %zu cells x %d headings, %zu all valid, %zu none, %zu mismatches\n", cells, n_yaw, full, none,
              mismatches);
  return fails ? 1 : 0;
}
