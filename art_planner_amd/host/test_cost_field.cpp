// Exercises Planner::computeCostField (artp_field_compute) through the host mirror on a map built here: 90 x 70 cells at
// 0.1 m, flat ground with a raised block and a trench, the mask from Planner::computeReachability with a keep-out zone
// cut into it.  Checked on the host: the source costs 0, nodes outside the mask are +inf, every finite node satisfies
// the Bellman equation over its ten moves for the flat-ground costs written out here, the keep-out zone is never entered,
// a path from the farthest node ends at the source with the field's cost, and the planner's Map carries "cost_to_go".
//   test_cost_field
// Exit code 0 = every check holds; 3 = no GPU (the constructor throws: no CPU fallback).
#include <array>
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

  std::vector<uint32_t> mask = planner->computeReachability(n_yaw);
  const size_t cells = static_cast<size_t>(rows) * cols;
  CHECK(mask.size() == cells);
  if (mask.size() != cells) return 1;
  for (int c = 20; c < 24; ++c)
    for (int r = 50; r < 80; ++r) mask[r + static_cast<size_t>(c) * rows] = 0;  // a keep-out zone the caller draws
  // the source: the first cell near the middle of the lower half where every heading is valid
  std::array<int, 3> src{{-1, -1, 0}};
  for (int r = 60; r < 80 && src[0] < 0; ++r)
    for (int c = 8; c < 16; ++c)
      if (mask[r + static_cast<size_t>(c) * rows] == (1u << n_yaw) - 1u) {
        src = {{r, c, 0}};
        break;
      }
  CHECK(src[0] >= 0);
  if (src[0] < 0) return 1;

  artp_field* field = nullptr;
  const std::vector<double> dist = planner->computeCostField(mask, n_yaw, {src}, false, &field);
  CHECK(dist.size() == cells * n_yaw && field != nullptr);
  if (dist.size() != cells * n_yaw || !field) return 1;
  auto at = [&](int r, int c, int k) { return dist[(r + static_cast<size_t>(c) * rows) * n_yaw + k]; };
  auto has = [&](int r, int c, int k) {
    return r >= 0 && r < rows && c >= 0 && c < cols && ((mask[r + static_cast<size_t>(c) * rows] >> k) & 1u);
  };
  CHECK(at(src[0], src[1], src[2]) == 0.0);
  // Bellman over the ten moves; objective 1 on the nominal lattice numbers
  const auto& v = params->objectives.custom_path_length;
  const int dr[8] = {-1, -1, -1, 0, 0, 1, 1, 1}, dc[8] = {-1, 0, 1, -1, 1, -1, 0, 1};
  const double turn = (2.0 * M_PI / n_yaw) / v.max_ang_vel;
  size_t bad = 0, finite = 0, outside = 0;
  double farthest = -1.0;
  std::array<int, 3> far{{0, 0, 0}};
  for (int c = 0; c < cols; ++c)
    for (int r = 0; r < rows; ++r)
      for (int k = 0; k < n_yaw; ++k) {
        const double d = at(r, c, k);
        if (!has(r, c, k)) {
          outside += !(std::isinf(d) && d > 0);
          continue;
        }
        double yaw = (2.0 * M_PI / n_yaw) * k;
        if (yaw > M_PI) yaw -= 2.0 * M_PI;
        double best = (r == src[0] && c == src[1] && k == src[2]) ? 0.0 : INFINITY;
        for (int j = 0; j < 8; ++j) {   // the move (r - dr, c - dc) -> (r, c)
          if (!has(r - dr[j], c - dc[j], k)) continue;
          const double dx = res * -dr[j], dy = res * -dc[j];
          const double lon = std::cos(yaw) * dx + std::sin(yaw) * dy, lat = -std::sin(yaw) * dx + std::cos(yaw) * dy;
          best = std::min(best, at(r - dr[j], c - dc[j], k) +
                                    std::max(std::fabs(lon) / v.max_lon_vel, std::fabs(lat) / v.max_lat_vel));
        }
        if (has(r, c, (k + 1) % n_yaw)) best = std::min(best, at(r, c, (k + 1) % n_yaw) + turn);
        if (has(r, c, (k + n_yaw - 1) % n_yaw)) best = std::min(best, at(r, c, (k + n_yaw - 1) % n_yaw) + turn);
        if (std::isinf(best) != std::isinf(d)) ++bad;
        else if (std::isfinite(d) && std::fabs(d - best) > 1e-9 * best) ++bad;
        if (std::isfinite(d)) {
          ++finite;
          if (d > farthest) {
            farthest = d;
            far = {{r, c, k}};
          }
        }
      }
  CHECK(bad == 0);
  CHECK(outside == 0);
  CHECK(finite > cells / 2);
  artp_field_stats_t st;
  CHECK(artp_field_stats(field, &st) == ARTP_OK);
  CHECK(st.reached_nodes == finite && st.outer_rounds > 0);

  // the path to the farthest node: source first, every state in the mask, the field's cost
  std::vector<int> nodes(3 * 4096);
  std::vector<double> se3(7 * 4096);
  size_t n = 0;
  double cost = 0.0;
  CHECK(artp_field_path(field, far.data(), nodes.data(), se3.data(), 4096, &n, &cost) == ARTP_OK);
  CHECK(n > 1 && cost == farthest);
  if (n > 1) {
    CHECK(nodes[0] == src[0] && nodes[1] == src[1] && nodes[2] == src[2]);
    CHECK(nodes[3 * (n - 1)] == far[0] && nodes[3 * (n - 1) + 1] == far[1] && nodes[3 * (n - 1) + 2] == far[2]);
    size_t off = 0;
    for (size_t i = 0; i < n; ++i) off += !has(nodes[3 * i], nodes[3 * i + 1], nodes[3 * i + 2]);
    CHECK(off == 0);
    size_t nonfinite = 0;
    for (size_t i = 0; i < 7 * n; ++i) nonfinite += !std::isfinite(se3[i]);
    CHECK(nonfinite == 0);
  }
  artp_field_destroy(field);

  const std::shared_ptr<Map>& map = planner->mapPtr();
  CHECK(map && map->exists("cost_to_go"));
  if (map && map->exists("cost_to_go")) {
    const std::vector<float>& layer = map->getLayer("cost_to_go");
    CHECK(layer.size() == cells);
    size_t wrong = 0;
    for (size_t i = 0; i < cells && i < layer.size(); ++i) {
      double b = INFINITY;
      for (int k = 0; k < n_yaw; ++k) b = std::min(b, dist[i * n_yaw + k]);
      wrong += layer[i] != static_cast<float>(b);
    }
    CHECK(wrong == 0);
  }
  std::printf("cost field: %zu of %zu nodes reached, farthest %.3f s in %zu states, %zu Bellman mismatches\n", finite,
              cells * n_yaw, farthest, n, bad);
  return fails ? 1 : 0;
}
