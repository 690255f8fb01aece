// Exercises Planner::computeLearnedCostField (artp_field_compute_learned) through the host mirror on a map built here:
// 90 x 70 cells at 0.1 m, flat ground with a raised block and a trench, the mask from Planner::computeReachability.  The
// motion-cost network comes from the blob file named on the command line (the runner writes seeded random parameters).
// Checked: the mirror's field equals, bit for bit, the C call with the planner's weights and threshold; the source costs
// 0; the field is not the reverse field (the learned cost is not symmetric); the planner's Map carries "cost_to_go";
// a kept learned field is refused by updateCostField.
//   test_cost_field_learned <weights.blob>
// Exit code 0 = every check holds; 3 = no GPU (the constructor throws: no CPU fallback); 2 = no blob file.
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
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

int main(int argc, char** argv) {
  const int rows = 90, cols = 70, n_yaw = 4;
  const double res = 0.1, pos_x = 0.3, pos_y = -0.2;
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
  params->planner.prm_motion_cost.cost_weights.energy = 0.5f;
  params->planner.prm_motion_cost.cost_weights.time = 1.0f;
  params->planner.prm_motion_cost.cost_weights.risk = 2.0f;
  params->planner.prm_motion_cost.risk_threshold = 1.0f;   // the risk is 1 - probability: every edge is feasible
  std::unique_ptr<HostPlanner> planner;
  try {
    planner.reset(new HostPlanner(params, 0));
  } catch (const std::exception& e) {
    std::printf("no GPU context: %s\n", e.what());
    return 3;
  }
  if (argc < 2) {
    std::printf("usage: test_cost_field_learned <weights.blob>\n");
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

  const size_t cells = static_cast<size_t>(rows) * cols;
  std::vector<uint32_t> mask = planner->computeReachability(n_yaw);
  CHECK(mask.size() == cells);
  if (mask.size() != cells) return 1;
  std::array<int, 3> src{{-1, -1, 0}};
  for (int r = 60; r < 80 && src[0] < 0; ++r)
    for (int c = 8; c < 16; ++c)
      if (mask[r + static_cast<size_t>(c) * rows] == (1u << n_yaw) - 1u) {
        src = {{r, c, 0}};
        break;
      }
  CHECK(src[0] >= 0);
  if (src[0] < 0) return 1;

  // without a network the mirror passes the library's refusal on
  bool threw = false;
  try {
    planner->computeLearnedCostField(mask, n_yaw, {src});
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

  artp_field* field = nullptr;
  const std::vector<double> dist = planner->computeLearnedCostField(mask, n_yaw, {src}, false, &field);
  CHECK(dist.size() == cells * n_yaw && field != nullptr);
  if (dist.size() != cells * n_yaw || !field) return 1;
  CHECK(dist[(src[0] + static_cast<size_t>(src[1]) * rows) * n_yaw + src[2]] == 0.0);

  // the C call with the planner's numbers
  artp_field_learned_params lp;
  artp_field_learned_params_defaults(&lp);
  lp.w_energy = 0.5f;
  lp.w_time = 1.0f;
  lp.w_risk = 2.0f;
  lp.risk_threshold = 1.0f;
  artp_field* direct = nullptr;
  CHECK(artp_field_compute_learned(ctx, &lp, n_yaw, nullptr, mask.data(), 0, src.data(), 1, 0, &direct) == ARTP_OK);
  std::vector<double> want(cells * n_yaw, -1.0);
  if (direct) CHECK(artp_field_dist(direct, want.data()) == ARTP_OK);
  size_t differ = 0, finite = 0, outside = 0;
  for (size_t i = 0; i < dist.size(); ++i) {
    differ += std::memcmp(&dist[i], &want[i], sizeof(double)) != 0;
    finite += std::isfinite(dist[i]);
    outside += !((mask[i / n_yaw] >> (i % n_yaw)) & 1u) && !(std::isinf(dist[i]) && dist[i] > 0);
  }
  CHECK(differ == 0);
  CHECK(outside == 0);
  CHECK(finite > cells / 2);
  artp_field_stats_t st;
  CHECK(artp_field_stats(field, &st) == ARTP_OK);
  CHECK(st.reached_nodes == finite && st.outer_rounds > 0);
  artp_field_destroy(direct);

  const std::shared_ptr<Map>& map = planner->mapPtr();
  size_t wrong = 0;
  CHECK(map && map->exists("cost_to_go"));
  if (map && map->exists("cost_to_go")) {
    const std::vector<float>& layer = map->getLayer("cost_to_go");
    CHECK(layer.size() == cells);
    for (size_t i = 0; i < cells && i < layer.size(); ++i) {
      double b = INFINITY;
      for (int k = 0; k < n_yaw; ++k) b = std::min(b, dist[i * n_yaw + k]);
      wrong += layer[i] != static_cast<float>(b);
    }
    CHECK(wrong == 0);
  }

  // the cost TO the source is another field, and the layer follows the last call
  const std::vector<double> rev = planner->computeLearnedCostField(mask, n_yaw, {src}, true);
  size_t asym = 0;
  for (size_t i = 0; i < dist.size(); ++i) asym += std::isfinite(dist[i]) && rev[i] != dist[i];
  CHECK(asym > 0);
  if (map && map->exists("cost_to_go")) {
    const std::vector<float>& layer = map->getLayer("cost_to_go");
    size_t stale = 0;
    for (size_t i = 0; i < cells && i < layer.size(); ++i) {
      double b = INFINITY;
      for (int k = 0; k < n_yaw; ++k) b = std::min(b, rev[i * n_yaw + k]);
      stale += layer[i] != static_cast<float>(b);
    }
    CHECK(stale == 0);
  }

  threw = false;
  try {
    planner->updateCostField(field, mask);
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
  artp_field_destroy(field);

  std::printf("learned cost field: %zu of %zu nodes reached, %zu differ from the C call, %zu layer cells wrong, %zu nodes "
              "differ from the reverse field\n", finite, cells * n_yaw, differ, wrong, asym);
  return fails ? 1 : 0;
}
