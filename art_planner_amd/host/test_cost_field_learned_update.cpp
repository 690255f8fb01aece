// Exercises Planner::updateLearnedCostField (artp_field_update_learned) through the host mirror on the map of
// test_cost_field_learned.cpp: 90 x 70 cells at 0.1 m, flat ground with a raised block and a trench, the mask from
// Planner::computeReachability, the motion-cost network from the blob file named on the command line.
// A kept learned field is updated three times -- the cost map alone (a ramp added to the elevation the network sees), the
// mask alone (a keep-out zone, handed in with its rectangle), both at once -- and after each update compared, bit for bit,
// with a new computeLearnedCostField on the same state; the planner's Map must carry the updated "cost_to_go".
//   test_cost_field_learned_update <weights.blob>
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

static const int rows = 90, cols = 70, n_yaw = 4;
static const double res = 0.1, pos_x = 0.3, pos_y = -0.2;

// the network on these heights: row-major, the row index growing along world x (the cost server's array)
static int costMap(artp_ctx* ctx, const std::vector<float>& elev) {
  std::vector<float> a(elev.size());
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) a[static_cast<size_t>(r) * cols + c] = elev[(rows - 1 - r) + static_cast<size_t>(cols - 1 - c) * rows];
  return artp_cost_update_map(ctx, a.data(), rows, cols, res, rows * res, cols * res, pos_x, pos_y);
}

static size_t differing(const std::vector<double>& a, const std::vector<double>& b) {
  size_t n = a.size() == b.size() ? 0 : 1;
  for (size_t i = 0; i < a.size() && i < b.size(); ++i) n += std::memcmp(&a[i], &b[i], sizeof(double)) != 0;
  return n;
}

int main(int argc, char** argv) {
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
    std::printf("usage: test_cost_field_learned_update <weights.blob>\n");
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
  const std::vector<uint32_t> mask = planner->computeReachability(n_yaw);
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
  CHECK(artp_cost_load_weights(ctx, blob.data(), blob.size()) == ARTP_OK);
  CHECK(costMap(ctx, elev) == ARTP_OK);
  if (fails) return 1;

  artp_field* field = nullptr;
  const std::vector<double> first = planner->computeLearnedCostField(mask, n_yaw, {src}, true, &field);
  CHECK(first.size() == cells * n_yaw && field != nullptr);
  if (!field) return 1;

  // a field of the geometric objectives is refused, and so is a learned field by the mask-only call
  artp_field* plain = nullptr;
  planner->computeCostField(mask, n_yaw, {src}, true, &plain);
  bool threw = false;
  try {
    planner->updateLearnedCostField(plain, mask);
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
  artp_field_destroy(plain);
  threw = false;
  try {
    planner->updateCostField(field, mask);
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);

  // the three states: another cost map, another mask, both
  std::vector<float> ramp(elev);
  for (int c = 0; c < cols; ++c)
    for (int r = 0; r < rows; ++r) ramp[r + static_cast<size_t>(c) * rows] += 0.004f * static_cast<float>(r + c);
  std::vector<uint32_t> zone(mask);
  const std::array<int, 4> zone_rect{{60, 40, 12, 9}};   // a keep-out zone on open ground; the source lies outside it
  for (int c = zone_rect[1]; c < zone_rect[1] + zone_rect[3]; ++c)
    for (int r = zone_rect[0]; r < zone_rect[0] + zone_rect[2]; ++r) zone[r + static_cast<size_t>(c) * rows] = 0u;
  CHECK(src[1] < zone_rect[1]);
  size_t differ = 0, moved = 0, stale = 0;
  std::vector<double> last = first;
  for (int step = 0; step < 3; ++step) {
    const std::vector<uint32_t>& want_mask = step == 1 ? zone : mask;
    if (step != 1) CHECK(costMap(ctx, step == 0 ? ramp : elev) == ARTP_OK);
    std::vector<double> got;
    if (step == 0)
      got = planner->updateLearnedCostField(field, {});
    else if (step == 1)
      got = planner->updateLearnedCostField(field, zone, &zone_rect);
    else
      got = planner->updateLearnedCostField(field, mask);
    artp_field_learned_update_stats_t us;
    CHECK(artp_field_learned_update_stats(field, &us) == ARTP_OK);
    CHECK(us.repriced_slots > 0 && us.changed_slots > 0 && us.changed_slots <= us.repriced_slots);
    CHECK((us.changed_words > 0) == (step != 0));
    const std::shared_ptr<Map>& map = planner->mapPtr();
    CHECK(map && map->exists("cost_to_go"));
    if (map && map->exists("cost_to_go")) {
      const std::vector<float>& layer = map->getLayer("cost_to_go");
      CHECK(layer.size() == cells);
      for (size_t i = 0; i < cells && i < layer.size(); ++i) {
        double b = INFINITY;
        for (int k = 0; k < n_yaw; ++k) b = std::min(b, got[i * n_yaw + k]);
        stale += !(layer[i] == static_cast<float>(b));
      }
    }
    const std::vector<double> want = planner->computeLearnedCostField(want_mask, n_yaw, {src}, true);
    const size_t d = differing(got, want);
    std::printf("step %d: %llu of %llu slots changed, %llu words, %llu tile runs, %zu nodes differ from a new field\n", step,
                (unsigned long long)us.changed_slots, (unsigned long long)us.repriced_slots,
                (unsigned long long)us.changed_words, (unsigned long long)us.tile_launches, d);
    differ += d;
    moved += differing(got, last);
    last = got;
  }
  CHECK(differ == 0);
  CHECK(stale == 0);
  CHECK(moved > 0);
  CHECK(last[(src[0] + static_cast<size_t>(src[1]) * rows) * n_yaw + src[2]] == 0.0);
  artp_field_destroy(field);

  std::printf("learned cost field update: 3 updates moved %zu nodes, %zu layer cells stale, %zu differ from a new field\n", moved,
              stale, differ);
  return fails ? 1 : 0;
}
