// Exercises Planner::updateClearanceCostField (artp_field_update_clearance) through the host mirror on the map of
// test_cost_field_clearance.cpp: 90 x 70 cells at 0.1 m, flat ground with a raised block and a trench, the mask from
// Planner::computeReachability at 8 headings, the distance objective (heights count).
// A kept clearance field (radius 5, yaw_spread 1, margin 0.3 m, gain 2, reverse) is updated twice -- a keep-out zone handed
// in with its rectangle; then the zone lifted again while a ramp raised the ground inside the rectangle, with
// refresh_heights -- and after each update compared, bit for bit, with a new computeClearanceCostField on the same state;
// the planner's Map must carry the updated "cost_to_go".
//   test_cost_field_clearance_update
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

static const int rows = 90, cols = 70, n_yaw = 8;
static const double res = 0.1;

static size_t differing(const std::vector<double>& a, const std::vector<double>& b) {
  size_t n = a.size() == b.size() ? 0 : 1;
  for (size_t i = 0; i < a.size() && i < b.size(); ++i) n += std::memcmp(&a[i], &b[i], sizeof(double)) != 0;
  return n;
}

static void install(HostPlanner& planner, const std::vector<float>& elev, const std::vector<float>& trav) {
  std::unique_ptr<Map> m(new Map);
  m->setGeometry(Map::Geometry{rows, cols, res, rows * res, cols * res, 0.3, -0.2});
  m->addLayer("elevation", elev.data());
  m->addLayer("traversability", trav.data());
  planner.setMap(std::move(m));
}

int main() {
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
  params->objectives.custom_path_length.use_directional_cost = false;   // objective 0: the heights are in the costs
  std::unique_ptr<HostPlanner> planner;
  try {
    planner.reset(new HostPlanner(params, 0));
  } catch (const std::exception& e) {
    std::printf("no GPU context: %s\n", e.what());
    return 3;
  }
  install(*planner, elev, trav);

  const size_t cells = static_cast<size_t>(rows) * cols;
  const std::vector<uint32_t> mask = planner->computeReachability(n_yaw);
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

  const double margin = 0.3, gain = 2.0;
  const int R = 5, spread = 1;
  artp_field* field = nullptr;
  const std::vector<double> first = planner->computeClearanceCostField(mask, n_yaw, {goal}, margin, gain, R, spread, false, true, &field);
  CHECK(first.size() == cells * n_yaw && field != nullptr);
  if (!field) return 1;

  // a field of the geometric objectives is refused
  artp_field* plain = nullptr;
  planner->computeCostField(mask, n_yaw, {goal}, true, &plain);
  bool threw = false;
  try {
    planner->updateClearanceCostField(plain, mask);
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
  artp_field_destroy(plain);

  // the two states: a keep-out zone on open ground (the goal lies outside it); then the zone lifted, the ground under it
  // and around it raised by a ramp
  std::vector<uint32_t> zone(mask);
  const std::array<int, 4> zone_rect{{60, 40, 12, 9}};
  for (int c = zone_rect[1]; c < zone_rect[1] + zone_rect[3]; ++c)
    for (int r = zone_rect[0]; r < zone_rect[0] + zone_rect[2]; ++r) zone[r + static_cast<size_t>(c) * rows] = 0u;
  CHECK(goal[1] < zone_rect[1]);
  const std::array<int, 4> ramp_rect{{58, 38, 16, 13}};   // the zone grown by two cells
  std::vector<float> ramp(elev);
  for (int c = ramp_rect[1]; c < ramp_rect[1] + ramp_rect[3]; ++c)
    for (int r = ramp_rect[0]; r < ramp_rect[0] + ramp_rect[2]; ++r)
      ramp[r + static_cast<size_t>(c) * rows] += 0.002f * static_cast<float>((r - ramp_rect[0]) * (ramp_rect[0] + ramp_rect[2] - 1 - r));

  size_t differ = 0, moved = 0, stale = 0;
  std::vector<double> last = first;
  for (int step = 0; step < 2; ++step) {
    std::vector<double> got;
    if (step == 0) {
      got = planner->updateClearanceCostField(field, zone, &zone_rect);
    } else {
      install(*planner, ramp, trav);   // the same geometry: the kept field may re-read its heights
      got = planner->updateClearanceCostField(field, mask, &ramp_rect, true);
    }
    artp_field_clearance_update_stats_t us;
    CHECK(artp_field_clearance_update_stats(field, &us) == ARTP_OK);
    CHECK(us.changed_words > 0 && us.changed_d2 > 0 && us.changed_slots > 0 && us.changed_slots <= us.repriced_slots);
    CHECK(us.clearance_tiles > 0 && us.clearance_tiles < 6 * 5 && us.weight_tiles > 0);
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
    std::vector<uint16_t> own(cells * n_yaw), fresh_d2(cells * n_yaw);
    CHECK(artp_field_clearance(field, own.data()) == ARTP_OK);
    artp_field* fresh = nullptr;
    const std::vector<double> want =
        planner->computeClearanceCostField(step == 0 ? zone : mask, n_yaw, {goal}, margin, gain, R, spread, false, true, &fresh);
    CHECK(fresh != nullptr);
    if (!fresh) return 1;
    CHECK(artp_field_clearance(fresh, fresh_d2.data()) == ARTP_OK && own == fresh_d2);
    artp_field_destroy(fresh);
    const size_t d = differing(got, want);
    std::printf("step %d: %llu words, %llu clearances and %llu of %llu slots changed in %llu + %llu tiles, %llu tile runs, %zu "
                "nodes differ from a new field\n", step, (unsigned long long)us.changed_words,
                (unsigned long long)us.changed_d2, (unsigned long long)us.changed_slots, (unsigned long long)us.repriced_slots,
                (unsigned long long)us.clearance_tiles, (unsigned long long)us.weight_tiles,
                (unsigned long long)us.tile_launches, d);
    differ += d;
    moved += differing(got, last);
    last = got;
  }
  CHECK(differ == 0);
  CHECK(stale == 0);
  CHECK(moved > 0);
  CHECK(differing(last, first) > 0);   // the ramp stays in the costs although the mask is the first one again
  CHECK(last[(goal[0] + static_cast<size_t>(goal[1]) * rows) * n_yaw + goal[2]] == 0.0);
  artp_field_destroy(field);

  std::printf("clearance cost field update: 2 updates moved %zu nodes, %zu layer cells stale, %zu differ from a new field\n",
              moved, stale, differ);
  return fails ? 1 : 0;
}
