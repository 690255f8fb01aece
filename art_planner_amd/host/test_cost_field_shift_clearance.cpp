// Exercises Planner::shiftClearanceCostField (artp_field_shift_clearance) through the host mirror.  The world and the
// windows of test_cost_field_shift.cpp: 110 x 90 cells at 0.1 m, flat ground with a raised block and a trench, the
// planner's map a 90 x 70 window of it.  A reverse clearance-weighted field from one goal is computed and kept on the first
// window; the second window (moved by (6, -4) cells) is set, its mask computed, and the kept field carried across.  dist
// must equal, bit for bit, a second computeClearanceCostField on the new map with the goal moved, the "cost_to_go" layer
// must follow, and the refusals must throw and leave the field as it was.  Then the same back onto the first window.
//   test_cost_field_shift_clearance
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

static const int kWorldRows = 110, kWorldCols = 90, kRows = 90, kCols = 70;
static const double kRes = 0.1;

// the window whose cell (0, 0) is world cell (top, left); a window further up the rows lies further along +x
// (pos_top, pos_left: the corner the map's position claims; a refusal needs no matching heights)
static std::unique_ptr<Map> window(const std::vector<float>& world, int top, int left, int pos_top, int pos_left) {
  std::vector<float> elev(static_cast<size_t>(kRows) * kCols), trav(elev.size(), 1.0f);
  for (int c = 0; c < kCols; ++c)
    for (int r = 0; r < kRows; ++r)
      elev[r + static_cast<size_t>(c) * kRows] = world[(top + r) + static_cast<size_t>(left + c) * kWorldRows];
  std::unique_ptr<Map> m(new Map);
  m->setGeometry(Map::Geometry{kRows, kCols, kRes, kRows * kRes, kCols * kRes, 0.3 - pos_top * kRes, -0.2 - pos_left * kRes});
  m->addLayer("elevation", elev.data());
  m->addLayer("traversability", trav.data());
  return m;
}
static std::unique_ptr<Map> window(const std::vector<float>& world, int top, int left) { return window(world, top, left, top, left); }

int main() {
  const int n_yaw = 8, top = 10, left = 8, si = 6, sj = -4;
  const double margin = 0.35, gain = 2.5;
  const int radius = 4;
  std::vector<float> world(static_cast<size_t>(kWorldRows) * kWorldCols, 0.0f);
  for (int c = 40; c < 52; ++c)
    for (int r = 50; r < 60; ++r) world[r + static_cast<size_t>(c) * kWorldRows] = 0.6f;   // block
  for (int c = 15; c < 70; ++c)
    for (int r = 25; r < 28; ++r) world[r + static_cast<size_t>(c) * kWorldRows] = -0.5f;  // trench
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
  const size_t cells = static_cast<size_t>(kRows) * kCols;
  const uint32_t full = (1u << n_yaw) - 1u;
  auto compute = [&](const std::vector<uint32_t>& mask, const std::array<int, 3>& g, artp_field** keep) {
    return planner->computeClearanceCostField(mask, n_yaw, {g}, margin, gain, radius, 0, false, true, keep);
  };

  // the new window first: the goal must be a node of both masks
  planner->setMap(window(world, top - si, left - sj));
  const std::vector<uint32_t> mask_new = planner->computeReachability(n_yaw);
  planner->setMap(window(world, top, left));
  const std::vector<uint32_t> mask_old = planner->computeReachability(n_yaw);
  CHECK(mask_old.size() == cells && mask_new.size() == cells);
  if (mask_old.size() != cells || mask_new.size() != cells) return 1;
  std::array<int, 3> goal{{-1, -1, 0}};
  for (int r = 55; r < 75 && goal[0] < 0; ++r)
    for (int c = 12; c < 22; ++c)
      if (mask_old[r + static_cast<size_t>(c) * kRows] == full && mask_new[(r + si) + static_cast<size_t>(c + sj) * kRows] == full) {
        goal = {{r, c, 0}};
        break;
      }
  CHECK(goal[0] >= 0);
  if (goal[0] < 0) return 1;
  const std::array<int, 3> goal_new{{goal[0] + si, goal[1] + sj, 0}};

  artp_field *field = nullptr, *plain = nullptr;
  const std::vector<double> first = compute(mask_old, goal, &field);
  CHECK(first.size() == cells * n_yaw && field != nullptr);
  if (first.size() != cells * n_yaw || !field) return 1;
  std::vector<uint16_t> d2_first(cells * n_yaw);
  CHECK(artp_field_clearance(field, d2_first.data()) == ARTP_OK);
  const std::vector<double> first_plain = planner->computeCostField(mask_old, n_yaw, {goal}, true, &plain);
  CHECK(plain != nullptr && differing(first_plain, first) > 0);      // the weights do something
  if (!plain) return 1;

  // refusals: each throws, the field stays
  auto refused = [&](artp_field* f, const std::vector<double>& was, const std::vector<uint32_t>& mask) {
    bool threw = false;
    try {
      planner->shiftClearanceCostField(f, mask);
    } catch (const std::exception&) {
      threw = true;
    }
    std::vector<double> kept(cells * n_yaw);
    return threw && artp_field_dist(f, kept.data()) == ARTP_OK && differing(kept, was) == 0;
  };
  std::vector<uint32_t> no_goal = mask_new;
  no_goal[goal_new[0] + static_cast<size_t>(goal_new[1]) * kRows] &= ~1u;
  planner->setMap(window(world, top - si, left - sj));
  CHECK(refused(field, first, no_goal));                           // the moved goal is no node of the mask
  CHECK(refused(field, first, std::vector<uint32_t>(cells - 1, full)));   // a mask of another size
  CHECK(refused(plain, first_plain, mask_new));                    // a field that is not clearance-weighted
  artp_field_destroy(plain);
  planner->setMap(window(world, top, left, top - 40, left));       // a map 40 rows further on: the goal's row + 40 >= 90
  CHECK(goal[0] + 40 >= kRows && refused(field, first, mask_new)); // the goal leaves the map
  artp_field_clearance_shift_stats_t ss;
  CHECK(artp_field_clearance_shift_stats(field, &ss) == ARTP_OK && ss.reached_nodes == 0 && ss.shift_rows == 0);   // nothing stored
  std::vector<uint16_t> d2(cells * n_yaw);
  CHECK(artp_field_clearance(field, d2.data()) == ARTP_OK && d2 == d2_first);

  // the move
  planner->setMap(window(world, top - si, left - sj));
  const std::vector<double> shifted = planner->shiftClearanceCostField(field, mask_new);
  artp_field* fresh = nullptr;
  const std::vector<double> anew = compute(mask_new, goal_new, &fresh);
  const size_t mism1 = differing(shifted, anew);
  CHECK(mism1 == 0);
  CHECK(fresh != nullptr);
  if (fresh) {
    std::vector<uint16_t> d2_new(cells * n_yaw);
    CHECK(artp_field_clearance(fresh, d2_new.data()) == ARTP_OK && artp_field_clearance(field, d2.data()) == ARTP_OK && d2 == d2_new);
    artp_field_destroy(fresh);
  }
  CHECK(artp_field_clearance_shift_stats(field, &ss) == ARTP_OK);
  CHECK(ss.shift_rows == si && ss.shift_cols == sj && ss.kept_cells == static_cast<uint64_t>(kRows - 6) * (kCols - 4));
  CHECK(ss.left_nodes > 0 && ss.added_nodes > 0 && ss.changed_slots > 0 && ss.weight_tiles > 0);
  size_t finite = 0;
  for (double d : anew) finite += std::isfinite(d);
  CHECK(ss.reached_nodes == finite && finite > 0);
  artp_field_stats_t st;
  CHECK(artp_field_stats(field, &st) == ARTP_OK && st.reached_nodes == finite);

  // the layer follows (compute above wrote the same numbers; write it again from a move by nothing)
  const std::vector<double> again = planner->shiftClearanceCostField(field, mask_new);
  CHECK(differing(again, anew) == 0);
  CHECK(artp_field_clearance_shift_stats(field, &ss) == ARTP_OK && ss.shift_rows == 0 && ss.shift_cols == 0 &&
        ss.changed_words == 0 && ss.changed_slots == 0 && ss.dead_nodes == 0);
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

  // a path of the carried field ends at the moved goal, on nodes of the new mask, with the new map's poses
  std::array<int, 3> from{{-1, -1, 0}};
  for (int r = 10; r < 80 && from[0] < 0; ++r)
    for (int c = 35; c < 60; ++c)
      if (std::isfinite(again[(r + static_cast<size_t>(c) * kRows) * n_yaw])) {
        from = {{r, c, 0}};
        break;
      }
  CHECK(from[0] >= 0);
  size_t n = 0;
  if (from[0] >= 0) {
    std::vector<int> nodes(3 * 4096);
    std::vector<double> se3(7 * 4096);
    double cost = 0.0;
    CHECK(artp_field_path(field, from.data(), nodes.data(), se3.data(), 4096, &n, &cost) == ARTP_OK);
    CHECK(n > 1 && cost == again[(from[0] + static_cast<size_t>(from[1]) * kRows) * n_yaw]);
    if (n > 1) {
      CHECK(nodes[3 * (n - 1)] == goal_new[0] && nodes[3 * (n - 1) + 1] == goal_new[1] && nodes[3 * (n - 1) + 2] == 0);
      const double x_goal = (0.3 - (top - si) * kRes) + (0.5 * kRows * kRes - 0.5 * kRes) - kRes * goal_new[0];
      CHECK(std::fabs(se3[7 * (n - 1)] - x_goal) < 1e-9);
    }
  }

  // and back: the first window again gives the first field, against a second compute there
  planner->setMap(window(world, top, left));
  const std::vector<double> back = planner->shiftClearanceCostField(field, mask_old);
  const std::vector<double> anew_old = compute(mask_old, goal, nullptr);
  const size_t mism2 = differing(back, anew_old);
  CHECK(mism2 == 0 && differing(back, first) == 0);
  CHECK(artp_field_clearance_shift_stats(field, &ss) == ARTP_OK && ss.shift_rows == -si && ss.shift_cols == -sj);
  CHECK(artp_field_clearance(field, d2.data()) == ARTP_OK && d2 == d2_first);
  artp_field_destroy(field);

  std::printf("clearance cost field shift: %zu of %zu nodes reached on the new map, path of %zu states, %zu + %zu mismatches\n",
              finite, cells * n_yaw, n, mism1, mism2);
  return fails ? 1 : 0;
}
