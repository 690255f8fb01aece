// Exercises Planner::blockCostFieldMoves, unblockCostField and planOnCostField (artp_field_block_moves, _unblock, _plan)
// through the host mirror on the map of test_cost_field.cpp: 90 x 70 cells at 0.1 m, flat ground with a raised block and a
// trench, the mask from Planner::computeReachability.  A reverse field from one goal is computed and kept.
//   1. a move in the middle of a path is blocked: dist must equal, bit for bit, a second field with the same move
//      blocked, the "cost_to_go" layer must follow and the new path must not use the move; unblocking gives the first
//      field back.
//   2. planOnCostField to eight targets: every move of every returned path passes artp_check_motions, a path's cost is
//      the kept field's dist at its target, and a second field with the same moves blocked holds the same bits.
//   test_cost_field_plan
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
  auto at = [&](const std::vector<double>& d, const std::array<int, 3>& v) {
    return d[(v[0] + static_cast<size_t>(v[1]) * rows) * n_yaw + v[2]];
  };

  // 1. the middle move of a path
  std::array<int, 3> from{{-1, -1, 0}};
  for (int r = 55; r < 75 && from[0] < 0; ++r)
    for (int c = 40; c < 60; ++c)
      if (std::isfinite(first[(r + static_cast<size_t>(c) * rows) * n_yaw])) {
        from = {{r, c, 0}};
        break;
      }
  CHECK(from[0] >= 0);
  if (from[0] < 0) return 1;
  std::vector<int> nodes(3 * 4096);
  size_t n = 0;
  double cost = 0.0;
  CHECK(artp_field_path(field, from.data(), nodes.data(), nullptr, 4096, &n, &cost) == ARTP_OK && n > 3);
  if (n <= 3) return 1;
  const size_t mid = n / 2;
  const std::array<int, 3> a{{nodes[3 * mid], nodes[3 * mid + 1], nodes[3 * mid + 2]}};
  const std::array<int, 3> b{{nodes[3 * mid + 3], nodes[3 * mid + 4], nodes[3 * mid + 5]}};
  uint64_t newly = 0;
  const std::vector<double> blocked = planner->blockCostFieldMoves(field, {a}, {b}, &newly);
  CHECK(newly == 1);
  artp_field* second = nullptr;
  planner->computeCostField(mask, n_yaw, {goal}, true, &second);
  CHECK(second != nullptr);
  if (!second) return 1;
  const std::vector<double> anew = planner->blockCostFieldMoves(second, {a}, {b});
  const size_t mism1 = differing(blocked, anew);
  CHECK(mism1 == 0);
  for (size_t i = 0; i < blocked.size(); ++i) CHECK(!(blocked[i] < first[i]));     // a block only raises distances
  double w = 0.0;
  CHECK(artp_field_edge_costs(field, a.data(), b.data(), 1, &w) == ARTP_OK && std::isinf(w));
  size_t n2 = 0;
  CHECK(artp_field_path(field, from.data(), nodes.data(), nullptr, 4096, &n2, &cost) == ARTP_OK);
  CHECK(cost == at(blocked, from));
  size_t used = 0;
  for (size_t i = 0; i + 1 < n2; ++i)
    used += std::memcmp(&nodes[3 * i], a.data(), 12) == 0 && std::memcmp(&nodes[3 * i + 3], b.data(), 12) == 0;
  CHECK(used == 0);
  const std::shared_ptr<Map>& map = planner->mapPtr();
  CHECK(map && map->exists("cost_to_go"));
  if (map && map->exists("cost_to_go")) {
    const std::vector<float>& layer = map->getLayer("cost_to_go");
    size_t wrong = layer.size() != cells;
    for (size_t i = 0; i < cells && i < layer.size(); ++i) {
      double best = INFINITY;
      for (int k = 0; k < n_yaw; ++k) best = std::min(best, anew[i * n_yaw + k]);
      wrong += layer[i] != static_cast<float>(best);
    }
    CHECK(wrong == 0);
  }
  bool threw = false;
  try {
    planner->blockCostFieldMoves(field, {a}, {{{a[0] + 2, a[1], a[2]}}});   // not a lattice move
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
  uint64_t cleared = 0;
  const std::vector<double> lifted = planner->unblockCostField(field, nullptr, &cleared);
  CHECK(cleared == 1 && differing(lifted, first) == 0);
  planner->unblockCostField(second);

  // 2. the lazy loop to eight targets spread over the map
  std::vector<std::array<int, 3>> targets;
  for (int r = 5; r < rows && targets.size() < 8; r += 11)
    for (int c = 62; c > 4 && targets.size() < 8; c -= 19)
      if (std::isfinite(first[(r + static_cast<size_t>(c) * rows) * n_yaw + 2])) targets.push_back({{r, c, 2}});
  CHECK(targets.size() == 8);
  const std::vector<Planner::CostFieldPlan> plans = planner->planOnCostField(field, targets);
  artp_field_plan_stats_t ps;
  CHECK(artp_field_plan_stats(field, &ps) == ARTP_OK && ps.rounds >= 1);
  std::vector<double> now(cells * n_yaw);
  CHECK(artp_field_dist(field, now.data()) == ARTP_OK);
  size_t solved = 0, bad_moves = 0, states = 0;
  for (size_t i = 0; i < plans.size(); ++i) {
    const Planner::CostFieldPlan& p = plans[i];
    CHECK(p.status == 0 || p.status == 1);
    if (p.status != 0) {
      CHECK(std::isinf(p.cost) && std::isinf(at(now, targets[i])));
      continue;
    }
    ++solved;
    states += p.states.size();
    CHECK(p.nodes.size() == p.states.size() && !p.nodes.empty());
    CHECK(p.nodes.front() == targets[i] && p.nodes.back() == goal);     // a reverse field: travel order
    CHECK(p.cost == at(now, targets[i]));
    if (p.states.size() > 1) {
      std::vector<uint8_t> ok(p.states.size() - 1);
      CHECK(artp_check_motions(planner->gpu()->get(), p.states[0].data(), p.states[1].data(), ok.size(), ok.data()) == ARTP_OK);
      for (uint8_t v : ok) bad_moves += !v;
    }
  }
  CHECK(solved > 0 && bad_moves == 0);
  uint64_t n_blocked = 0;
  CHECK(artp_field_blocked_count(field, &n_blocked) == ARTP_OK && n_blocked == ps.moves_blocked);
  // the same set on the second field, in one call
  std::vector<uint16_t> words(cells * n_yaw);
  CHECK(artp_field_blocked(field, words.data()) == ARTP_OK);
  std::vector<std::array<int, 3>> ba, bb;
  const int dr[8] = {-1, -1, -1, 0, 0, 1, 1, 1}, dc[8] = {-1, 0, 1, -1, 1, -1, 0, 1};
  for (size_t i = 0; i < words.size(); ++i)
    for (int j = 0; j < 10; ++j)
      if ((words[i] >> j) & 1u) {   // a reverse field stores the move v -> u at v under the move itself
        const int k = static_cast<int>(i % n_yaw), cell = static_cast<int>(i / n_yaw), r = cell % rows, c = cell / rows;
        ba.push_back({{r, c, k}});
        bb.push_back(j < 8 ? std::array<int, 3>{{r + dr[j], c + dc[j], k}}
                           : std::array<int, 3>{{r, c, (k + (j == 8 ? 1 : n_yaw - 1)) % n_yaw}});
      }
  CHECK(ba.size() == n_blocked);
  size_t mism2 = 0;
  if (!ba.empty()) {
    const std::vector<double> same_set = planner->blockCostFieldMoves(second, ba, bb);
    mism2 = differing(same_set, now);
  } else {
    mism2 = differing(first, now);
  }
  CHECK(mism2 == 0);
  artp_field_destroy(second);
  artp_field_destroy(field);

  std::printf("cost field plan: %zu of 8 targets solved in %llu rounds, %llu moves checked, %llu blocked, %zu states, "
              "%zu + %zu mismatches\n", solved, (unsigned long long)ps.rounds, (unsigned long long)ps.moves_checked,
              (unsigned long long)ps.moves_blocked, states, mism1, mism2);
  return fails ? 1 : 0;
}
