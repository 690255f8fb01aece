// Exercises Planner::computeClearance and computeClearanceCostField (artp_clearance_map, artp_field_compute_clearance)
// through the host mirror on the map of test_cost_field.cpp: 90 x 70 cells at 0.1 m, flat ground with a raised block and a
// trench, the mask from Planner::computeReachability at 8 headings.
//   1. the facade's d2 (radius 5, yaw_spread 1) equals a brute-force loop over the definition, written here
//   2. a clearance field with gain 0 equals computeCostField's field bit for bit
//   3. planOnCostField on a kept clearance field (margin 0.3 m, gain 2) to eight targets: every move of every returned
//      path passes artp_check_motions; a blocked move and unblockCostField work on the kept field; updateCostField is
//      refused
//   test_cost_field_clearance
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

  const std::vector<uint32_t> mask = planner->computeReachability(n_yaw);
  const size_t cells = static_cast<size_t>(rows) * cols;
  CHECK(mask.size() == cells);
  if (mask.size() != cells) return 1;

  // 1. d2 against the definition
  const int R = 5, spread = 1;
  const std::vector<uint16_t> d2 = planner->computeClearance(mask, n_yaw, R, spread, false);
  CHECK(d2.size() == cells * n_yaw);
  if (d2.size() != cells * n_yaw) return 1;
  size_t mism_d2 = 0, finite_d2 = 0;
  for (int c = 0; c < cols; ++c)
    for (int r = 0; r < rows; ++r)
      for (int k = 0; k < n_yaw; ++k) {
        unsigned want = 0;
        if ((mask[r + static_cast<size_t>(c) * rows] >> k) & 1u) {
          want = 0xffffu;
          for (int dc = -R; dc <= R; ++dc)
            for (int dr = -R; dr <= R; ++dr) {
              const int rr = r + dr, cc = c + dc;
              const unsigned dd = static_cast<unsigned>(dr * dr + dc * dc);
              if (dd > static_cast<unsigned>(R * R) || dd >= want || rr < 0 || rr >= rows || cc < 0 || cc >= cols) continue;
              const uint32_t w = mask[rr + static_cast<size_t>(cc) * rows];
              bool obstacle = false;
              for (int t = -spread; t <= spread; ++t) obstacle |= !((w >> ((k + t + n_yaw) % n_yaw)) & 1u);
              if (obstacle) want = dd;
            }
        }
        const unsigned got = d2[(r + static_cast<size_t>(c) * rows) * n_yaw + k];
        mism_d2 += got != want;
        finite_d2 += got != 0 && got != 0xffffu;
      }
  CHECK(mism_d2 == 0 && finite_d2 > 1000);
  bool threw = false;
  try {
    planner->computeClearance(mask, n_yaw, 33);
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);

  // 2. gain 0 is the plain field
  std::array<int, 3> goal{{-1, -1, 0}};
  for (int r = 60; r < 80 && goal[0] < 0; ++r)
    for (int c = 8; c < 16; ++c)
      if (mask[r + static_cast<size_t>(c) * rows] == (1u << n_yaw) - 1u) {
        goal = {{r, c, 0}};
        break;
      }
  CHECK(goal[0] >= 0);
  if (goal[0] < 0) return 1;
  const std::vector<double> plain = planner->computeCostField(mask, n_yaw, {goal}, true);
  const std::vector<double> gain0 = planner->computeClearanceCostField(mask, n_yaw, {goal}, 0.3, 0.0, R, spread, false, true);
  const size_t mism_gain0 = differing(plain, gain0);
  CHECK(plain.size() == cells * n_yaw && mism_gain0 == 0);

  // 3. a kept clearance field: plan, block, unblock
  artp_field* field = nullptr;
  const std::vector<double> first = planner->computeClearanceCostField(mask, n_yaw, {goal}, 0.3, 2.0, R, spread, false, true, &field);
  CHECK(first.size() == cells * n_yaw && field != nullptr);
  if (first.size() != cells * n_yaw || !field) return 1;
  size_t raised = 0;
  for (size_t i = 0; i < first.size(); ++i) {
    CHECK(std::isfinite(first[i]) == std::isfinite(plain[i]));
    CHECK(!(first[i] < plain[i]));                                   // a factor >= 1 only raises distances
    raised += first[i] > plain[i];
  }
  CHECK(raised > 0);
  std::vector<uint16_t> own(cells * n_yaw);
  CHECK(artp_field_clearance(field, own.data()) == ARTP_OK && own == d2);
  threw = false;
  try {
    planner->updateCostField(field, mask);
  } catch (const std::exception&) {
    threw = true;
  }
  CHECK(threw);
  std::vector<std::array<int, 3>> targets;
  for (int r = 5; r < rows && targets.size() < 8; r += 11)
    for (int c = 62; c > 4 && targets.size() < 8; c -= 19)
      if (std::isfinite(first[(r + static_cast<size_t>(c) * rows) * n_yaw + 2])) targets.push_back({{r, c, 2}});
  CHECK(targets.size() == 8);
  const std::vector<Planner::CostFieldPlan> plans = planner->planOnCostField(field, targets);
  artp_field_plan_stats_t ps;
  CHECK(artp_field_plan_stats(field, &ps) == ARTP_OK && ps.rounds >= 1);
  size_t solved = 0, bad_moves = 0, moves = 0;
  for (size_t i = 0; i < plans.size(); ++i) {
    const Planner::CostFieldPlan& p = plans[i];
    CHECK(p.status == 0 || p.status == 1);
    if (p.status != 0) continue;
    ++solved;
    CHECK(p.nodes.size() == p.states.size() && !p.nodes.empty());
    CHECK(p.nodes.front() == targets[i] && p.nodes.back() == goal);     // a reverse field: travel order
    if (p.states.size() > 1) {
      std::vector<uint8_t> ok(p.states.size() - 1);
      CHECK(artp_check_motions(planner->gpu()->get(), p.states[0].data(), p.states[1].data(), ok.size(), ok.data()) == ARTP_OK);
      for (uint8_t v : ok) bad_moves += !v;
      moves += ok.size();
    }
  }
  CHECK(solved > 0 && moves > 0 && bad_moves == 0);
  uint64_t cleared = 0;
  const std::vector<double> lifted = planner->unblockCostField(field, nullptr, &cleared);
  CHECK(cleared == ps.moves_blocked && differing(lifted, first) == 0);
  if (!plans.empty() && plans[0].status == 0 && plans[0].nodes.size() > 2) {
    uint64_t newly = 0;
    const std::vector<double> cut = planner->blockCostFieldMoves(field, {plans[0].nodes[0]}, {plans[0].nodes[1]}, &newly);
    CHECK(newly == 1);
    for (size_t i = 0; i < cut.size(); ++i) CHECK(!(cut[i] < first[i]));
  }
  artp_field_destroy(field);

  std::printf("cost field clearance: %zu nodes with a finite clearance, %zu of 8 targets solved in %llu rounds, %zu moves "
              "checked on the paths, %llu blocked; %zu mismatches\n", finite_d2, solved, (unsigned long long)ps.rounds, moves,
              (unsigned long long)ps.moves_blocked, mism_d2 + mism_gain0 + bad_moves);
  return fails ? 1 : 0;
}
