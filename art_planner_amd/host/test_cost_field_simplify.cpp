// Exercises Planner::simplifyCostFieldPaths and planOnCostField(simplify = true) (artp_field_simplify_paths) through the
// host mirror on the map of test_cost_field.cpp: 90 x 70 cells at 0.1 m, flat ground with a raised block and a trench, the
// mask from Planner::computeReachability.  A reverse field from one goal is computed and kept, and planOnCostField gives
// checked lattice paths to eight targets.
//   1. the paths simplified with window 0 (all pairs) and with a window that covers the longest: both must equal, bit for
//      bit -- states, count and cost --, artp_roadmap_simplify_path on a roadmap of the same objective and velocities,
//      one path at a time.
//   2. window 16: the kept indices ascend from 0 to n - 1 in steps of at most 16, every pair of neighbouring kept states
//      passes artp_check_motions and artp_check_edges_interp, and the cost is at most the one of window 1, which keeps
//      every state; planOnCostField(simplify = true, window 16) on a second field holds the same bits.
//   test_cost_field_simplify
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

typedef std::vector<std::array<double, 7>> States;

static bool same_states(const States& a, const States& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (std::memcmp(a[i].data(), b[i].data(), 7 * sizeof(double)) != 0) return false;
  return true;
}

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

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
  std::array<int, 3> goal{{-1, -1, 0}};
  for (int r = 60; r < 80 && goal[0] < 0; ++r)
    for (int c = 8; c < 16; ++c)
      if (mask[r + static_cast<size_t>(c) * rows] == (1u << n_yaw) - 1u) {
        goal = {{r, c, 0}};
        break;
      }
  CHECK(goal[0] >= 0);
  if (goal[0] < 0) return 1;
  artp_field *field = nullptr, *second = nullptr;
  const std::vector<double> first = planner->computeCostField(mask, n_yaw, {goal}, true, &field);
  planner->computeCostField(mask, n_yaw, {goal}, true, &second);
  CHECK(field != nullptr && second != nullptr);
  if (!field || !second) return 1;
  std::vector<std::array<int, 3>> targets;
  for (int r = 5; r < rows && targets.size() < 8; r += 11)
    for (int c = 62; c > 4 && targets.size() < 8; c -= 19)
      if (std::isfinite(first[(r + static_cast<size_t>(c) * rows) * n_yaw + 2])) targets.push_back({{r, c, 2}});
  CHECK(targets.size() == 8);
  const std::vector<Planner::CostFieldPlan> plans = planner->planOnCostField(field, targets);
  std::vector<States> paths;
  size_t longest = 0;
  for (const auto& p : plans) {
    CHECK(p.simplified.empty() && std::isinf(p.simplified_cost));       // not asked for
    if (p.status == 0) {
      paths.push_back(p.states);
      longest = std::max(longest, p.states.size());
    }
  }
  CHECK(paths.size() >= 4 && longest >= 10);
  if (paths.empty()) return 1;

  // 1. a window that covers the paths: the roadmap's simplifier
  artp_field_simplify_stats_t ss{};
  const std::vector<Planner::SimplifiedPath> all_pairs = planner->simplifyCostFieldPaths(field, paths, 0, &ss);
  const std::vector<Planner::SimplifiedPath> covering = planner->simplifyCostFieldPaths(field, paths, (unsigned)longest);
  CHECK(all_pairs.size() == paths.size() && covering.size() == paths.size() && ss.paths == paths.size() && ss.batches >= 1);
  const auto& cpl = params->objectives.custom_path_length;
  size_t mism1 = 0, states_in = 0, states_out = 0;
  for (size_t q = 0; q < paths.size(); ++q) {
    artp_roadmap_params rp;
    artp_roadmap_params_defaults(&rp);
    rp.n_milestones = 8;
    rp.objective = 1;
    rp.max_lon_vel = cpl.max_lon_vel;
    rp.max_lat_vel = cpl.max_lat_vel;
    rp.max_ang_vel = cpl.max_ang_vel;
    artp_roadmap* rm = nullptr;
    CHECK(artp_roadmap_build(planner->gpu()->get(), &rp, paths[q].front().data(), paths[q].back().data(), &rm) == ARTP_OK);
    if (!rm) return 1;
    States want(paths[q].size());
    size_t n_out = 0;
    double cost = 0.0;
    CHECK(artp_roadmap_simplify_path(rm, paths[q][0].data(), paths[q].size(), want[0].data(), &n_out, &cost) == ARTP_OK);
    artp_roadmap_destroy(rm);
    want.resize(n_out);
    for (const auto* got : {&all_pairs[q], &covering[q]})
      mism1 += !(got->status == 0 && same_states(got->states, want) && same_bits(got->cost, cost) &&
                 got->kept.size() == n_out);
    states_in += paths[q].size();
    states_out += n_out;
  }
  CHECK(mism1 == 0);
  CHECK(states_out < states_in);

  // 2. window 16 on its own terms, and through planOnCostField
  const std::vector<Planner::SimplifiedPath> w16 = planner->simplifyCostFieldPaths(field, paths, 16);
  const std::vector<Planner::SimplifiedPath> w1 = planner->simplifyCostFieldPaths(field, paths, 1);
  size_t bad_pairs = 0;
  for (size_t q = 0; q < paths.size(); ++q) {
    const Planner::SimplifiedPath& s = w16[q];
    CHECK(s.status == 0 && !s.kept.empty() && s.kept.front() == 0 && s.kept.back() == paths[q].size() - 1);
    CHECK(w1[q].status == 0 && w1[q].kept.size() == paths[q].size() && s.cost <= w1[q].cost && std::isfinite(w1[q].cost));
    for (size_t i = 0; i + 1 < s.kept.size(); ++i) CHECK(s.kept[i] < s.kept[i + 1] && s.kept[i + 1] - s.kept[i] <= 16);
    for (size_t i = 0; i < s.kept.size(); ++i)
      CHECK(std::memcmp(s.states[i].data(), paths[q][s.kept[i]].data(), 7 * sizeof(double)) == 0);
    if (s.states.size() > 1) {
      std::vector<uint8_t> ok(s.states.size() - 1), ok2(ok.size());
      std::vector<uint32_t> ni(ok.size());
      CHECK(artp_check_motions(planner->gpu()->get(), s.states[0].data(), s.states[1].data(), ok.size(), ok.data()) == ARTP_OK);
      CHECK(artp_check_edges_interp(planner->gpu()->get(), s.states[0].data(), s.states[1].data(), ok.size(), ok2.data(),
                                    ni.data()) == ARTP_OK);
      for (size_t i = 0; i < ok.size(); ++i) bad_pairs += !ok[i] || !ok2[i];
    }
  }
  CHECK(bad_pairs == 0);
  const std::vector<Planner::CostFieldPlan> both = planner->planOnCostField(second, targets, 64, nullptr, true, 16);
  size_t mism2 = 0, at = 0;
  CHECK(both.size() == plans.size());
  for (size_t i = 0; i < both.size() && i < plans.size(); ++i) {
    mism2 += !(both[i].status == plans[i].status && same_states(both[i].states, plans[i].states) &&
               same_bits(both[i].cost, plans[i].cost));
    if (plans[i].status == 0) {
      mism2 += !(same_states(both[i].simplified, w16[at].states) && same_bits(both[i].simplified_cost, w16[at].cost));
      ++at;
    } else {
      mism2 += !both[i].simplified.empty();
    }
  }
  CHECK(mism2 == 0);
  artp_field_destroy(second);
  artp_field_destroy(field);

  std::printf("cost field simplify: %zu paths, %zu states in, %zu kept with all pairs (%llu candidates, %llu usable), "
              "%zu + %zu mismatches\n", paths.size(), states_in, states_out, (unsigned long long)ss.candidates,
              (unsigned long long)ss.usable_candidates, mism1, mism2);
  return fails ? 1 : 0;
}
