// Exercises BatchPRM::solveMany (artp_roadmap_solve_many) through the host mirror on a flat map built here:
// 100 x 100 cells at 0.1 m, start (-4, -4, yaw 0), a ring of goals, one goal off the map.  Every goal's status and cost
// must equal setQuery(start, goal) + solve() on the same roadmap afterwards, and every path must run from the start
// to its goal.
//   test_roadmap_many
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

static void toState(const double* s, Planner::StateType* st) {
  st->setXYZ(s[0], s[1], s[2]);
  st->rotation().x = s[3];
  st->rotation().y = s[4];
  st->rotation().z = s[5];
  st->rotation().w = s[6];
}

int main() {
  const int rows = 100, cols = 100;
  const double res = 0.1;
  std::vector<float> elev(static_cast<size_t>(rows) * cols, 0.0f), trav(elev.size(), 1.0f);
  auto params = std::make_shared<Params>();
  // shipped YAML robot (art_planner_ros/config/params.yaml:55-71)
  params->robot.torso.length = 1.31; params->robot.torso.width = 0.65; params->robot.torso.height = 0.3;
  params->robot.torso.offset.z = 0.04;
  params->robot.feet.offset.x = 0.51; params->robot.feet.offset.y = 0.2; params->robot.feet.offset.z = -0.475;
  params->robot.feet.reach.x = 0.2; params->robot.feet.reach.y = 0.2; params->robot.feet.reach.z = 0.2;
  params->planner.prm_motion_cost.max_n_vertices = 2000;
  params->planner.plan_time = 0.02;
  std::unique_ptr<Planner> planner;
  try {
    planner.reset(new Planner(params, 0));
  } catch (const std::exception& e) {
    std::printf("no GPU context: %s\n", e.what());
    return 3;
  }
  std::unique_ptr<Map> m(new Map);
  m->setGeometry(Map::Geometry{rows, cols, res, rows * res, cols * res, 0.0, 0.0});
  m->addLayer("elevation", elev.data());
  m->addLayer("traversability", trav.data());
  planner->setMap(std::move(m));
  const double s[7] = {-4.0, -4.0, 0.0, 0.0, 0.0, 0.0, 1.0};
  const double g0[7] = {4.0, 4.0, 0.0, 0.0, 0.0, 0.0, 1.0};
  Planner::StateType start, goal;
  toState(s, &start);
  toState(g0, &goal);
  CHECK(planner->plan(start, goal) == PlannerStatus::SOLVED);
  const auto prm = planner->roadmap();
  CHECK(prm != nullptr && prm->numVertices() > 2);
  if (!prm || prm->numVertices() <= 2) return 1;
  // goals: a ring around the middle of the map, a state right next to the start (a near goal), one off the map
  std::vector<BatchPRM::StateArray> goals;
  for (int i = 0; i < 16; ++i) {
    const double a = 2.0 * M_PI * i / 16.0, yaw = a / 2.0;
    goals.push_back({3.0 * std::cos(a), 3.0 * std::sin(a), 0.0, 0.0, 0.0, std::sin(yaw / 2), std::cos(yaw / 2)});
  }
  goals.push_back({-3.95, -4.0, 0.0, 0.0, 0.0, 0.0, 1.0});
  goals.push_back({40.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0});
  const BatchPRM::StateArray sa = BatchPRM::flatten(start);
  std::vector<int32_t> status;
  std::vector<double> cost;
  std::vector<std::vector<BatchPRM::StateArray>> paths;
  const size_t fallback = prm->solveMany(sa, goals, &status, &cost, &paths);
  CHECK(status.size() == goals.size() && cost.size() == goals.size() && paths.size() == goals.size());
  CHECK(fallback >= 1);
  CHECK(status.back() == ARTP_GOAL_INVALID && std::isinf(cost.back()) && paths.back().empty());
  size_t solved = 0;
  for (size_t i = 0; i + 1 < goals.size(); ++i) {
    solved += status[i] == ARTP_GOAL_SOLVED;
    if (status[i] != ARTP_GOAL_SOLVED) continue;
    CHECK(paths[i].size() >= 2);
    CHECK(paths[i].front() == sa && paths[i].back() == goals[i]);
  }
  CHECK(solved >= goals.size() - 2);
  // the same answers one query at a time
  for (size_t i = 0; i < goals.size(); ++i) {
    int32_t st = ARTP_GOAL_SOLVED;
    double c = INFINITY;
    try {
      prm->setQuery(sa, goals[i]);
    } catch (const std::exception&) {
      st = ARTP_GOAL_INVALID;
    }
    if (st == ARTP_GOAL_SOLVED) {
      std::vector<BatchPRM::StateArray> p;
      if (!prm->solve(&p, &c)) st = ARTP_GOAL_UNREACHABLE;
    }
    CHECK(st == status[i]);
    if (st == ARTP_GOAL_SOLVED) CHECK(std::fabs(c - cost[i]) <= 1e-12 * c);
  }
  std::printf("solveMany: %zu goals, %zu solved, %zu through the fallback, all equal to the sequential queries\n",
              goals.size(), solved, fallback);
  if (fails) std::printf("%d check(s) failed\n", fails);
  return fails ? 1 : 0;
}
