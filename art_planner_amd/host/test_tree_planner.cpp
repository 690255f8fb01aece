// Exercises art_planner::Planner with the tree planner names (params.planner.name = "rrt_star", "inf_rrt_star",
// "rrt_sharp"; the reference's og::RRTstar / InformedRRTstar / RRTsharp) on a flat map built here:
// 100 x 100 cells at 0.1 m, (-4, -4, yaw 0) -> (4, 4).  For every name plan() returns SOLVED, the path runs from the
// start to the goal, its cost is no less than the straight line, and the simplified path is no costlier.
//   test_tree_planner
// Exit code 0 = every check holds; 3 = no GPU (the constructor throws: no CPU fallback).
#include <cmath>
#include <cstdio>
#include <memory>
#include <string>
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

// PathLengthObjective::motionCost of the Euclidean objective (path_length_objective.cpp:26-70)
static double pathCost(const Planner::Path& p, double v) {
  double c = 0.0;
  for (size_t i = 1; i < p.size(); ++i)
    c += std::sqrt(std::pow(p[i][0] - p[i - 1][0], 2) + std::pow(p[i][1] - p[i - 1][1], 2) +
                   std::pow(p[i][2] - p[i - 1][2], 2)) / v;
  return c;
}

int main() {
  const int rows = 100, cols = 100;
  const double res = 0.1;
  std::vector<float> elev(static_cast<size_t>(rows) * cols, 0.0f), trav(elev.size(), 1.0f);
  const double s[7] = {-4.0, -4.0, 0.0, 0.0, 0.0, 0.0, 1.0};
  const double g[7] = {4.0, 4.0, 0.0, 0.0, 0.0, 0.0, 1.0};
  for (const char* name : {"rrt_star", "inf_rrt_star", "rrt_sharp"}) {
    auto params = std::make_shared<Params>();
    // shipped YAML robot (art_planner_ros/config/params.yaml:55-71)
    params->robot.torso.length = 1.31; params->robot.torso.width = 0.65; params->robot.torso.height = 0.3;
    params->robot.torso.offset.z = 0.04;
    params->robot.feet.offset.x = 0.51; params->robot.feet.offset.y = 0.2; params->robot.feet.offset.z = -0.475;
    params->robot.feet.reach.x = 0.2; params->robot.feet.reach.y = 0.2; params->robot.feet.reach.z = 0.2;
    params->planner.name = name;
    params->planner.plan_time = 0.05;
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
    CHECK(planner->hasMap());
    Planner::StateType start, goal;
    toState(s, &start);
    toState(g, &goal);
    const PlannerStatus st = planner->plan(start, goal);
    CHECK(st == PlannerStatus::SOLVED);
    if (st != PlannerStatus::SOLVED) continue;
    CHECK(planner->tree() != nullptr);
    const Planner::Path path = planner->getSolutionPathFlat(false);
    const Planner::Path simple = planner->getSolutionPathFlat(true);
    const double cost = planner->getSolutionCost();
    const double straight = std::hypot(g[0] - s[0], g[1] - s[1]) / params->objectives.custom_path_length.max_lon_vel;
    CHECK(path.size() >= 2 && simple.size() >= 2);
    for (const auto* p : {&path, &simple}) {
      CHECK(std::hypot((*p)[0][0] - s[0], (*p)[0][1] - s[1]) < 1e-9);
      CHECK(std::hypot(p->back()[0] - g[0], p->back()[1] - g[1]) <= 0.3 + 1e-9);
    }
    const double c_path = pathCost(path, params->objectives.custom_path_length.max_lon_vel);
    const double c_simple = pathCost(simple, params->objectives.custom_path_length.max_lon_vel);
    CHECK(std::fabs(c_path - cost) <= 1e-9 * cost);
    CHECK(cost >= straight * (1 - 1e-12));
    CHECK(c_simple <= c_path * (1 + 1e-9));
    const auto stats = planner->tree()->stats();
    std::printf("%s: SOLVED, %zu states, cost %.4f (straight line %.4f), simplified %zu states %.4f, %llu vertices, "
                "%llu batches\n", name, path.size(), cost, straight, simple.size(), c_simple,
                (unsigned long long)stats[0], (unsigned long long)stats[1]);
  }
  if (fails) std::printf("%d check(s) failed\n", fails);
  return fails ? 1 : 0;
}
