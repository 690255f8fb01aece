// The ob::Planner-shaped front of the batched tree planners: what Planner::Planner sets as ss_'s planner for
// "rrt_star", "inf_rrt_star" and "rrt_sharp" (the reference: og::RRTstar / og::InformedRRTstar / og::RRTsharp,
// planner.cpp:92-105), over BatchTree (artp_tree_* of the C ABI).  solve() builds a fresh tree for the problem
// definition's start and goal and grows it for params.planner.plan_time, like Planner::plan does.  Needs OMPL's
// planning layer: compiled with -DARTP_HAVE_OMPL only (tests/fake_include in this image).
#pragma once

#ifndef ARTP_HAVE_OMPL
#error "the ob::Planner shells need OMPL (or the scaffold under tests/fake_include): build with -DARTP_HAVE_OMPL"
#endif

#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include <ompl/base/Planner.h>
#include <ompl/base/PlannerStatus.h>
#include <ompl/base/PlannerTerminationCondition.h>
#include <ompl/base/ProblemDefinition.h>
#include <ompl/base/goals/GoalSampleableRegion.h>
#include <ompl/geometric/PathGeometric.h>

#include "art_planner/planners/batch_tree.h"
#include "art_planner/validity_checker/validity_checker.h"

namespace og = ompl::geometric;

namespace art_planner {

class BatchTreePlanner : public ob::Planner {
 public:
  // name: the planner name of params.planner.name ("rrt_star", "inf_rrt_star", "rrt_sharp")
  BatchTreePlanner(const ob::SpaceInformationPtr& si, const std::string& name) : ob::Planner(si, name) {}

  // the BatchTree Planner::plan() drives: the shell and the facade grow the same kind of tree
  void bindTree(const std::shared_ptr<BatchTree>& tree, const ParamsConstPtr& params) {
    tree_ = tree;
    params_ = params;
  }

  void clear() override {
    ob::Planner::clear();
    std::lock_guard<std::mutex> lock(mutex_);
    if (tree_) tree_->clear();
  }
  void setup() override { ob::Planner::setup(); }

  ob::PlannerStatus solve(const ob::PlannerTerminationCondition& ptc) override {
    std::lock_guard<std::mutex> lock(mutex_);
    if (!tree_ || !pdef_) return ob::PlannerStatus::ABORT;
    if (pdef_->getStartStateCount() == 0) return ob::PlannerStatus::INVALID_START;
    const ob::GoalPtr goal = pdef_->getGoal();
    if (!goal) return ob::PlannerStatus::INVALID_GOAL;
    BatchTree::StateArray s, g;
    flattenSE3(pdef_->getStartState(0), s.data());
    {
      ob::State* gs = si_->allocState();
      goal->as<ob::GoalSampleableRegion>()->sampleGoal(gs);
      flattenSE3(gs, g.data());
      si_->freeState(gs);
    }
    if (ptc()) return ob::PlannerStatus::TIMEOUT;
    std::vector<BatchTree::StateArray> flat;
    double cost = 0.0;
    bool solved = false;
    try {
      solved = tree_->plan(s, g, params_ ? params_->planner.plan_time : 0.0, &flat, &cost);
    } catch (const std::exception&) {   // start or goal rejected by the device
      return ob::PlannerStatus::ABORT;
    }
    if (!solved) return ob::PlannerStatus::TIMEOUT;
    auto path = std::make_shared<og::PathGeometric>(si_);
    ob::State* st = si_->allocState();
    for (const BatchTree::StateArray& f : flat) {
      unflattenSE3(f.data(), st);
      path->append(st);
    }
    si_->freeState(st);
    pdef_->addSolutionPath(path, false, 0.0, getName());
    last_cost_ = cost;
    return ob::PlannerStatus::EXACT_SOLUTION;
  }
  double lastSolutionCost() const { return last_cost_; }

 private:
  std::shared_ptr<BatchTree> tree_;
  ParamsConstPtr params_;
  double last_cost_{0.0};
  mutable std::mutex mutex_;
};

}  // namespace art_planner
