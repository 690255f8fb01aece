// art_planner::BatchTree -- the batched counterpart of the reference's tree planners (OMPL's RRTstar, InformedRRTstar,
// RRTsharp, selected by params.planner.name in Planner::Planner, art_planner/src/planner.cpp:92-105), each batch of
// samples as one device batch per stage on the MI355X (include/artp_c.h: artp_tree_*).  Like the reference, which
// clears its planner before every solve, plan() builds a FRESH tree per call and grows it for the planning time.
// Objective: PathLengthObjective (objectives.custom_path_length.*) -- the reference's getObjective (planner.cpp:27-35)
// never gives the tree planners the learned cost.
#pragma once

#include <array>
#include <cstdint>
#include <string>
#include <vector>

#include "art_planner/gpu_context.h"
#include "art_planner/params.h"

namespace art_planner {

class BatchTree {
 public:
  using StateArray = std::array<double, 7>;  // x y z qx qy qz qw (OMPL SE3 state, flattened)

  // artp_tree_params::variant of a planner name; -1 when the name is not a tree planner
  static int variantOf(const std::string& name) {
    if (name == "rrt_star") return 0;
    if (name == "inf_rrt_star") return 1;
    if (name == "rrt_sharp") return 2;
    return -1;
  }

  BatchTree(const ParamsConstPtr& params, const GpuContextPtr& gpu, int variant)
      : params_(params), gpu_(gpu), variant_(variant) {}
  ~BatchTree() { clear(); }
  BatchTree(const BatchTree&) = delete;
  BatchTree& operator=(const BatchTree&) = delete;

  void setSeed(uint64_t seed) { seed_ = seed; }
  // samples per batch (artp_tree_params::batch, default 1024)
  void setBatch(uint32_t batch) { batch_ = batch; }
  void clear() {
    if (tree_) artp_tree_destroy(tree_);
    tree_ = nullptr;
  }

  // A fresh tree from s to g grown for plan_time seconds (at least one batch).  Returns true with the root -> goal
  // chain and its cost when the goal became a vertex.  Throws on an invalid start or goal.
  bool plan(const StateArray& s, const StateArray& g, double plan_time, std::vector<StateArray>* path, double* cost) {
    clear();
    artp_tree_params p;
    artp_tree_params_defaults(&p);
    p.seed = seed_;
    p.variant = variant_;
    p.objective = params_->objectives.custom_path_length.use_directional_cost ? 1 : 0;
    p.max_lon_vel = params_->objectives.custom_path_length.max_lon_vel;
    p.max_lat_vel = params_->objectives.custom_path_length.max_lat_vel;
    p.max_ang_vel = params_->objectives.custom_path_length.max_ang_vel;
    p.batch = batch_;
    p.plan_time = plan_time > 0.0 ? plan_time : 0.0;
    throwOnError(gpu_->get(), artp_tree_create(gpu_->get(), &p, s.data(), g.data(), &tree_), "artp_tree_create");
    throwOnError(gpu_->get(), artp_tree_grow(tree_, p.plan_time > 0.0 ? 0 : 1, nullptr), "artp_tree_grow");
    size_t n = 0;
    double c = 0.0;
    throwOnError(gpu_->get(), artp_tree_solve(tree_, nullptr, 0, &n, &c), "artp_tree_solve");
    if (n == 0) return false;
    path->assign(n, StateArray{});
    throwOnError(gpu_->get(), artp_tree_solve(tree_, (*path)[0].data(), n, &n, &c), "artp_tree_solve");
    if (cost) *cost = c;
    return true;
  }

  // Planner::getSolutionPath(true): the roadmap's all-pairs shortcut search (artp_tree_simplify_path)
  void simplify(std::vector<StateArray>* path, double* cost = nullptr) {
    if (!tree_ || path->empty()) return;
    std::vector<StateArray> out(path->size());
    size_t n = 0;
    double c = 0.0;
    throwOnError(gpu_->get(), artp_tree_simplify_path(tree_, (*path)[0].data(), path->size(), out[0].data(), &n, &c),
                 "artp_tree_simplify_path");
    out.resize(n);
    path->swap(out);
    if (cost) *cost = c;
  }

  // artp_tree_stats of the last plan() (zeros before the first)
  std::array<uint64_t, 8> stats() const {
    std::array<uint64_t, 8> out{};
    if (tree_) throwOnError(gpu_->get(), artp_tree_stats(tree_, out.data()), "artp_tree_stats");
    return out;
  }

 private:
  ParamsConstPtr params_;
  GpuContextPtr gpu_;
  int variant_;
  uint64_t seed_{42};
  uint32_t batch_{1024};
  artp_tree* tree_{nullptr};
};

}  // namespace art_planner
