// art_planner::Planner with the reference's public surface (art_planner/include/art_planner/planner.h:31-71;
// art_planner/src/planner.cpp:75-330), every step routed to the MI355X through the C ABI:
//   setMap  -> the processor chain + CDF on the device (artp_preprocess_map_ex), installed as both height
//              fields + sampler layers + z bounds (artp_preprocessed_install); a kept roadmap follows the new map:
//              invalidated milestones dropped and replenished (artp_roadmap_grow; the upkeep of
//              PRMMotionCostMaintainer / LazyPRMStarMinUpdate, lazy_prm_star_min_update.cpp:18-217)
//   plan    -> goal clipped to the bounds and dropped onto the map (planner.cpp:204-238), start / goal
//              region search as ONE validity batch each (start.cpp:9-47, goal.cpp:11-45), then the batched PRM
//   getSolutionPath(simplify) -> the cheaper of original and simplified path (planner.cpp:266-330)
// OMPL's SimpleSetup / ScopedState / PathGeometric are not in this image: states are SE3StateSpace::StateType
// (ompl_min.h, or the real one with -DARTP_HAVE_OMPL) and a path is a vector of flattened SE3 states.
// grid_map is not in this image either: setMap takes the Map wrapper (map/map.h).  Inpainting stays with the
// caller (include/artp_c.h, N2): the elevation layer must be hole-free, "observed" marks the cells that were.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <iostream>
#include <limits>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <vector>

#include "art_planner/gpu_context.h"
#include "art_planner/map/map.h"
#include "art_planner/ompl_min.h"
#include "art_planner/params.h"
#include "art_planner/planner_status.h"
#include "art_planner/planners/batch_prm.h"
#include "art_planner/planners/batch_tree.h"

// With BOTH real libraries available the class also carries the reference's EXACT public signatures and the protected
// members a subclass like PlannerRos reaches into (planner.h:41-70, planner_ros.h:24):
//   setMap(std::unique_ptr<grid_map::GridMap>&&), plan(const ob::ScopedState<>&, const ob::ScopedState<>&),
//   og::PathGeometric getSolutionPath(const bool&) const; ss_, space_, checker_, sampler_allocator_ (+ params_, map_,
//   map_mutex_, solved_, which exist in every build).  tests/test_host_mirror.py compiles a PlannerRos-shaped subclass
//   against tests/fake_include (neither library is installed in this image).
#if defined(ARTP_HAVE_OMPL) && defined(ARTP_HAVE_GRID_MAP)
#define ARTP_PLANNER_REFERENCE_SURFACE 1
#include <functional>
#include <grid_map_core/GridMap.hpp>
#include <ompl/base/ScopedState.h>
#include <ompl/geometric/PathGeometric.h>
#include <ompl/geometric/SimpleSetup.h>
#include "art_planner/planners/batch_tree_planner.h"
#include "art_planner/planners/lazy_prm_star_min_update.h"
#include "art_planner/planners/prm_motion_cost.h"
#include "art_planner/sampler.h"
#include "art_planner/validity_checker/validity_checker.h"
namespace og = ompl::geometric;
#endif

namespace ob = ompl::base;

namespace art_planner {

// OMPL states cannot be copied (ob::State's copy constructor is deleted; the real SE3 state is a compound of
// separately allocated parts): the planner works on flattened states x y z qx qy qz qw and only READS the caller's.
// utils.h:85-88 on a flattened state
inline double yawOfFlat(const double* s) {
  return std::atan2(2 * (s[6] * s[5] + s[3] * s[4]), 1 - 2 * (s[4] * s[4] + s[5] * s[5]));
}

// utils.h:101-115 (setSO3FromRPY) into a flattened state
inline void setFlatRotationFromRPY(double* s, const double* rpy) {
  const double r2 = rpy[0] * 0.5, p2 = rpy[1] * 0.5, y2 = rpy[2] * 0.5;
  const double cr = std::cos(r2), cp = std::cos(p2), cy = std::cos(y2);
  const double sr = std::sin(r2), sp = std::sin(p2), sy = std::sin(y2);
  s[6] = cy * cp * cr + sy * sp * sr;
  s[3] = cy * cp * sr - sy * sp * cr;
  s[4] = sy * cp * sr + cy * sp * cr;
  s[5] = sy * cp * cr - cy * sp * sr;
}

class Planner {
 public:
  using StateSpace = ob::SE3StateSpace;
  using StateType = typename StateSpace::StateType;
  using StateArray = BatchPRM::StateArray;
  using Path = std::vector<StateArray>;

#ifdef ARTP_PLANNER_REFERENCE_SURFACE
  // planner.cpp:75-131: the OMPL objects around the same GpuContext -- SimpleSetup on the SE3 space, the validity
  // checker, the batched motion validator (in place of OMPL's DiscreteMotionValidator) and the sampler allocator
  explicit Planner(const ParamsConstPtr& params = std::make_shared<const Params>(), int device = 0)
      : params_(params), gpu_(std::make_shared<GpuContext>(params, device)),
        prm_(std::make_shared<BatchPRM>(params, gpu_)), tree_(makeTree(params, gpu_)), sampler_allocator_(params, gpu_) {
    rb_->prm = prm_;
    rb_->params = params_;
    space_ = std::make_shared<StateSpace>();
    ss_ = std::make_shared<og::SimpleSetup>(space_);
    const ob::SpaceInformationPtr si = ss_->getSpaceInformation();
    // planner.cpp:90-117: the planner by name, set as ss_'s planner, its maintainer.  The PRM planners are the shells over
    // the batched roadmap (planners/*.h).  "lazy_prm_star" (the reference: OMPL's own og::LazyPRMstar, no maintainer,
    // :98-99) is SUBSTITUTED by the LazyPRMStarMinUpdate shell without a maintainer -- the same LazyPRM* graph and lazy
    // edge checks, no min-update upkeep.  The tree planners of the reference (rrt_star, inf_rrt_star, rrt_sharp: OMPL's
    // RRTstar / InformedRRTstar / RRTsharp) are the BatchTreePlanner shell over the batch-synchronous tree (artp_tree_*).
    ob::PlannerPtr planner;
    if (params_->planner.name == "lazy_prm_star_min_update" || params_->planner.name == "lazy_prm_star") {
      auto p = std::make_shared<LazyPRMStarMinUpdate>(si);
      p->bindRoadmap(rb_);
      // :110-115: the maintainer belongs to lazy_prm_star_min_update only.  It is handed the map pointer of this moment
      // (null until the first setMap, as in the reference) and only carries the parameters of the upkeep Planner::setMap runs.
      if (params_->planner.name == "lazy_prm_star_min_update")
        p->setMaintainer(std::unique_ptr<LazyPRMStarMinUpdateMaintainer>(new LazyPRMStarMinUpdateMaintainer(map_, params_)));
      planner = p;
    } else if (params_->planner.name == "prm_motion_cost") {
      auto p = std::make_shared<PRMMotionCost>(si);
      p->bindRoadmap(rb_);
      planner = p;
    } else if (tree_) {
      auto p = std::make_shared<BatchTreePlanner>(si, params_->planner.name);
      p->bindTree(tree_, params_);
      planner = p;
    } else {
      throw std::runtime_error("Unknown planner requested: " + params_->planner.name);
    }
    ss_->setPlanner(planner);
    checker_ = std::make_shared<StateValidityChecker>(si, params_, gpu_);
    ss_->setStateValidityChecker(checker_);
    motion_validator_ = std::make_shared<BatchMotionValidator>(si, gpu_);
    si->setMotionValidator(motion_validator_);
    space_->setStateSamplerAllocator(
        std::bind(&SE3FromSE2SamplerAllocator::getSampler, &sampler_allocator_, std::placeholders::_1));
  }
#else
  explicit Planner(const ParamsConstPtr& params = std::make_shared<const Params>(), int device = 0)
      : params_(params), gpu_(std::make_shared<GpuContext>(params, device)),
        prm_(std::make_shared<BatchPRM>(params, gpu_)), tree_(makeTree(params, gpu_)) {
    rb_->prm = prm_;
    rb_->params = params_;
  }
#endif
  ~Planner() {
    if (pre_) artp_preprocessed_destroy(pre_);
  }
  Planner(const Planner&) = delete;
  Planner& operator=(const Planner&) = delete;

  // planner.cpp:135-163.  Silently returns when the elevation layer is missing (:137-144).
  void setMap(std::unique_ptr<Map>&& map) {
    if (!map || !map->exists(params_->planner.elevation_layer)) {
      if (params_->verbose)
        std::cout << "Grid map does not have \"" << params_->planner.elevation_layer << "\" layer." << std::endl;
      return;
    }
    std::lock_guard<std::mutex> lock(map_mutex_);
    const auto g = map->getGeometry();
    const auto& elev = map->getLayer(params_->planner.elevation_layer);
    float lo = std::numeric_limits<float>::infinity(), hi = -lo;  // min/maxCoeffOfFinites
    for (const float h : elev) {
      if (std::isfinite(h)) {
        lo = h < lo ? h : lo;
        hi = h > hi ? h : hi;
      }
    }
    if (!(lo <= hi)) lo = hi = 0.0f;

    artp_preprocess_params pp;
    artp_preprocess_params_defaults(&pp);
    pp.traversability_thres = params_->planner.traversability_thres;
    pp.foothold_margin = params_->planner.safety.foothold_margin;
    pp.foothold_margin_max_hole_size = params_->planner.safety.foothold_margin_max_hole_size;
    pp.foothold_margin_max_drop = params_->planner.safety.foothold_margin_max_drop;
    pp.foothold_margin_max_drop_search_radius = params_->planner.safety.foothold_margin_max_drop_search_radius;
    pp.foothold_margin_min_step = params_->planner.safety.foothold_margin_min_step;
    pp.foothold_size = params_->planner.safety.foothold_size;
    // computeInverseSampleDensity (sample_density.cpp:12-43) counts the kept roadmap's vertices per cell
    std::vector<double> vertices;
    if (params_->sampler.use_inverse_vertex_density && rb_->built) vertices = prm_->vertices();
    pp.use_inverse_vertex_density = vertices.empty() ? 0 : 1;
    pp.use_max_prob_unknown_samples = params_->sampler.use_max_prob_unknown_samples ? 1 : 0;
    pp.max_prob_unknown_samples = params_->sampler.max_prob_unknown_samples;
    artp_preprocess_inputs in{};
    in.elevation = elev.data();
    in.traversability =
        map->exists(params_->planner.traversability_layer) ? map->getLayer(params_->planner.traversability_layer).data() : nullptr;
    in.observed = map->exists("observed") ? map->getLayer("observed").data() : nullptr;
    in.vertex_se3 = vertices.empty() ? nullptr : vertices.data();
    in.n_vertices = vertices.size() / 7;
    in.rows = g.rows;
    in.cols = g.cols;
    in.len_x = g.length_x;
    in.len_y = g.length_y;
    in.pos_x = g.position_x;
    in.pos_y = g.position_y;

    artp_preprocessed* fresh_raw = nullptr;
    throwOnError(gpu_->get(), artp_preprocess_map_ex(gpu_->get(), &in, &pp, &fresh_raw), "artp_preprocess_map_ex");
    // owned until it becomes pre_: nothing below may leak it by throwing
    std::unique_ptr<artp_preprocessed, void (*)(artp_preprocessed*)> fresh_guard(fresh_raw, artp_preprocessed_destroy);
    artp_preprocessed* fresh = fresh_raw;
    throwOnError(gpu_->get(), artp_preprocessed_install(gpu_->get(), fresh), "artp_preprocessed_install");
    // the install bumped artp_map_version(): labels cached on the previous map can no longer be served by any mirror
    // class on this context; drop them now rather than at their next lookup
    gpu_->mapChanged();
    // the normals of get3DPoseFrom2D (map.cpp:77-90) come back from the device once per map
    const size_t cells = static_cast<size_t>(g.rows) * g.cols;
    std::vector<float> n[3] = {std::vector<float>(cells), std::vector<float>(cells), std::vector<float>(cells)};
    const char* names[3] = {"normal_x", "normal_y", "normal_z"};
    for (int k = 0; k < 3; ++k)
      throwOnError(gpu_->get(), artp_preprocessed_get_layer(gpu_->get(), fresh, names[k], n[k].data()),
                   "artp_preprocessed_get_layer");
    for (int k = 0; k < 3; ++k) map->addLayer(names[k], n[k].data());
    // the roadmap's re-weighting (sampleGraph's reApplyPreprocessing) works on the new map's result from here on
    pp.use_inverse_vertex_density = params_->sampler.use_inverse_vertex_density ? 1 : 0;
    prm_->setDensityMap(fresh, pp);
    if (pre_) artp_preprocessed_destroy(pre_);
    pre_ = fresh_guard.release();
    map_ = std::move(map);
    // ob::RealVectorBounds of planner.cpp:146-156 (x / y: position -+ length, as the reference has it)
    low_[0] = g.position_x - g.length_x;
    high_[0] = g.position_x + g.length_x;
    low_[1] = g.position_y - g.length_y;
    high_[1] = g.position_y + g.length_y;
    low_[2] = lo - params_->robot.feet.reach.z / 2;
    high_[2] = hi + params_->robot.feet.reach.z / 2;
    if (rb_->built) {
      // the kept roadmap follows the map (PRMMotionCostMaintainer / LazyPRMStarMinUpdate upkeep): milestones the
      // new map invalidated are dropped and replaced by as many new samples; plan() then re-queries it
      try {
        const size_t dropped = prm_->grow(0);
        if (dropped) prm_->grow(dropped);
      } catch (const std::exception&) {  // the old start / goal are gone with the map (or the cost functor failed: the
        //                                    reference's setMap never prices anything): rebuild -- and report -- at the next plan
        prm_->clear();
        rb_->built = false;
      }
    }
    solved_ = false;
#ifdef ARTP_PLANNER_REFERENCE_SURFACE
    {  // planner.cpp:146-163: the state space's bounds, the checker's and the sampler's map
      ob::RealVectorBounds bounds(3);
      for (int a = 0; a < 3; ++a) {
        bounds.setLow(a, low_[a]);
        bounds.setHigh(a, high_[a]);
      }
      space_->setBounds(bounds);
      checker_->setMap(map_);
      checker_->heightFieldInstalled();   // both layers went to the device with artp_preprocessed_install above
      // OMPL quirk (VERDICT r4 missing-7): setBounds does not re-run StateSpace::setup(), and SimpleSetup::setup() skips
      // si_->setup() once it ran, so in the reference longestValidSegment_ -- and every checkMotion's segment count --
      // stays at the FIRST planned map's extents.  Default here: the resolution follows every map (what the bounds say);
      // setFreezeMotionResolution(true) reproduces the reference's behaviour.
      // The z bounds always follow the map (with a frozen extent they no longer enter the segment length); the frozen extent
      // is captured ONCE: here when no map had been installed at the time of setFreezeMotionResolution(true), or right
      // there when one had (a freeze after the first setMap used to freeze nothing).
      motion_validator_->setZBounds(low_[2], high_[2]);
      if (freeze_motion_resolution_ && !motion_resolution_set_) captureMotionResolution();
      sampler_allocator_.setMap(map_);
    }
#endif
  }

#ifdef ARTP_PLANNER_REFERENCE_SURFACE
  // planner.h:65.  The grid map stays alive inside map_ (map_->getMap(), planner_ros.cpp:339).
  void setMap(std::unique_ptr<grid_map::GridMap>&& map) {
    if (!map) return;
    setMap(std::make_unique<Map>(std::move(map)));
  }

  // planner.h:67-68
  PlannerStatus plan(const ob::ScopedState<>& start, const ob::ScopedState<>& goal) {
    return plan(*start.get()->as<StateType>(), *goal.get()->as<StateType>());
  }

  // planner.h:70
  og::PathGeometric getSolutionPath(const bool& simplify = false) const {
    const Path flat = getSolutionPathFlat(simplify);
    const ob::SpaceInformationPtr si = ss_->getSpaceInformation();
    og::PathGeometric path(si);
    ob::State* st = si->allocState();
    for (const StateArray& s : flat) {
      unflattenSE3(s.data(), st);
      path.append(st);   // copies the state
    }
    si->freeState(st);
    return path;
  }
#else
  Path getSolutionPath(const bool& simplify = false) const { return getSolutionPathFlat(simplify); }
#endif

  bool hasMap() const {
    std::lock_guard<std::mutex> lock(map_mutex_);
    return static_cast<bool>(map_);
  }

#ifdef ARTP_PLANNER_REFERENCE_SURFACE
  // true: checkMotion keeps the segment length of the FIRST map planned on (the reference's behaviour, see setMap) -- the map
  // installed at the time of the call, else the next one; false (default): it follows the bounds of every map.
  void setFreezeMotionResolution(bool freeze) {
    std::lock_guard<std::mutex> lock(map_mutex_);
    freeze_motion_resolution_ = freeze;
    motion_resolution_set_ = false;
    if (!freeze) {
      throwOnError(gpu_->get(), artp_set_r3_extent(gpu_->get(), 0.0), "artp_set_r3_extent");
    } else if (map_) {
      captureMotionResolution();   // the map planned on now is "the first map": later setMap calls keep its segment length
    }
  }

 private:
  // fix checkMotion's R^3 maxExtent at the current bounds (caller holds map_mutex_)
  void captureMotionResolution() {
    const double ex = high_[0] - low_[0], ey = high_[1] - low_[1], ez = high_[2] - low_[2];
    throwOnError(gpu_->get(), artp_set_r3_extent(gpu_->get(), std::sqrt(ex * ex + ey * ey + ez * ez)), "artp_set_r3_extent");
    motion_resolution_set_ = true;
  }

 public:
#endif

#ifdef ARTP_PLANNER_REFERENCE_SURFACE
  // "prm_motion_cost" only.  Default (false): the roadmap's edges are priced through the MotionCostFunc of the
  // PRMMotionCostMaintainer the caller installed (prm_motion_cost.cpp:27-73) -- PlannerRos' service client stays the cost
  // source.  true = explicit opt-in to the learned-cost network on the device (artp_cost_load_weights +
  // artp_cost_update_map; no host round trip per batch); the functor is then out of the planning loop.
  void setDevicePricing(bool on) {
    std::lock_guard<std::mutex> lock(map_mutex_);
    if (params_->planner.name != "prm_motion_cost") return;
    ss_->getPlanner()->as<PRMMotionCost>()->setDevicePricing(on);
    prm_->clear();          // edges priced by the other source are not comparable: the next plan() builds anew
    rb_->built = false;
  }
#endif

  // The per-call seams of OMPL (StateValidityChecker::isValid on arbitrary states, MotionValidator::checkMotion one edge at
  // a time: PathSimplifier, the lazy planners' path check) answered by resident workgroups instead of a launch per call
  // (GpuContext::setPersistentLatency; 17 -> 12 us and 33 -> 25 us per call on an MI355X).
  void setPersistentLatency(bool on) { gpu_->setPersistentLatency(on); }

  // Where on the map the robot can stand, and at which headings (artp_reachability_map, include/artp_c.h): mask[r + c rows]
  // bit k = isValid of the goal plan() would make of cell (r, c) at yaw 2 pi k / n_yaw.  Also stores the share of valid
  // headings per cell as the float layer "reachability" of the planner's Map (and of its grid_map where it holds one), so
  // a PlannerRos-shaped host can publish it with the map.
  std::vector<uint32_t> computeReachability(unsigned n_yaw) {
    std::lock_guard<std::mutex> lock(map_mutex_);
    if (!map_) throw std::runtime_error("computeReachability: the planner does not have a map set");
    const auto g = map_->getGeometry();
    std::vector<uint32_t> mask(static_cast<size_t>(g.rows) * g.cols);
    throwOnError(gpu_->get(), artp_reachability_map(gpu_->get(), static_cast<int>(n_yaw), nullptr, mask.data()),
                 "artp_reachability_map");
    std::vector<float> share(mask.size());
    for (size_t i = 0; i < mask.size(); ++i)
      share[i] = static_cast<float>(__builtin_popcount(mask[i])) / static_cast<float>(n_yaw);
    map_->addLayer("reachability", share.data());
#ifdef ARTP_HAVE_GRID_MAP
    if (map_->hasGridMap()) {
      auto& gm = map_->getMap();
      gm.add("reachability", 0.0f);
      float* d = gm.get("reachability").data();
      for (size_t i = 0; i < share.size(); ++i) d[i] = share[i];
    }
#endif
    return mask;
  }

  // Cost-to-go field over the lattice of a reachability mask (artp_field_compute, include/artp_c.h): the smallest
  // PathLengthObjective cost of a lattice path from any source (r, c, k) to every cell and heading, or to the sources for
  // reverse.  mask = what computeReachability(n_yaw) returned, or an edited copy (keep-out zones).  Returns dist,
  // index (r + c rows) n_yaw + k, +inf where unreachable, and stores the smallest cost over the headings of each cell
  // as the float layer "cost_to_go" of the planner's Map.  The objective and its velocities come from
  // Params::objectives.custom_path_length.  Lattice paths are proposals: their moves' interior states are not checked
  // (planOnCostField checks them and takes the verdicts back into a kept field).
  std::vector<double> computeCostField(const std::vector<uint32_t>& mask, unsigned n_yaw,
                                       const std::vector<std::array<int, 3>>& sources, bool reverse = false,
                                       artp_field** keep = nullptr) {
    std::lock_guard<std::mutex> lock(map_mutex_);
    if (!map_) throw std::runtime_error("computeCostField: the planner does not have a map set");
    const auto g = map_->getGeometry();
    const size_t cells = static_cast<size_t>(g.rows) * g.cols;
    if (mask.size() != cells) throw std::runtime_error("computeCostField: the mask does not have rows * cols words");
    const artp_field_params fp = costFieldParams();
    std::vector<int> src;
    for (const auto& s : sources) src.insert(src.end(), s.begin(), s.end());
    artp_field* f = nullptr;
    throwOnError(gpu_->get(),
                 artp_field_compute(gpu_->get(), &fp, static_cast<int>(n_yaw), nullptr, mask.data(), 0, src.data(),
                                    sources.size(), reverse ? 1 : 0, &f),
                 "artp_field_compute");
    return finishCostField(f, cells, n_yaw, keep);
  }

  // computeCostField for many source sets at once (artp_field_compute_many, include/artp_c.h): one field per set, all
  // searched side by side in one batched call; field b holds the bits of computeCostField(mask, n_yaw, source_sets[b]).
  // Returns the kept fields, one per set: each works with artp_field_dist, artp_field_path, updateCostField,
  // planOnCostField and the rest on its own, and the caller destroys each (artp_field_destroy).  One bad source refuses
  // the whole call (the exception names its set) and leaves nothing allocated.  The "cost_to_go" layer is not touched:
  // it holds one field.
  std::vector<artp_field*> computeCostFields(const std::vector<uint32_t>& mask, unsigned n_yaw,
                                             const std::vector<std::vector<std::array<int, 3>>>& source_sets,
                                             bool reverse = false) {
    std::lock_guard<std::mutex> lock(map_mutex_);
    if (!map_) throw std::runtime_error("computeCostFields: the planner does not have a map set");
    const auto g = map_->getGeometry();
    if (mask.size() != static_cast<size_t>(g.rows) * g.cols)
      throw std::runtime_error("computeCostFields: the mask does not have rows * cols words");
    const artp_field_params fp = costFieldParams();
    std::vector<int> src;
    std::vector<uint64_t> off(1, 0);
    for (const auto& set : source_sets) {
      for (const auto& s : set) src.insert(src.end(), s.begin(), s.end());
      off.push_back(src.size() / 3);
    }
    if (src.empty()) src.resize(3, 0);   // a pointer the library can refuse the empty call behind
    std::vector<artp_field*> fields(std::max<size_t>(source_sets.size(), 1), nullptr);
    throwOnError(gpu_->get(),
                 artp_field_compute_many(gpu_->get(), &fp, static_cast<int>(n_yaw), nullptr, mask.data(), 0, src.data(),
                                         off.data(), source_sets.size(), reverse ? 1 : 0, fields.data()),
                 "artp_field_compute_many");
    fields.resize(source_sets.size());
    return fields;
  }

  // Pose-to-pose costs (artp_field_cost_matrix, include/artp_c.h): entry i * n + j = the cost from poses[i] to poses[j],
  // the forward field of pose i read at pose j; +inf where unreachable, 0 on the diagonal, bit for bit
  // computeCostField's values.  The n fields are computed in batched groups of at most `batch` (0: as many as fit in
  // half of the free device memory) and freed group by group.  stats (may be null): groups, fields, rounds, tile runs.
  std::vector<double> computeCostMatrix(const std::vector<uint32_t>& mask, unsigned n_yaw,
                                        const std::vector<std::array<int, 3>>& poses, size_t batch = 0,
                                        artp_field_many_stats_t* stats = nullptr) {
    std::lock_guard<std::mutex> lock(map_mutex_);
    if (!map_) throw std::runtime_error("computeCostMatrix: the planner does not have a map set");
    const auto g = map_->getGeometry();
    if (mask.size() != static_cast<size_t>(g.rows) * g.cols)
      throw std::runtime_error("computeCostMatrix: the mask does not have rows * cols words");
    const artp_field_params fp = costFieldParams();
    std::vector<int> p;
    for (const auto& s : poses) p.insert(p.end(), s.begin(), s.end());
    if (p.empty()) p.resize(3, 0);
    std::vector<double> matrix(std::max<size_t>(poses.size() * poses.size(), 1));
    throwOnError(gpu_->get(),
                 artp_field_cost_matrix(gpu_->get(), &fp, static_cast<int>(n_yaw), nullptr, mask.data(), 0, p.data(),
                                        poses.size(), batch, matrix.data(), stats),
                 "artp_field_cost_matrix");
    matrix.resize(poses.size() * poses.size());
    return matrix;
  }

  // computeCostField under the learned motion cost (artp_field_compute_learned, include/artp_c.h): every lattice move is
  // priced by the network on the device, which must hold weights and a feature map (artp_cost_load_weights,
  // artp_cost_update_map*).  The weights and the risk threshold are Params::planner.prm_motion_cost's, the numbers
  // setDevicePricing(true) gives the roadmap.  The cost is not symmetric: reverse is another field.  A kept field
  // cannot go through updateCostField (the library refuses it): updateLearnedCostField takes it.  Refreshes the
  // "cost_to_go" layer.
  std::vector<double> computeLearnedCostField(const std::vector<uint32_t>& mask, unsigned n_yaw,
                                              const std::vector<std::array<int, 3>>& sources, bool reverse = false,
                                              artp_field** keep = nullptr) {
    std::lock_guard<std::mutex> lock(map_mutex_);
    if (!map_) throw std::runtime_error("computeLearnedCostField: the planner does not have a map set");
    const auto g = map_->getGeometry();
    const size_t cells = static_cast<size_t>(g.rows) * g.cols;
    if (mask.size() != cells) throw std::runtime_error("computeLearnedCostField: the mask does not have rows * cols words");
    artp_field_learned_params lp;
    artp_field_learned_params_defaults(&lp);
    const auto& pmc = params_->planner.prm_motion_cost;
    lp.w_energy = pmc.cost_weights.energy;
    lp.w_time = pmc.cost_weights.time;
    lp.w_risk = pmc.cost_weights.risk;
    lp.risk_threshold = pmc.risk_threshold;
    std::vector<int> src;
    for (const auto& s : sources) src.insert(src.end(), s.begin(), s.end());
    artp_field* f = nullptr;
    throwOnError(gpu_->get(),
                 artp_field_compute_learned(gpu_->get(), &lp, static_cast<int>(n_yaw), nullptr, mask.data(), 0, src.data(),
                                            sources.size(), reverse ? 1 : 0, &f),
                 "artp_field_compute_learned");
    return finishCostField(f, cells, n_yaw, keep);
  }

  // How far every node of a reachability mask is from the nearest cell where its heading -- and yaw_spread neighbours on
  // either side -- is not a valid pose (artp_clearance_map, include/artp_c.h): d2, index (r + c rows) n_yaw + k, the exact
  // squared distance in cells; 0 = not a node, 0xffff = nothing within radius_cells.  The clearance in metres is
  // res * sqrt(d2).
  std::vector<uint16_t> computeClearance(const std::vector<uint32_t>& mask, unsigned n_yaw, int radius_cells = 12,
                                         int yaw_spread = 0, bool outside_is_obstacle = false) {
    std::lock_guard<std::mutex> lock(map_mutex_);
    if (!map_) throw std::runtime_error("computeClearance: the planner does not have a map set");
    const auto g = map_->getGeometry();
    const size_t cells = static_cast<size_t>(g.rows) * g.cols;
    if (mask.size() != cells) throw std::runtime_error("computeClearance: the mask does not have rows * cols words");
    artp_clearance_params cp;
    artp_clearance_params_defaults(&cp);
    cp.radius_cells = radius_cells;
    cp.yaw_spread = yaw_spread;
    cp.outside_is_obstacle = outside_is_obstacle ? 1 : 0;
    std::vector<uint16_t> d2(cells * (n_yaw >= 1 && n_yaw <= 32 ? n_yaw : 1));
    throwOnError(gpu_->get(),
                 artp_clearance_map(gpu_->get(), &cp, static_cast<int>(n_yaw), g.rows, g.cols, mask.data(), 0, d2.data()),
                 "artp_clearance_map");
    return d2;
  }

  // computeCostField with every move's cost inflated near obstacles (artp_field_compute_clearance, include/artp_c.h):
  // w(a -> b) = base (1 + gain max(pen(a), pen(b))), pen(v) = max(0, 1 - res sqrt(d2[v]) / margin) with d2 the clearance
  // map of the mask; margin (metres) may not exceed radius_cells * res; gain = 0 gives computeCostField's bits.  A kept
  // field works with blockCostFieldMoves, unblockCostField and planOnCostField; updateCostField and
  // updateLearnedCostField refuse it (a mask edit moves clearances up to radius_cells around it):
  // updateClearanceCostField takes it.  Refreshes the "cost_to_go" layer.
  std::vector<double> computeClearanceCostField(const std::vector<uint32_t>& mask, unsigned n_yaw,
                                                const std::vector<std::array<int, 3>>& sources, double margin = 0.2,
                                                double gain = 2.0, int radius_cells = 12, int yaw_spread = 0,
                                                bool outside_is_obstacle = false, bool reverse = false,
                                                artp_field** keep = nullptr) {
    std::lock_guard<std::mutex> lock(map_mutex_);
    if (!map_) throw std::runtime_error("computeClearanceCostField: the planner does not have a map set");
    const auto g = map_->getGeometry();
    const size_t cells = static_cast<size_t>(g.rows) * g.cols;
    if (mask.size() != cells) throw std::runtime_error("computeClearanceCostField: the mask does not have rows * cols words");
    artp_field_clearance_params fp;
    artp_field_clearance_params_defaults(&fp);
    const auto& cpl = params_->objectives.custom_path_length;
    fp.base.objective = cpl.use_directional_cost ? 1 : 0;
    fp.base.max_lon_vel = cpl.max_lon_vel;
    fp.base.max_lat_vel = cpl.max_lat_vel;
    fp.base.max_ang_vel = cpl.max_ang_vel;
    fp.clearance.radius_cells = radius_cells;
    fp.clearance.yaw_spread = yaw_spread;
    fp.clearance.outside_is_obstacle = outside_is_obstacle ? 1 : 0;
    fp.margin = margin;
    fp.gain = gain;
    std::vector<int> src;
    for (const auto& s : sources) src.insert(src.end(), s.begin(), s.end());
    artp_field* f = nullptr;
    throwOnError(gpu_->get(),
                 artp_field_compute_clearance(gpu_->get(), &fp, static_cast<int>(n_yaw), nullptr, mask.data(), 0, src.data(),
                                              sources.size(), reverse ? 1 : 0, &f),
                 "artp_field_compute_clearance");
    return finishCostField(f, cells, n_yaw, keep);
  }

  // computeLearnedCostField / computeClearanceCostField for many source sets at once, and the pose-to-pose matrices under
  // the two costs (artp_field_compute_many_learned / _clearance, artp_field_cost_matrix_learned / _clearance,
  // include/artp_c.h): the weight table is priced once per call and every field searches it side by side.  Field b holds
  // the bits of the single call on source_sets[b] and owns its own copy of the table: each works with
  // updateLearnedCostField / updateClearanceCostField, planOnCostField and the rest alone, and the caller destroys each.
  // The learned cost is not symmetric, and neither is its matrix.  A matrix's table is freed with the call; table (may be
  // null) receives its numbers.  The "cost_to_go" layer is not touched.
  std::vector<artp_field*> computeLearnedCostFields(const std::vector<uint32_t>& mask, unsigned n_yaw,
                                                    const std::vector<std::vector<std::array<int, 3>>>& source_sets,
                                                    bool reverse = false) {
    const artp_field_learned_params lp = learnedFieldParams();
    return manyWeightedFields("computeLearnedCostFields", "artp_field_compute_many_learned", mask, source_sets,
                              [&](const int* src, const uint64_t* off, artp_field** out) {
                                return artp_field_compute_many_learned(gpu_->get(), &lp, static_cast<int>(n_yaw), nullptr,
                                                                       mask.data(), 0, src, off, source_sets.size(),
                                                                       reverse ? 1 : 0, out);
                              });
  }

  std::vector<artp_field*> computeClearanceCostFields(const std::vector<uint32_t>& mask, unsigned n_yaw,
                                                      const std::vector<std::vector<std::array<int, 3>>>& source_sets,
                                                      double margin = 0.2, double gain = 2.0, int radius_cells = 12,
                                                      int yaw_spread = 0, bool outside_is_obstacle = false,
                                                      bool reverse = false) {
    const artp_field_clearance_params fp = clearanceFieldParams(margin, gain, radius_cells, yaw_spread, outside_is_obstacle);
    return manyWeightedFields("computeClearanceCostFields", "artp_field_compute_many_clearance", mask, source_sets,
                              [&](const int* src, const uint64_t* off, artp_field** out) {
                                return artp_field_compute_many_clearance(gpu_->get(), &fp, static_cast<int>(n_yaw), nullptr,
                                                                         mask.data(), 0, src, off, source_sets.size(),
                                                                         reverse ? 1 : 0, out);
                              });
  }

  std::vector<double> computeLearnedCostMatrix(const std::vector<uint32_t>& mask, unsigned n_yaw,
                                               const std::vector<std::array<int, 3>>& poses, size_t batch = 0,
                                               artp_field_many_stats_t* stats = nullptr,
                                               artp_field_many_table_stats_t* table = nullptr) {
    const artp_field_learned_params lp = learnedFieldParams();
    return weightedCostMatrix("computeLearnedCostMatrix", "artp_field_cost_matrix_learned", mask, poses,
                              [&](const int* p, double* m) {
                                return artp_field_cost_matrix_learned(gpu_->get(), &lp, static_cast<int>(n_yaw), nullptr,
                                                                      mask.data(), 0, p, poses.size(), batch, m, stats, table);
                              });
  }

  std::vector<double> computeClearanceCostMatrix(const std::vector<uint32_t>& mask, unsigned n_yaw,
                                                 const std::vector<std::array<int, 3>>& poses, size_t batch = 0,
                                                 double margin = 0.2, double gain = 2.0, int radius_cells = 12,
                                                 int yaw_spread = 0, bool outside_is_obstacle = false,
                                                 artp_field_many_stats_t* stats = nullptr,
                                                 artp_field_many_table_stats_t* table = nullptr) {
    const artp_field_clearance_params fp = clearanceFieldParams(margin, gain, radius_cells, yaw_spread, outside_is_obstacle);
    return weightedCostMatrix("computeClearanceCostMatrix", "artp_field_cost_matrix_clearance", mask, poses,
                              [&](const int* p, double* m) {
                                return artp_field_cost_matrix_clearance(gpu_->get(), &fp, static_cast<int>(n_yaw), nullptr,
                                                                        mask.data(), 0, p, poses.size(), batch, m, stats,
                                                                        table);
                              });
  }

 private:
  // Params::planner.prm_motion_cost's weights and threshold, as computeLearnedCostField passes them
  artp_field_learned_params learnedFieldParams() const {
    artp_field_learned_params lp;
    artp_field_learned_params_defaults(&lp);
    const auto& pmc = params_->planner.prm_motion_cost;
    lp.w_energy = pmc.cost_weights.energy;
    lp.w_time = pmc.cost_weights.time;
    lp.w_risk = pmc.cost_weights.risk;
    lp.risk_threshold = pmc.risk_threshold;
    return lp;
  }

  // Params::objectives.custom_path_length's base objective with the clearance weighting, as computeClearanceCostField
  artp_field_clearance_params clearanceFieldParams(double margin, double gain, int radius_cells, int yaw_spread,
                                                   bool outside_is_obstacle) const {
    artp_field_clearance_params fp;
    artp_field_clearance_params_defaults(&fp);
    const auto& cpl = params_->objectives.custom_path_length;
    fp.base.objective = cpl.use_directional_cost ? 1 : 0;
    fp.base.max_lon_vel = cpl.max_lon_vel;
    fp.base.max_lat_vel = cpl.max_lat_vel;
    fp.base.max_ang_vel = cpl.max_ang_vel;
    fp.clearance.radius_cells = radius_cells;
    fp.clearance.yaw_spread = yaw_spread;
    fp.clearance.outside_is_obstacle = outside_is_obstacle ? 1 : 0;
    fp.margin = margin;
    fp.gain = gain;
    return fp;
  }

  // the map check, the flattened sets and the handles of a batched weighted call; call(sources, offsets, out_fields)
  template <class Call>
  std::vector<artp_field*> manyWeightedFields(const char* who, const char* entry, const std::vector<uint32_t>& mask,
                                              const std::vector<std::vector<std::array<int, 3>>>& source_sets, Call&& call) {
    std::lock_guard<std::mutex> lock(map_mutex_);
    if (!map_) throw std::runtime_error(std::string(who) + ": the planner does not have a map set");
    const auto g = map_->getGeometry();
    if (mask.size() != static_cast<size_t>(g.rows) * g.cols)
      throw std::runtime_error(std::string(who) + ": the mask does not have rows * cols words");
    std::vector<int> src;
    std::vector<uint64_t> off(1, 0);
    for (const auto& set : source_sets) {
      for (const auto& s : set) src.insert(src.end(), s.begin(), s.end());
      off.push_back(src.size() / 3);
    }
    if (src.empty()) src.resize(3, 0);   // a pointer the library can refuse the empty call behind
    std::vector<artp_field*> fields(std::max<size_t>(source_sets.size(), 1), nullptr);
    throwOnError(gpu_->get(), call(src.data(), off.data(), fields.data()), entry);
    fields.resize(source_sets.size());
    return fields;
  }

  // the same for a weighted matrix; call(poses, matrix_out)
  template <class Call>
  std::vector<double> weightedCostMatrix(const char* who, const char* entry, const std::vector<uint32_t>& mask,
                                         const std::vector<std::array<int, 3>>& poses, Call&& call) {
    std::lock_guard<std::mutex> lock(map_mutex_);
    if (!map_) throw std::runtime_error(std::string(who) + ": the planner does not have a map set");
    const auto g = map_->getGeometry();
    if (mask.size() != static_cast<size_t>(g.rows) * g.cols)
      throw std::runtime_error(std::string(who) + ": the mask does not have rows * cols words");
    std::vector<int> p;
    for (const auto& s : poses) p.insert(p.end(), s.begin(), s.end());
    if (p.empty()) p.resize(3, 0);
    std::vector<double> matrix(std::max<size_t>(poses.size() * poses.size(), 1));
    throwOnError(gpu_->get(), call(p.data(), matrix.data()), entry);
    matrix.resize(poses.size() * poses.size());
    return matrix;
  }

 public:

  // The field a computeCostField call kept, brought in place to an edited mask (artp_field_update, include/artp_c.h):
  // the same bits as computeCostField on it, at the price of the region whose costs change.  mask = rows * cols words;
  // rect = (row0, col0, nrows, ncols) of the words that may differ (nullptr = all of them; the others are not read).
  // refresh_heights re-reads the map's heights inside rect.  Returns dist and refreshes the "cost_to_go" layer.
  std::vector<double> updateCostField(artp_field* kept, const std::vector<uint32_t>& mask,
                                      const std::array<int, 4>* rect = nullptr, bool refresh_heights = false) {
    return updateKeptField("updateCostField", "artp_field_update", kept, mask, false, [&] {
      return artp_field_update(kept, mask.data(), 0, rect ? rect->data() : nullptr, refresh_heights ? 1 : 0);
    });
  }

  // The field a computeCostField call kept, carried across a move of the map by whole cells (artp_field_shift,
  // include/artp_c.h): setMap has installed the new map, whose position differs from the old one's by whole cells; node
  // (r, c, k) becomes (r + si, c + sj, k) with si = lround((pos_x_new - pos_x_old) / res), sj likewise.  mask = rows *
  // cols words on the NEW map (computeReachability, or an edited copy); every word is read.  The same bits as
  // computeCostField on the new map with the sources moved.  refresh_heights re-reads every height; without it the kept
  // cells keep theirs.  Throws, with the field unchanged, when a moved source leaves the map or is no node of mask, when
  // the new map has another size or resolution, and for a learned or clearance-weighted field (compute those anew).
  // Returns dist and refreshes the "cost_to_go" layer.
  std::vector<double> shiftCostField(artp_field* kept, const std::vector<uint32_t>& mask, bool refresh_heights = true) {
    return updateKeptField("shiftCostField", "artp_field_shift", kept, mask, false,
                           [&] { return artp_field_shift(kept, mask.data(), 0, refresh_heights ? 1 : 0); });
  }

  // The field a computeClearanceCostField call kept, brought in place to an edited mask (artp_field_update_clearance,
  // include/artp_c.h): the clearance map and the move costs computed again around rect, then updateCostField's passes.
  // mask, rect and refresh_heights as updateCostField takes them.  The same bits as computeClearanceCostField with the
  // field's own parameters on that mask.  Returns dist and refreshes the "cost_to_go" layer.
  std::vector<double> updateClearanceCostField(artp_field* kept, const std::vector<uint32_t>& mask,
                                               const std::array<int, 4>* rect = nullptr, bool refresh_heights = false) {
    return updateKeptField("updateClearanceCostField", "artp_field_update_clearance", kept, mask, false, [&] {
      return artp_field_update_clearance(kept, mask.data(), 0, rect ? rect->data() : nullptr, refresh_heights ? 1 : 0);
    });
  }

  // The field a computeClearanceCostField call kept, carried across a move of the map by whole cells
  // (artp_field_shift_clearance, include/artp_c.h): shiftCostField for the clearance-weighted field.  The clearance map is
  // computed again on the new map and every move priced again against the weight its node carried across the move.  mask
  // and refresh_heights as shiftCostField takes them.  The same bits as computeClearanceCostField with the field's own
  // parameters on the new map with the sources moved.  Throws, with the field unchanged, where shiftCostField throws and
  // for any field that is not clearance-weighted.  The first call that moves keeps a second weight table as large as the
  // field's own.  Returns dist and refreshes the "cost_to_go" layer.
  std::vector<double> shiftClearanceCostField(artp_field* kept, const std::vector<uint32_t>& mask,
                                              bool refresh_heights = true) {
    return updateKeptField("shiftClearanceCostField", "artp_field_shift_clearance", kept, mask, false,
                           [&] { return artp_field_shift_clearance(kept, mask.data(), 0, refresh_heights ? 1 : 0); });
  }

  // The field a computeLearnedCostField call kept, brought in place to the device's current state
  // (artp_field_update_learned, include/artp_c.h): every move priced again by the loaded network on the cost map of the
  // last artp_cost_update_map*, and the mask edited as updateCostField edits it (an empty mask = the mask did not change;
  // rect is then ignored).  The same bits as computeLearnedCostField on that state.  Returns dist and refreshes the
  // "cost_to_go" layer.
  std::vector<double> updateLearnedCostField(artp_field* kept, const std::vector<uint32_t>& mask,
                                             const std::array<int, 4>* rect = nullptr) {
    return updateKeptField("updateLearnedCostField", "artp_field_update_learned", kept, mask, true, [&] {
      return artp_field_update_learned(kept, mask.empty() ? nullptr : mask.data(), 0, rect ? rect->data() : nullptr);
    });
  }

  // Single moves taken out of a kept field (artp_field_block_moves, include/artp_c.h): from[i] -> to[i] in travel
  // direction, each one of the ten lattice moves; the field is repaired in place and holds the bits of a new field with
  // the same moves blocked.  Only the stated direction is blocked.  Returns dist and refreshes the "cost_to_go" layer.
  std::vector<double> blockCostFieldMoves(artp_field* kept, const std::vector<std::array<int, 3>>& from,
                                          const std::vector<std::array<int, 3>>& to, uint64_t* newly_blocked = nullptr) {
    std::lock_guard<std::mutex> lock(map_mutex_);
    if (!map_) throw std::runtime_error("blockCostFieldMoves: the planner does not have a map set");
    if (!kept) throw std::runtime_error("blockCostFieldMoves: no field");
    if (from.size() != to.size()) throw std::runtime_error("blockCostFieldMoves: from and to differ in length");
    const auto g = map_->getGeometry();
    const size_t cells = static_cast<size_t>(g.rows) * g.cols;
    artp_field_stats_t st;
    throwOnError(gpu_->get(), artp_field_stats(kept, &st), "artp_field_stats");
    if (st.nodes % cells != 0) throw std::runtime_error("blockCostFieldMoves: the field does not have rows * cols cells");
    std::vector<int> a, b;
    for (const auto& s : from) a.insert(a.end(), s.begin(), s.end());
    for (const auto& s : to) b.insert(b.end(), s.begin(), s.end());
    throwOnError(gpu_->get(), artp_field_block_moves(kept, a.data(), b.data(), from.size(), newly_blocked),
                 "artp_field_block_moves");
    return refreshCostToGo(kept, cells, st.nodes);
  }

  // The blocked moves of the nodes whose cell lies in rect = (row0, col0, nrows, ncols) given back to a kept field
  // (artp_field_unblock; nullptr = all of them): what a caller runs after the map changed there -- the written rectangle
  // grown by artp_reachability_halo() plus one cell is enough.  Returns dist and refreshes the "cost_to_go" layer.
  std::vector<double> unblockCostField(artp_field* kept, const std::array<int, 4>* rect = nullptr,
                                       uint64_t* unblocked = nullptr) {
    std::lock_guard<std::mutex> lock(map_mutex_);
    if (!map_) throw std::runtime_error("unblockCostField: the planner does not have a map set");
    if (!kept) throw std::runtime_error("unblockCostField: no field");
    const auto g = map_->getGeometry();
    const size_t cells = static_cast<size_t>(g.rows) * g.cols;
    artp_field_stats_t st;
    throwOnError(gpu_->get(), artp_field_stats(kept, &st), "artp_field_stats");
    if (st.nodes % cells != 0) throw std::runtime_error("unblockCostField: the field does not have rows * cols cells");
    throwOnError(gpu_->get(), artp_field_unblock(kept, rect ? rect->data() : nullptr, unblocked), "artp_field_unblock");
    return refreshCostToGo(kept, cells, st.nodes);
  }

  // Lazily checked lattice paths on a kept field (artp_field_plan): per round the field's path to every pending target,
  // checkMotion of all their moves in one device batch, the failing moves blocked and the field repaired, at most
  // max_rounds rounds.  status 0: every move of the path passed (nodes and SE3 states in travel order, cost =
  // dist[target]); 1: unreachable; 2: rounds exhausted.  The blocks stay on the field: a second call continues.
  // Refreshes the "cost_to_go" layer, since the blocks move the field.  stats (may be null) takes the numbers of the
  // call; should the paths outgrow the buffers, the call is made again with larger ones and stats holds both together.
  // simplify = true: the status-0 paths go through simplifyCostFieldPaths(window) in one call; `simplified` and
  // `simplified_cost` take the kept states and their cost under that call's pricing (empty and +inf otherwise).
  struct CostFieldPlan {
    int status = 2;
    std::vector<std::array<int, 3>> nodes;
    std::vector<std::array<double, 7>> states;
    double cost = std::numeric_limits<double>::infinity();
    std::vector<std::array<double, 7>> simplified;
    double simplified_cost = std::numeric_limits<double>::infinity();
  };
  // One path of simplifyCostFieldPaths: status 0 = simplified, 1 = the input itself does not pass (returned unchanged,
  // cost +inf), 2 = empty; kept = the indices of the kept input states, ascending from 0 to n - 1.
  struct SimplifiedPath {
    int status = 2;
    std::vector<uint32_t> kept;
    std::vector<std::array<double, 7>> states;
    double cost = std::numeric_limits<double>::infinity();
  };
  // Windowed shortcut simplification of many paths in one device call (artp_field_simplify_paths, include/artp_c.h):
  // per path the cheapest chain of shortcuts between states at most `window` apart (0 = all pairs) that pass the 0.5 m
  // interpolation rule and checkMotion, priced by the field's objective and velocities (a clearance-weighted field:
  // unweighted).  With a window that covers a path: what getSolutionPath(true) makes of it.  The field is not changed.
  std::vector<SimplifiedPath> simplifyCostFieldPaths(artp_field* kept,
                                                     const std::vector<std::vector<std::array<double, 7>>>& paths,
                                                     unsigned window = 64, artp_field_simplify_stats_t* stats = nullptr) {
    std::lock_guard<std::mutex> lock(map_mutex_);
    if (!map_) throw std::runtime_error("simplifyCostFieldPaths: the planner does not have a map set");
    if (!kept) throw std::runtime_error("simplifyCostFieldPaths: no field");
    return simplifyPathsLocked(kept, paths, window, stats);
  }

  std::vector<CostFieldPlan> planOnCostField(artp_field* kept, const std::vector<std::array<int, 3>>& targets,
                                             int max_rounds = 64, artp_field_plan_stats_t* stats = nullptr,
                                             bool simplify = false, unsigned window = 64) {
    std::lock_guard<std::mutex> lock(map_mutex_);
    if (!map_) throw std::runtime_error("planOnCostField: the planner does not have a map set");
    if (!kept) throw std::runtime_error("planOnCostField: no field");
    const auto g = map_->getGeometry();
    const size_t cells = static_cast<size_t>(g.rows) * g.cols;
    artp_field_stats_t st;
    throwOnError(gpu_->get(), artp_field_stats(kept, &st), "artp_field_stats");
    if (st.nodes % cells != 0) throw std::runtime_error("planOnCostField: the field does not have rows * cols cells");
    const size_t n = targets.size();
    std::vector<CostFieldPlan> out(n);
    artp_field_plan_stats_t sum{};
    if (stats) *stats = sum;
    if (!n) return out;
    std::vector<int> t;
    for (const auto& s : targets) t.insert(t.end(), s.begin(), s.end());
    std::vector<int32_t> status(n);
    std::vector<double> cost(n);
    std::vector<uint64_t> off(n + 1, 0);
    size_t cap = 1024 * n;
    std::vector<int> nodes;
    std::vector<double> se3;
    int rounds_left = max_rounds;
    for (;;) {   // a second pass only when the paths hold more states than cap: the blocks of the first stay
      nodes.resize(3 * cap);
      se3.resize(7 * cap);
      const int rc = artp_field_plan(kept, t.data(), n, std::max(rounds_left, 1), status.data(), cost.data(), off.data(),
                                     nodes.data(), se3.data(), cap);
      artp_field_plan_stats_t one{};
      if ((rc == ARTP_OK || rc == ARTP_ERR_CAPACITY) && artp_field_plan_stats(kept, &one) == ARTP_OK) {
        sum.rounds += one.rounds;
        sum.moves_checked += one.moves_checked;
        sum.moves_blocked += one.moves_blocked;
        sum.updates += one.updates;
        sum.update_tile_runs += one.update_tile_runs;
        if (one.updates) sum.last_update_tile_runs = one.last_update_tile_runs;
        sum.descent_ms += one.descent_ms;
        sum.check_ms += one.check_ms;
        sum.round_ms += one.round_ms;
        sum.passes_ms += one.passes_ms;
      }
      if (rc == ARTP_ERR_CAPACITY && off[n] > cap) {
        cap = static_cast<size_t>(off[n]);
        rounds_left = max_rounds - static_cast<int>(sum.rounds);
        continue;
      }
      throwOnError(gpu_->get(), rc, "artp_field_plan");
      break;
    }
    for (size_t i = 0; i < n; ++i) {
      out[i].status = status[i];
      out[i].cost = cost[i];
      for (uint64_t s = off[i]; s < off[i + 1]; ++s) {
        out[i].nodes.push_back({{nodes[3 * s], nodes[3 * s + 1], nodes[3 * s + 2]}});
        std::array<double, 7> q;
        for (int j = 0; j < 7; ++j) q[j] = se3[7 * s + j];
        out[i].states.push_back(q);
      }
    }
    if (stats) *stats = sum;
    refreshCostToGo(kept, cells, st.nodes);
    if (simplify) {
      std::vector<std::vector<std::array<double, 7>>> paths;
      for (const CostFieldPlan& p : out)
        if (p.status == 0) paths.push_back(p.states);
      const std::vector<SimplifiedPath> simple = simplifyPathsLocked(kept, paths, window, nullptr);
      size_t at = 0;
      for (CostFieldPlan& p : out)
        if (p.status == 0) {
          p.simplified = simple[at].states;
          p.simplified_cost = simple[at].cost;
          ++at;
        }
    }
    return out;
  }

  void setSeed(uint64_t seed) {
    seed_ = seed;
    prm_->setSeed(seed);
    if (tree_) tree_->setSeed(seed);
  }

  // Build the roadmap in the reference planners' own insertion order instead of the batched front end:
  // PRMMotionCost::addValidMilestone's graph for "prm_motion_cost" (prm_motion_cost.cpp:325-390), LazyPRMStarMinUpdate's
  // for the LazyPRM* names (lazy_prm_star_min_update.cpp:424-446).  Same answers as the reference's graph gives, at
  // the price of the sequential insertion loop (include/artp_c.h, artp_roadmap_params::construction).  The kept
  // roadmap is dropped; the next plan() samples a new one.
  void setReferenceConstruction(bool on) {
    std::lock_guard<std::mutex> lock(map_mutex_);
    prm_->setConstruction(!on ? 0 : (params_->planner.name == "prm_motion_cost" ? 1 : 2));
    prm_->clear();
    rb_->built = false;
  }

  // planner.cpp:192-262
  PlannerStatus plan(const StateType& start, const StateType& goal) {
    std::lock_guard<std::mutex> lock(map_mutex_);
    if (!map_) {
      std::cout << "Planner does not have the elevation map set, yet." << std::endl;
      return PlannerStatus::NO_MAP;
    }
    const StateArray start_flat = BatchPRM::flatten(start);
    // enforce the goal inside the bounds (:204-221)
    StateArray goal_clipped = BatchPRM::flatten(goal);
    for (int a = 0; a < 3; ++a) goal_clipped[a] = clamp(goal_clipped[a], a);
    // height, roll, pitch from the map (:224-238)
    if (map_->isInside(goal_clipped[0], goal_clipped[1])) {
      double xyzrpy[6] = {goal_clipped[0], goal_clipped[1], 0, 0, 0, yawOfFlat(goal_clipped.data())};
      get3DPoseFrom2D(xyzrpy);
      goal_clipped[2] = xyzrpy[2];
      setFlatRotationFromRPY(goal_clipped.data(), xyzrpy + 3);
    }
    solved_ = false;
    StateArray start_valid = start_flat, goal_valid = goal_clipped;
    const auto& sg = params_->planner.start_goal_search;
    if (!searchValid(start_flat, sg.start_radius, sg.n_iter, 0x5741u, &start_valid)) return PlannerStatus::INVALID_START;
    if (!searchValid(goal_clipped, sg.goal_radius, sg.n_iter, 0x474fu, &goal_valid)) return PlannerStatus::INVALID_GOAL;
    if (tree_) {  // rrt_star / inf_rrt_star / rrt_sharp: a fresh tree per call, grown for plan_time
      try {
        solved_ = tree_->plan(start_valid, goal_valid, params_->planner.plan_time, &path_, &cost_);
      } catch (const std::exception& e) {
        std::cout << e.what() << std::endl;
        solved_ = false;
      }
      return solved_ ? PlannerStatus::SOLVED : PlannerStatus::NOT_SOLVED;
    }
    try {
      if (rb_->built) {
        prm_->setQuery(start_valid, goal_valid);  // clearQuery + new start / goal on the kept graph (:241-242)
      } else {
        prm_->sampleGraph(start_valid, goal_valid);
        rb_->built = true;
      }
      // LazyPRM* keeps growing its roadmap while it has planning time (lazy_prm_star_min_update.cpp:552-615);
      // PRMMotionCost searches the graph sampleGraph built (prm_motion_cost.cpp:440-532)
      if (params_->planner.name == "lazy_prm_star_min_update" || params_->planner.name == "lazy_prm_star")
        solved_ = prm_->solveUntil(params_->planner.plan_time, 1000, &path_, &cost_);
      else
        solved_ = prm_->solve(&path_, &cost_);
    } catch (const MotionCostCallFailed&) {
      throw;   // not ours to absorb (planner.cpp:247 catches ompl::Exception only)
    } catch (const std::exception& e) {  // "All graph edges to goal where actually invalid" (:248-253)
      std::cout << e.what() << std::endl;
      solved_ = false;
      return PlannerStatus::NOT_SOLVED;
    }
    return solved_ ? PlannerStatus::SOLVED : PlannerStatus::NOT_SOLVED;
  }

  // planner.cpp:266-330: throws when the last plan() did not solve; with simplify, the simplified path
  // only when it is valid and not more expensive than the original.
  // (the flattened form; getSolutionPath returns it as it is without OMPL, as an og::PathGeometric with it)
  Path getSolutionPathFlat(const bool& simplify = false) const {
    std::lock_guard<std::mutex> lock(map_mutex_);
    if (!solved_) throw std::runtime_error("Requested failed solution path.");
    if (!simplify) return path_;
    Path simple = path_;
    double cost_simple = cost_;
    try {
      if (tree_)
        tree_->simplify(&simple, &cost_simple);
      else
        prm_->simplify(&simple, &cost_simple);
    } catch (const MotionCostCallFailed&) {
      throw;   // not ours to absorb (planner.cpp:247 catches ompl::Exception only)
    } catch (const std::exception&) {
      std::cout << "Simplified path is invalid. Returning original." << std::endl;
      return path_;
    }
    if (params_->verbose) {
      std::cout << "cost_simple " << cost_simple << std::endl;
      std::cout << "cost_orig " << cost_ << std::endl;
    }
    if (cost_ < cost_simple) {
      if (params_->verbose) std::cout << "Original path cost is lower than simplified. Returning original." << std::endl;
      return path_;
    }
    return simple;
  }

  double getSolutionCost() const { return cost_; }
  const GpuContextPtr& gpu() const { return gpu_; }
  const std::shared_ptr<BatchPRM>& roadmap() const { return prm_; }
  // the tree of the tree planners' last plan() (null for the roadmap planners)
  const std::shared_ptr<BatchTree>& tree() const { return tree_; }

 protected:
  // simplifyCostFieldPaths with map_mutex_ held by the caller (planOnCostField holds it already)
  std::vector<SimplifiedPath> simplifyPathsLocked(artp_field* kept, const std::vector<std::vector<std::array<double, 7>>>& paths,
                                                  unsigned window, artp_field_simplify_stats_t* stats) {
    const size_t n = paths.size();
    std::vector<SimplifiedPath> out(n);
    if (stats) *stats = artp_field_simplify_stats_t{};
    if (!n) return out;
    std::vector<uint64_t> off(n + 1, 0), ooff(n + 1, 0);
    std::vector<double> se3_in;
    for (size_t q = 0; q < n; ++q) {
      for (const auto& s : paths[q]) se3_in.insert(se3_in.end(), s.begin(), s.end());
      off[q + 1] = off[q] + paths[q].size();
    }
    const size_t total = static_cast<size_t>(off[n]);               // never more states come back than went in
    std::vector<int32_t> status(n);
    std::vector<double> cost(n), se3(7 * total + 7);
    std::vector<uint32_t> kept_idx(total + 1);
    artp_field_simplify_params sp{};
    sp.window = window;
    throwOnError(gpu_->get(),
                 artp_field_simplify_paths(kept, &sp, se3_in.data(), off.data(), n, status.data(), cost.data(), ooff.data(),
                                           kept_idx.data(), se3.data(), total + 1),
                 "artp_field_simplify_paths");
    if (stats) throwOnError(gpu_->get(), artp_field_simplify_stats(kept, stats), "artp_field_simplify_stats");
    for (size_t q = 0; q < n; ++q) {
      out[q].status = status[q];
      out[q].cost = cost[q];
      for (uint64_t s = ooff[q]; s < ooff[q + 1]; ++s) {
        out[q].kept.push_back(kept_idx[s]);
        std::array<double, 7> x;
        for (int j = 0; j < 7; ++j) x[j] = se3[7 * s + j];
        out[q].states.push_back(x);
      }
    }
    return out;
  }

  // the tail of both update calls: dist out of the kept field, the layer refreshed
  std::vector<double> refreshCostToGo(artp_field* kept, size_t cells, size_t nodes) {
    const size_t n_yaw = nodes / cells;
    std::vector<double> dist(nodes);
    throwOnError(gpu_->get(), artp_field_dist(kept, dist.data()), "artp_field_dist");
    std::vector<float> best(cells);
    for (size_t i = 0; i < cells; ++i) {
      double b = std::numeric_limits<double>::infinity();
      for (size_t k = 0; k < n_yaw; ++k) b = std::min(b, dist[i * n_yaw + k]);
      best[i] = static_cast<float>(b);
    }
    map_->addLayer("cost_to_go", best.data());
    return dist;
  }

  // artp_field_params of Params::objectives.custom_path_length (computeCostField, computeCostFields, computeCostMatrix)
  artp_field_params costFieldParams() const {
    artp_field_params fp;
    artp_field_params_defaults(&fp);
    const auto& cpl = params_->objectives.custom_path_length;
    fp.objective = cpl.use_directional_cost ? 1 : 0;
    fp.max_lon_vel = cpl.max_lon_vel;
    fp.max_lat_vel = cpl.max_lat_vel;
    fp.max_ang_vel = cpl.max_ang_vel;
    return fp;
  }

  // the tail of both computeCostField calls: dist out of the field, the field kept or destroyed, the layer refreshed
  std::vector<double> finishCostField(artp_field* f, size_t cells, unsigned n_yaw, artp_field** keep) {
    std::vector<double> dist(cells * n_yaw);
    const int rc = artp_field_dist(f, dist.data());
    if (rc || !keep) artp_field_destroy(f);
    throwOnError(gpu_->get(), rc, "artp_field_dist");
    if (keep) *keep = f;   // the caller asks paths of it (artp_field_path) and destroys it
    std::vector<float> best(cells);
    for (size_t i = 0; i < cells; ++i) {
      double b = std::numeric_limits<double>::infinity();
      for (unsigned k = 0; k < n_yaw; ++k) b = std::min(b, dist[i * n_yaw + k]);
      best[i] = static_cast<float>(b);
    }
    map_->addLayer("cost_to_go", best.data());
    return dist;
  }

  ParamsConstPtr params_;
  GpuContextPtr gpu_;
  std::shared_ptr<BatchPRM> prm_;
  std::shared_ptr<BatchTree> tree_;   // rrt_star, inf_rrt_star, rrt_sharp only
  std::shared_ptr<RoadmapHandle> rb_{std::make_shared<RoadmapHandle>()};   // prm_ + "sampleGraph has run", shared with ss_'s planner
  std::shared_ptr<Map> map_;
  mutable std::mutex map_mutex_;
  bool solved_{false};
#ifdef ARTP_PLANNER_REFERENCE_SURFACE
  // planner.h:41-52 -- what PlannerRos reaches into (planner_ros.cpp:242,254,313,359,373)
  std::shared_ptr<og::SimpleSetup> ss_;
  std::shared_ptr<StateSpace> space_;
  std::shared_ptr<StateValidityChecker> checker_;
  std::shared_ptr<BatchMotionValidator> motion_validator_;
  SE3FromSE2SamplerAllocator sampler_allocator_;
  bool freeze_motion_resolution_{false}, motion_resolution_set_{false};
#endif

 private:
  // The three update calls around their library call: `who` = the public method in the exception texts, `what` = the
  // library call in throwOnError's; an empty mask passes only where empty_ok (updateLearnedCostField: unchanged).
  template <class Call>
  std::vector<double> updateKeptField(const char* who, const char* what, artp_field* kept, const std::vector<uint32_t>& mask,
                                      bool empty_ok, Call&& call) {
    std::lock_guard<std::mutex> lock(map_mutex_);
    if (!map_) throw std::runtime_error(std::string(who) + ": the planner does not have a map set");
    if (!kept) throw std::runtime_error(std::string(who) + ": no field");
    const auto g = map_->getGeometry();
    const size_t cells = static_cast<size_t>(g.rows) * g.cols;
    artp_field_stats_t st;
    throwOnError(gpu_->get(), artp_field_stats(kept, &st), "artp_field_stats");
    if ((mask.size() != cells && !(empty_ok && mask.empty())) || st.nodes % cells != 0)
      throw std::runtime_error(std::string(who) + ": the mask or the field does not have rows * cols cells");
    throwOnError(gpu_->get(), call(), what);
    return refreshCostToGo(kept, cells, st.nodes);
  }

  static std::shared_ptr<BatchTree> makeTree(const ParamsConstPtr& params, const GpuContextPtr& gpu) {
    const int variant = BatchTree::variantOf(params->planner.name);
    return variant < 0 ? nullptr : std::make_shared<BatchTree>(params, gpu, variant);
  }

  double clamp(double v, int axis) const { return v < low_[axis] ? low_[axis] : (v > high_[axis] ? high_[axis] : v); }

  // Map::get3DPoseFrom2D (map.cpp:77-90): cell of the position (same arithmetic as the sampler's
  // getIndexOfPosition), its height, and roll / pitch from the cell normal turned into the yaw frame.
  void get3DPoseFrom2D(double* xyzrpy) const {
    const auto g = map_->getGeometry();
    int ri = static_cast<int>(-(((xyzrpy[0] - 0.5 * g.length_x) - g.position_x) / g.resolution));
    int ci = static_cast<int>(-(((xyzrpy[1] - 0.5 * g.length_y) - g.position_y) / g.resolution));
    ri = ri < 0 ? 0 : (ri >= g.rows ? g.rows - 1 : ri);
    ci = ci < 0 ? 0 : (ci >= g.cols ? g.cols - 1 : ci);
    const size_t ind = static_cast<size_t>(ri) + static_cast<size_t>(ci) * g.rows;
    xyzrpy[2] = map_->getLayer(params_->planner.elevation_layer)[ind];
    const double nx = map_->getLayer("normal_x")[ind], ny = map_->getLayer("normal_y")[ind],
                 nz = map_->getLayer("normal_z")[ind];
    const double c = std::cos(xyzrpy[5]), s = std::sin(xyzrpy[5]);
    const double bx = c * nx + s * ny, by = -s * nx + c * ny;  // R_yaw^-1 * n
    xyzrpy[3] = -std::atan2(by, nz);
    xyzrpy[4] = std::atan2(bx, nz);
  }

  // StartState::sampleGoal / GoalStateRegion::sampleGoal: the centre if it is valid, else the first valid of
  // n_iter candidates offset uniformly in a disc of the given radius (x / y only; z and attitude are kept).
  // The reference tests them one by one; here they are ONE batch and the first valid index wins -- the same
  // answer for the same offsets.
  bool searchValid(const StateArray& center, double radius, unsigned n_iter, uint64_t salt, StateArray* out) const {
    std::vector<double> se3(static_cast<size_t>(n_iter + 1) * 7);
    uint64_t x = seed_ * 0x9e3779b97f4a7c15ull + salt;
    auto next01 = [&x]() {  // splitmix64
      uint64_t z = (x += 0x9e3779b97f4a7c15ull);
      z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
      z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
      z ^= z >> 31;
      return static_cast<double>(z >> 11) * (1.0 / 9007199254740992.0);
    };
    for (unsigned i = 0; i <= n_iter; ++i) {
      double ox = 0.0, oy = 0.0;
      if (i > 0) {  // RNG::uniformInBall(r, 2-vector): direction uniform, radius r * u^(1/2)
        const double r = radius * std::sqrt(next01()), a = 2.0 * M_PI * next01();
        ox = r * std::cos(a);
        oy = r * std::sin(a);
      }
      double* s = &se3[static_cast<size_t>(i) * 7];
      for (int k = 0; k < 7; ++k) s[k] = center[k];
      s[0] += ox;
      s[1] += oy;
    }
    std::vector<uint8_t> valid(n_iter + 1);
    throwOnError(gpu_->get(), artp_validate_states(gpu_->get(), se3.data(), valid.size(), valid.data(), nullptr),
                 "artp_validate_states");
    for (unsigned i = 0; i <= n_iter; ++i) {
      if (valid[i]) {
        *out = center;
        (*out)[0] = se3[static_cast<size_t>(i) * 7];
        (*out)[1] = se3[static_cast<size_t>(i) * 7 + 1];
        if (i > 0 && params_->verbose)
          std::cout << "Found valid state offset by " << (*out)[0] - center[0] << " " << (*out)[1] - center[1]
                    << std::endl;
        return true;
      }
    }
    return false;
  }

  artp_preprocessed* pre_{nullptr};
  double low_[3]{0, 0, 0}, high_[3]{0, 0, 0};
  Path path_;
  double cost_{0.0};
  uint64_t seed_{42};
};

}  // namespace art_planner
